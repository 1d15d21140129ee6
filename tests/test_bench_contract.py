"""bench.py prints exactly one JSON line with the contract's fields (pytest -m gpu; small workload so it runs in
seconds: EDSR-baseline, 2 timed steps, batch 4)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--batch", "4", "--workload", "edsr", "--full"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["unit"] == "patches/s" and d["value"] > 0 and abs(d["value"] - 4 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["value"] > 0 and c["cores"] >= 1


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_alone():
    """Without --full the default run times its steps and prints the line: the contract's fields and the roofline derived from
    the headline, no kernel-timing step, no side measurement, no CPU baseline."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "LR-patches/sec (128x128x3, x4) fwd+bwd" and d["unit"] == "patches/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 1 and d["warmup"] == 0 and d["config"]["per_gpu_batch"] == 32
    assert d["value"] > 0 and abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["families"] == [] and r["kernel"] is None
    for k in ("cpu_baseline", "meta_rcan", "config4_point", "han_bf16", "meta_edsr", "b1_point", "sparnet", "inference", "bf16x3"):
        assert k not in d, k


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_steps_outputs(tmp_path):
    """--dump-outputs DIR: the loss and SR output of the last timed step as float .npy files, named on the JSON line."""
    import numpy as np
    d = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--batch", "2", "--workload", "edsr", "--no-cpu-baseline", "--no-kernel-timing", "--dump-outputs", str(d)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["dump_outputs"]["arrays"] == {"loss": {"shape": [], "elements_written": 1},
                                              "out": {"shape": [2, 3, 512, 512], "elements_written": 2 * 3 * 512 * 512}}
    loss, sr = np.load(d / "loss.npy"), np.load(d / "out.npy")
    assert loss.dtype == np.float32 and sr.dtype == np.float32 and sr.shape == (2, 3, 512, 512)
    assert np.isfinite(sr).all() and abs(float(loss) - line["config"]["final_loss"]) < 1e-7


def test_dump_outputs_keeps_to_its_budget_with_a_fixed_sample(tmp_path):
    """A large output is written as the same seeded element sample every time; small arrays whole; 64 MB in all."""
    import numpy as np
    import bench
    rng = np.random.default_rng(0)
    arrays = {"loss": np.array(0.25, np.float32), "out": rng.random((20, 3, 512, 512), dtype=np.float32),
              "stat": rng.random(7)}
    info = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 * 10 ** 6
    assert info["loss"] == {"shape": [], "elements_written": 1} and info["stat"]["elements_written"] == 7
    assert 0 < info["out"]["elements_written"] < arrays["out"].size
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.isin(a[:1000], arrays["out"]).all()
    assert np.load(tmp_path / "a" / "stat.npy").dtype == np.float64 and np.load(tmp_path / "a" / "loss.npy").shape == ()


@pytest.mark.gpu
def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher and no WORLD_SIZE: bench.py spawns its two ranks as a child
    torch.distributed.run (never exec) and relays rank 0's single JSON line.  Rehearsed on the one GPU of this box: both ranks
    on cuda:0, gloo transport; the default N > 1 workload = BASELINE config 4 (QRCAN, global batch 32, strong scaling,
    hipGraph replay), with --full's weak-scaling object and watchdogged overlapped-exchange object beside it."""
    env = dict(os.environ, SISR_BENCH_SHARE_GPU="1", SISR_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"],
                         capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 2 and d["warmup"] == 1
    assert d["config"]["global_batch"] == 32 and d["config"]["per_gpu_batch"] == 16 and d["value"] > 0
    assert "grad_exchange" in d["config"] and d["config"]["grad_exchange"]
    w = d["weak_scaling"]
    assert w.get("per_gpu_batch") == 32 and w.get("global_batch") == 64 and w["value"] > 0, w
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1


@pytest.mark.gpu
def test_bench_refuses_a_world_size_mismatch():
    """Inside a launcher's world the --gpus flag must agree with it."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and "torch.distributed.run" in (out.stderr + out.stdout)
