"""Time the geometric self-ensemble (ensemble.py, csrc/ensemble.hip) against the form a user writes by hand with torch ops.

(a) The kernel pair.  sisr_dihedral_fan on an LR batch and sisr_dihedral_merge on the matching SR batches, against the
    torch-op form on the same tensors: eight flip / transpose / contiguous copies for the fan; eight inverse flip /
    transpose views, a stack and a mean for the merge.  HIP events around each form, all four timed in turn within every
    repeat (so drift hits them alike), after a warm-up; median and spread (min, p10, p90, max).
    Bytes: the algorithm needs 9 x the input for fan (read once, written eight times) and 9 x the output for merge (eight
    read, one written).  The kernels issue exactly those accesses -- every element is read once and written once per
    variant, nothing is staged through memory -- so their issued bytes equal the algorithmic bytes by construction; hardware
    counters were not collected.  The rate is those bytes over the median time; at these sizes (7 MB .. 100 MB, under the
    256 MiB Infinity Cache) it is not an HBM rate, so no share of an HBM peak is claimed.
(b) A full-depth RCAN x4 run_eval of one 339 x 510 image: plain; the hand-made ensemble (eight batch-1 run_eval calls with
    the torch ops around them); run_eval(self_ensemble=True) (two batch-4 forwards between the two kernels).  Host clock
    around calls that end in a device synchronise, the two ensemble forms alternating.

    python tools/ensemble_bench.py [--reps 200] [--net-reps 5] [--out profiles/ensemble_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLIPS = ((), (-1,), (-2,), (-2, -1))


def _spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), p10=float(np.percentile(v, 10)),
                p90=float(np.percentile(v, 90)), max=float(v.max()))


def torch_fan(x):
    """the eight variants as eight contiguous copies (the first is the input itself)"""
    return [(b.flip(*d) if d else b).contiguous() for b in (x, x.transpose(-1, -2)) for d in FLIPS]


def torch_merge(outs):
    """outs: the eight network outputs in variant order -> each mapped back, stacked, averaged"""
    import torch
    back = []
    for k, o in enumerate(outs):
        o = o.flip(*FLIPS[k % 4]) if FLIPS[k % 4] else o
        back.append(o.transpose(-1, -2) if k >= 4 else o)
    return torch.stack(back).mean(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--net-reps", type=int, default=5)
    ap.add_argument("--net-warmup", type=int, default=2)
    ap.add_argument("--skip-net", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    a = ap.parse_args()
    import torch
    import sisr_amd
    E = sisr_amd.ensemble
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench needs a HIP device")
    g = torch.Generator().manual_seed(0)
    kernels = []
    for name, (n, c, h, w), scale in (("div2k_339x510_x4", (1, 3, 339, 510), 4), ("128x128_x4", (1, 3, 128, 128), 4)):
        H, W = h * scale, w * scale
        x = torch.rand((n, c, h, w), generator=g).cuda()
        up, tu = torch.rand((4 * n, c, H, W), generator=g).cuda(), torch.rand((4 * n, c, W, H), generator=g).cuda()
        outs = [up[k * n:(k + 1) * n] for k in range(4)] + [tu[k * n:(k + 1) * n] for k in range(4)]
        forms = {"kernel_fan": lambda: E.dihedral_fan(x), "torch_fan": lambda: torch_fan(x),
                 "kernel_merge": lambda: E.dihedral_merge(up, tu), "torch_merge": lambda: torch_merge(outs)}
        # the two forms compute the same thing (the torch mean sums in another order)
        ku, kt = forms["kernel_fan"]()
        tv = forms["torch_fan"]()
        assert torch.equal(ku, torch.cat(tv[:4])) and torch.equal(kt, torch.cat(tv[4:]))
        merge_diff = float((forms["kernel_merge"]() - forms["torch_merge"]()).abs().max())
        for _ in range(a.warmup):
            for f in forms.values():
                f()
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
              for k in forms}
        for i in range(a.reps):
            for k, f in forms.items():
                ev[k][i][0].record()
                f()
                ev[k][i][1].record()
        torch.cuda.synchronize()
        us = {k: np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in v]) for k, v in ev.items()}
        fan_bytes, merge_bytes = 9 * n * c * h * w * 4, 9 * n * c * H * W * 4
        r = dict(case=name, input=[n, c, h, w], merged=[n, c, H, W], reps=a.reps, warmup=a.warmup,
                 us={k: _spread(v) for k, v in us.items()},
                 pair_us=dict(kernel=_spread(us["kernel_fan"] + us["kernel_merge"]),
                              torch=_spread(us["torch_fan"] + us["torch_merge"])),
                 fan_algorithmic_bytes=fan_bytes, fan_issued_bytes=fan_bytes,
                 merge_algorithmic_bytes=merge_bytes, merge_issued_bytes=merge_bytes,
                 fan_gbs=fan_bytes / (float(np.median(us["kernel_fan"])) * 1e-6) / 1e9,
                 merge_gbs=merge_bytes / (float(np.median(us["kernel_merge"])) * 1e-6) / 1e9,
                 merge_max_abs_kernel_minus_torch=merge_diff)
        r["torch_over_kernel"] = r["pair_us"]["torch"]["median"] / r["pair_us"]["kernel"]["median"]
        kernels.append(r)
        print(f"{name:>18}: fan {r['us']['kernel_fan']['median']:7.1f} us (torch {r['us']['torch_fan']['median']:7.1f})  "
              f"merge {r['us']['kernel_merge']['median']:7.1f} us (torch {r['us']['torch_merge']['median']:7.1f})  "
              f"pair x{r['torch_over_kernel']:.2f}  fan {r['fan_gbs']:.0f} GB/s  merge {r['merge_gbs']:.0f} GB/s", flush=True)
    doc = dict(tool="tools/ensemble_bench.py", device=torch.cuda.get_device_name(0), kernels=kernels)

    if not a.skip_net:
        torch.manual_seed(8)
        h = sisr_amd.available_models["rcan"](device=0, model_save_dir="/tmp", eval_mode=True, scale=4)
        x = torch.rand((1, 3, 339, 510), generator=g).cuda()

        def plain():
            return h.run_eval(x, keep_on_device=True)[0]

        def hand():
            outs = [h.run_eval(v, keep_on_device=True)[0] for v in torch_fan(x)]
            return torch_merge(outs)

        def plus():
            return h.run_eval(x, keep_on_device=True, self_ensemble=True)[0]

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        for _ in range(a.net_warmup):
            for f in (plain, hand, plus):
                f()
        secs = {"plain": [], "hand_made_8_calls": [], "self_ensemble": []}
        for _ in range(a.net_reps):
            for k, f in (("plain", plain), ("hand_made_8_calls", hand), ("self_ensemble", plus)):
                s, out = timed(f)
                secs[k].append(s)
                if k == "hand_made_8_calls":
                    ref = out
                elif k == "self_ensemble":
                    diff = float((out - ref).abs().max())
        net = dict(model="rcan x4, full depth (10 groups x 20 blocks, 64 features)", input=[1, 3, 339, 510],
                   precision=os.environ.get("SISR_PRECISION", "default"), reps=a.net_reps, warmup=a.net_warmup,
                   seconds={k: _spread(v) for k, v in secs.items()},
                   max_abs_self_ensemble_minus_hand_made=diff)
        net["hand_made_over_self_ensemble"] = net["seconds"]["hand_made_8_calls"]["median"] / net["seconds"]["self_ensemble"]["median"]
        net["self_ensemble_over_plain"] = net["seconds"]["self_ensemble"]["median"] / net["seconds"]["plain"]["median"]
        doc["run_eval"] = net
        print(f"rcan x4 339x510: plain {net['seconds']['plain']['median'] * 1e3:.1f} ms  hand-made "
              f"{net['seconds']['hand_made_8_calls']['median'] * 1e3:.1f} ms  self_ensemble "
              f"{net['seconds']['self_ensemble']['median'] * 1e3:.1f} ms  (x{net['hand_made_over_self_ensemble']:.2f}; "
              f"|plus - hand| {diff:.1e})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
