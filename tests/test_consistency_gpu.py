"""Degradation-consistency loss on the GPU: ops.degrade_valid (csrc/consistency.hip) and its adjoint against the float64 twin
with the stock-torch fp32 composition on the same device as the yardstick, against the real 8-bit tile degrader, and the
handlers' training steps, eager and replayed from a hipGraph."""
import itertools

import numpy as np
import pytest
import torch

from sisr_amd import architectures as A
from sisr_amd import consistency, degrade, handlers, hip, ops

import _consistency as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _cases():
    """(B, C, s, l, h, w), LR sizes: every scale with every blur edge on small odd tiles; the non-square 13 x 20; the 1-output
    tile; per axis one below, at and one above the forward kernel's workgroup tile edge (in kept outputs) -- whose HR sizes
    92, 96, 100 also lie below, at and above a multiple of the adjoint kernel's edge --; and tiles whose HR side is that edge
    itself, one LR pixel less and one more."""
    T, TB = ops.degrade_valid_tile(), ops.degrade_valid_tile(backward=True)
    out = []
    for n, (s, l) in enumerate(itertools.product((2, 3, 4), (1, 7, 21))):
        m = degrade.consistency_margin(s, l)
        out.append((2, (1, 3)[n % 2], s, l, 2 * m + 3, 2 * m + 6))
    m = degrade.consistency_margin(4, 21)
    out.append((2, 3, 4, 21, 13, 20))
    out += [(2, 1, 4, 21, 2 * m + 1, 2 * m + 1), (2, 3, 2, 7, 2 * degrade.consistency_margin(2, 7) + 1, 2 * degrade.consistency_margin(2, 7) + 1)]
    out += [(2, 1, 4, 21, 2 * m + T - 1, 2 * m + T), (2, 3, 4, 21, 2 * m + T, 2 * m + T + 1), (2, 1, 4, 21, 2 * m + T + 1, 2 * m + T - 1)]
    assert TB % 2 == 0
    out += [(2, 1, 2, 1, TB // 2, TB // 2 + 1), (2, 3, 2, 1, TB // 2 - 1, TB // 2)]
    return out


def _id(c):
    return "B%dC%d-s%d-l%d-%dx%d" % c


def _hip(x, K, s, g):
    x = x.to(DEV).requires_grad_(True)
    y = ops.degrade_valid(x, K.to(DEV), s)
    (dx,) = torch.autograd.grad(y, x, g.to(DEV))
    return y.detach(), dx


def _stock(x, k, s, g):
    x = x.to(DEV).requires_grad_(True)
    y = S.stock(x, k.float().to(DEV), s)
    (dx,) = torch.autograd.grad(y, x, g.to(DEV))
    return y.detach(), dx


@pytest.fixture(scope="module")
def runs():
    """per case, computed once and never modified: fp32 inputs, (value, adjoint of g) of the float64 twin on the host, of the
    stock fp32 composition on the device and of the HIP operator"""
    out = {}
    for n, case in enumerate(_cases()):
        B, C, s, l, h, w = case
        m = degrade.consistency_margin(s, l)
        k = S.kernels(B, l, seed=n).float().double()  # fp32 values, as the loaders ship them: twin, yardstick and operator see the same
        x = S.image(B, C, s * h, s * w, seed=100 + n).float()
        g = torch.randn(B, C, h - 2 * m, w - 2 * m, generator=torch.Generator().manual_seed(200 + n))
        K = torch.from_numpy(degrade.compose_degradation(k.numpy(), s)[0])
        x64 = x.double().requires_grad_(True)
        y64 = S.twin(x64, k, s)
        (d64,) = torch.autograd.grad(y64, x64, g.double())
        out[_id(case)] = dict(x=x, g=g, k=k, K=K, s=s, ref=(y64.detach(), d64), stock=_stock(x, k, s, g), hip=_hip(x, K, s, g))
    torch.cuda.synchronize()
    return out


IDS = [_id(c) for c in _cases()]


@pytest.mark.parametrize("cid", IDS)
def test_forward_and_adjoint_within_twice_the_stock_fp32_error(runs, cid):
    """|hip - twin| <= 2 |stock - twin| in relative L2 and in max-abs, forward and gradient; the factor covers a different
    summation order and nothing else.  The kernels accumulate in float64 over the float64 composed kernel and round once, so each
    element is the fp32 number nearest the exact sum, which no fp32 composition can beat.  Measured on an MI355X over these cases
    (hip / stock): relative L2 forward 8.9e-09 .. 3.1e-08 / 8.9e-09 .. 9.9e-08, gradient 2.4e-08 .. 2.9e-08 / 3.7e-08 .. 1.2e-07;
    max-abs forward <= 3.0e-08 / <= 1.7e-07, gradient <= 3.0e-08 / <= 8.0e-08; never above the stock figure, equal to it at
    the 1-output tile (DESIGN.md 6y has the same pairs)."""
    r = runs[cid]
    for what, i in (("forward", 0), ("gradient", 1)):
        ref, st, hp = r["ref"][i], r["stock"][i], r["hip"][i]
        assert hp.dtype == torch.float32 and hp.shape == ref.shape and hp.is_contiguous()
        e_l2, s_l2, e_max, s_max = S.rel_l2(hp, ref), S.rel_l2(st, ref), S.max_abs(hp, ref), S.max_abs(st, ref)
        print(f"{cid} {what}: rel L2 hip {e_l2:.3e} stock {s_l2:.3e}; max abs hip {e_max:.3e} stock {s_max:.3e}")
        assert e_l2 <= 2 * s_l2, (what, e_l2, s_l2)
        assert e_max <= 2 * s_max, (what, e_max, s_max)


@pytest.mark.parametrize("cid", IDS)
def test_adjoint_identity(runs, cid):
    """<D x, g> and <x, D^T g>, both summed in float64 from the fp32 outputs, under the same measured bound: an operator pair
    within 2 e_f and 2 e_b of the exact one (e: the stock composition's measured relative L2 errors) can differ by at most
    2 e_f |y| |g| + 2 e_b |x| |dx| (Cauchy-Schwarz), the exact pair by nothing"""
    r = runs[cid]
    x, g = r["x"].double(), r["g"].double()
    y, dx = (t.double().cpu() for t in r["hip"])
    a, b = float((y * g).sum()), float((x * dx).sum())
    e_f, e_b = S.rel_l2(r["stock"][0], r["ref"][0]), S.rel_l2(r["stock"][1], r["ref"][1])
    bound = 2 * e_f * float(y.norm() * g.norm()) + 2 * e_b * float(x.norm() * dx.norm())
    print(f"{cid}: <Dx, g> {a:.9e} <x, D^T g> {b:.9e} diff {abs(a - b):.3e} bound {bound:.3e}")
    assert abs(a - b) <= bound
    ya, da = (t.double() for t in r["ref"])
    assert abs(float((ya * g).sum()) - float((x * da).sum())) <= 1e-12 * abs(a)  # the twin's own pair is exact


@pytest.mark.parametrize("cid", IDS)
def test_dx_is_complete_and_repeats_bit_for_bit(runs, cid):
    """the adjoint kernel run straight into a buffer pre-filled with NaN: finite everywhere, zero outside all footprints, equal
    to the operator's gradient; a second run of both kernels gives the same bits"""
    r = runs[cid]
    x, g, K, s = r["x"].to(DEV), r["g"].to(DEV), r["K"].to(DEV), r["s"]
    B, C, H, W = x.shape
    n = K.shape[1]
    _, m, off = degrade.consistency_geometry(s, n)
    ho, wo = g.shape[2:]
    dx = torch.full((B, C, H, W), float("nan"), device=DEV)
    L = hip.lib()
    hip.check(L.sisr_degrade_valid_bwd(hip.ptr(g), K.data_ptr(), hip.ptr(dx), B, C, H, W, n, s, off, ho, wo, hip.stream()), "bwd")
    assert bool(torch.isfinite(dx).all())
    assert torch.equal(dx, r["hip"][1])
    covered = torch.zeros(H, W, dtype=torch.bool)
    covered[off:off + s * (ho - 1) + n, off:off + s * (wo - 1) + n] = True
    assert bool((dx.cpu()[:, :, ~covered] == 0).all())
    assert (int((~covered).sum()) > 0) == (off > 0)  # off = 0 (s = 4 at l = 21, s = 2 at l = 7): the footprints cover the tile
    y2, dx2 = _hip(r["x"], r["K"], s, r["g"])
    assert torch.equal(y2, r["hip"][0]) and torch.equal(dx2, r["hip"][1])


def test_l1_wrapper_gradient():
    """gamma-less core of the loss term, ops.l1_loss(ops.degrade_valid(x, K, s), lr) with lr drawn independently of x: value and
    gradient against the float64 twin under the measured bound.  The seed is one for which no |D(x) - lr| is below 1e-4 in
    float64 (asserted here, on the host), so no element sits near the kink, fp32 and float64 agree on every sign and no element
    is left out.  B C ho wo = 128, so the mean's 1 / N is exact in fp32."""
    s, l, h = 4, 21, 16
    k = S.kernels(2, l, seed=5).float().double()
    x = S.image(2, 1, s * h, s * h, seed=6).float()
    lr = torch.rand(2, 1, h - 8, h - 8, generator=torch.Generator().manual_seed(11))
    K = torch.from_numpy(degrade.compose_degradation(k.numpy(), s)[0])
    x64 = x.double().requires_grad_(True)
    d64 = S.twin(x64, k, s)
    gap = float((d64 - lr.double()).abs().min())
    assert gap >= 1e-4, gap
    v64 = (d64 - lr.double()).abs().mean()
    (g64,) = torch.autograd.grad(v64, x64)

    def run(fn):
        xd = x.to(DEV).requires_grad_(True)
        v = fn(xd)
        (gd,) = torch.autograd.grad(v, xd)
        return v.detach(), gd

    vs, gs = run(lambda t: (S.stock(t, k.float().to(DEV), s) - lr.to(DEV)).abs().mean())
    vh, gh = run(lambda t: ops.l1_loss(ops.degrade_valid(t, K.to(DEV), s), lr.to(DEV)))
    e_v, s_v = abs(float(vh) - float(v64)), abs(float(vs) - float(v64))
    e_g, s_g, e_m, s_m = S.rel_l2(gh, g64), S.rel_l2(gs, g64), S.max_abs(gh, g64), S.max_abs(gs, g64)
    print(f"l1 wrapper: min gap {gap:.2e}; value hip {e_v:.3e} stock {s_v:.3e}; gradient rel L2 hip {e_g:.3e} stock {s_g:.3e}; "
          f"max abs hip {e_m:.3e} stock {s_m:.3e}")
    assert e_g <= 2 * s_g and e_m <= 2 * s_m
    # the value: one fp32 mean of 128 terms either way; an fp32 result cannot be held tighter than a unit by a yardstick that
    # may land on the nearest number by luck
    assert e_v <= max(2 * s_v, 2.0 ** -23 * float(v64))


def test_frozen_input_kept_gradient_and_kernel_without_gradient(runs):
    """the node's autograd contract: an input that needs no gradient gives a result that needs none; a non-leaf input gets the
    adjoint through the chain (d / da of <D(a x), g> is <D^T g, x>); a kept .grad is added to, not replaced; K never takes a
    gradient"""
    r = runs[IDS[9]]
    x, g, K, s = r["x"].to(DEV), r["g"].to(DEV), r["K"].to(DEV), r["s"]
    assert not ops.degrade_valid(x, K, s).requires_grad
    a = torch.ones((), device=DEV, requires_grad=True)
    (ops.degrade_valid(a * x, K, s) * g).sum().backward()
    want = float((r["hip"][1].double() * x.double()).sum())
    assert abs(float(a.grad) - want) <= 1e-5 * abs(want)
    xl = x.clone().requires_grad_(True)
    for _ in range(2):
        ops.degrade_valid(xl, K, s).backward(g)
    assert torch.equal(xl.grad, 2 * r["hip"][1])
    with pytest.raises(RuntimeError, match="no gradient"):
        ops.degrade_valid(x, K.clone().requires_grad_(True), s)


# ----------------------------------------------------------------------------- against the real degrader
def test_kept_pixels_match_the_8_bit_tile_degrader():
    """degrade.degrade_tiles (the Pillow-exact 8-bit pipeline, flips on) against ops.degrade_valid on the matching HR tiles with
    the kernels composed for the same flips, all eight flag combinations, tiles at the image corner included.  The image lies in
    [0.25, 0.75], so nothing clips.  Every kept pixel within (A (A + 1/2) + 1/2) / 255 plus the fp32 slack: A = 1.171875 is the
    absolute tap sum at s = 4, from the table; the blur's truncation to a byte (< 1) goes through both passes, the halves are
    the two roundings."""
    s, crop, l = 4, 12, 21
    m = degrade.consistency_margin(s, l)
    A_ = S.abs_tap_sum(s)
    assert A_ == 1.171875
    flips = list(itertools.product((0, 1), repeat=3))
    gen = torch.Generator().manual_seed(3)
    smooth = torch.nn.functional.interpolate(torch.rand(2, 3, 18, 20, generator=gen), size=(144, 160), mode="bicubic", align_corners=False)
    images = [(0.25 + 0.5 * (t - t.min()) / (t.max() - t.min())).contiguous().to(DEV) for t in smooth]
    assert all(0.25 <= float(t.min()) and float(t.max()) <= 0.75 for t in images)
    k = S.kernels(8, l, seed=21)
    origins = [(0, 0), (24, 28), (5, 17), (24, 0), (0, 28), (11, 3), (7, 7), (20, 20)]  # of the un-augmented LR tiles, in a 36 x 40 LR image
    per = [images[b % 2] for b in range(8)]
    lr = degrade.degrade_tiles(per, k.float(), origins, crop, s, flips=flips)
    assert lr.shape == (8, 3, crop, crop)
    hr = torch.stack([S.augment(per[b][:, s * ty:s * (ty + crop), s * tx:s * (tx + crop)], flips[b]) for b, (ty, tx) in enumerate(origins)])
    k64 = k.float().double()  # the degrader receives the kernels in fp32
    K = torch.from_numpy(degrade.compose_degradation(k64.numpy(), s, np.array(flips))[0])
    got = ops.degrade_valid(hr.contiguous(), K.to(DEV), s)
    turned = torch.from_numpy(degrade.flip_kernels(k64.numpy(), np.array(flips)))
    ref = S.twin(hr.double().cpu(), turned, s)
    slack = 2 * S.max_abs(S.stock(hr.contiguous(), turned.float().to(DEV), s), ref)  # the fp32 slack, measured as above
    diff = (got.double().cpu() - lr[:, :, m:crop - m, m:crop - m].double().cpu()).abs()
    bound = (A_ * (A_ + 0.5) + 0.5) / 255 + slack
    print(f"against degrade_tiles: max |diff| {float(diff.max()) * 255:.3f} / 255, mean {float(diff.mean()) * 255:.3f} / 255, "
          f"bound {bound * 255:.3f} / 255 (fp32 slack {slack:.2e})")
    assert got.shape == (8, 3, crop - 2 * m, crop - 2 * m)
    assert float(diff.max()) <= bound
    # the kernel's orientation matters: with the un-flipped kernels the flipped tiles miss the bound
    plain = ops.degrade_valid(hr.contiguous(), torch.from_numpy(degrade.compose_degradation(k64.numpy(), s)[0]).to(DEV), s)
    off = (plain.double().cpu() - lr[:, :, m:crop - m, m:crop - m].double().cpu()).abs().amax(dim=(1, 2, 3))
    print("un-flipped kernels, per sample max |diff| * 255:", [round(float(v) * 255, 2) for v in off])
    assert float(off[0]) <= bound and float(off[1:].max()) > bound


# ----------------------------------------------------------------------------- handlers
class _SmallRCANHandler(handlers.BaseModel):
    """RCANHandler around a reduced RCAN: one group, one block, 16 features, x4"""

    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, perceptual=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = A.RCAN(n_resblocks=1, n_resgroups=1, n_feats=16, scale=4)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.training_setup(lr, None, None, perceptual, device)
        self.model_name = 'rcan'


def _small_qrcan(tmp_path, **kw):
    return handlers.QRCANHandler(device=0, model_save_dir=str(tmp_path), eval_mode=False, scale=4, style="standard", n_resblocks=1,
                                 n_resgroups=1, n_feats=16, include_q_layer=True, metadata=["blur_kernel"], **kw)


def _batch(step, B=2):
    """an online batch as the loaders hand it over: 24 x 24 LR tiles, their 96 x 96 HR tiles, kernels and flags"""
    g = torch.Generator().manual_seed(50 + step)
    flips = torch.tensor([[(step + b) & 1, (step + b) >> 1 & 1, (step + 2 * b) >> 2 & 1] for b in range(B)])
    return dict(x=torch.rand(B, 3, 24, 24, generator=g), y=torch.rand(B, 3, 96, 96, generator=g),
                blur_kernels=S.kernels(B, 21, seed=60 + step).float(), flips=flips)


def _twin_loss(out, b, gamma):
    """base + gamma * twin, float64, from the step's returned output"""
    o = out.detach().double().cpu()
    k = torch.from_numpy(degrade.flip_kernels(b["blur_kernels"].double().numpy(), b["flips"].numpy()))
    term = (S.twin(o, k, 4) - b["x"].double()[:, :, 4:20, 4:20]).abs().mean()
    base = (o - b["y"].double()).abs().mean()
    return float(base + gamma * term), float(base), float(term)


@pytest.mark.parametrize("kind", ["rcan", "qrcan"])
def test_handler_trains_with_the_term_eager_and_graphed(tmp_path, kind):
    """three train_steps at B = 2, 24 x 24 LR -> 96 x 96, consistency_loss = 0.5, each with other kernels and flags, eager and
    replayed from a hipGraph.  Every loss -- the second and third replays read kernels and flags the capture never saw: the
    static buffer is refreshed -- equals base + gamma * twin of the returned output within the operator's bound (the operator
    and both L1 means are fp32 numbers nearest their float64 values or a few units off: 1e-6 relative); the graphed trajectory
    equals the eager one as tests/test_freq_loss_gpu.py holds its term (1e-6 absolute per loss, 1e-5 on the parameter sum); the
    binding is gone after every step; run_eval(request_loss=True) after the steps returns the base loss alone."""
    gamma = 0.5
    md = torch.rand(2, 10, generator=torch.Generator().manual_seed(1)) * 0.4
    extra = dict(metadata=md, metadata_keys=[("blur_kernel", "blur_kernel")] * 10) if kind == "qrcan" else {}
    runs = {}
    for mode in (False, True):
        torch.manual_seed(8)
        h = (_SmallRCANHandler(device=0, model_save_dir=str(tmp_path), consistency_loss=gamma) if kind == "rcan"
             else _small_qrcan(tmp_path, consistency_loss=gamma))
        h.use_graph = mode
        assert isinstance(h.criterion, consistency.ConsistencyMechanism) and type(h.criterion.base) is handlers.L1Loss
        ls = []
        for step in range(3):
            b = _batch(step)
            loss, out = h.train_step(b["x"], b["y"], blur_kernels=b["blur_kernels"], flips=b["flips"], **extra)
            want, base, term = _twin_loss(out, b, gamma)
            print(f"{kind} graph={mode} step {step}: loss {float(loss):.8f} float64 {want:.8f} (base {base:.6f} term {term:.6f})")
            assert abs(float(loss) - want) <= 1e-6 * want, (step, float(loss), want)
            assert term > 1e-3 and h.criterion._bound is None
            ls.append(float(loss))
        assert bool(h._graphs) == mode and (not mode or len(h._graphs) == 1)
        runs[mode] = (ls, float(sum(p.detach().double().sum() for p in h.net.parameters())))
        b = _batch(7)
        out, eval_loss, _ = h.run_eval(b["x"], b["y"], request_loss=True, keep_on_device=True, **extra)
        base = float((out.double().cpu() - b["y"].double()).abs().mean())
        assert abs(float(eval_loss) - base) <= 1e-6 * base, (float(eval_loss), base)
    assert np.allclose(runs[True][0], runs[False][0], rtol=0, atol=1e-6), runs
    assert abs(runs[True][1] - runs[False][1]) < 1e-5


def test_unset_key_leaves_the_step_bit_identical(tmp_path):
    """a handler built with consistency_loss unset or 0 takes the same steps, bit for bit, as one built without the key -- also
    when the batch carries kernels and flags"""
    outs = []
    for kw, feed in (({}, False), ({"consistency_loss": None}, True), ({"consistency_loss": 0}, True)):
        torch.manual_seed(8)
        h = _SmallRCANHandler(device=0, model_save_dir=str(tmp_path), **kw)
        assert type(h.criterion) is handlers.L1Loss
        got = []
        for step in range(2):
            b = _batch(step)
            more = dict(blur_kernels=b["blur_kernels"], flips=b["flips"]) if feed else {}
            loss, out = h.train_step(b["x"], b["y"], **more)
            got += [loss.cpu(), out.cpu()]
        outs.append(got + [p.detach().cpu().clone() for p in h.net.parameters()])
    for other in outs[1:]:
        assert len(other) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(outs[0], other))


def test_srmd_input_carries_metadata_planes_behind_the_image(tmp_path):
    """SRMD's x is the LR image with its metadata maps concatenated: the term reads the first three planes"""
    import sisr_amd
    gamma = 0.5
    torch.manual_seed(8)
    h = sisr_amd.srmd.SRMDHandler(device=0, model_save_dir=str(tmp_path), eval_mode=False, consistency_loss=gamma, metadata=["blur_kernel"],
                                  nb=1, nc=64, scale=4)
    b = _batch(1)
    md = torch.rand(2, 10, generator=torch.Generator().manual_seed(1)) * 0.4
    loss, out = h.train_step(b["x"], b["y"], metadata=md, metadata_keys=[("blur_kernel", "blur_kernel")] * 10,
                             blur_kernels=b["blur_kernels"], flips=b["flips"])
    want, base, term = _twin_loss(out, b, gamma)
    print(f"srmd: loss {float(loss):.8f} float64 {want:.8f} (base {base:.6f} term {term:.6f})")
    assert abs(float(loss) - want) <= 1e-6 * want
