"""Every conv and weight-gradient form against float64 on EXACT data, bit for bit (pytest -m gpu).

Operands are small dyadic rationals (tests/_exact.py): every product is exact and every partial sum fits fp32's
significand, so each correct kernel form returns the exact result whatever its summation order, tiling, K-split or MFMA
type, and the comparison has zero tolerance: `torch.equal(got.double(), exact)`.  Each comparison is preceded by a budget
assertion (a case over budget is a test bug).  Outputs are prefilled with NaN, so an element left unwritten fails.  The
only roundings compared against are the ones a kernel performs on purpose, each said where it is used: bf16-stored outputs
(one round-to-nearest-even of the exact fp32 value) and the LeakyReLU slope 0.2f (one fp32 rounding of v * 0.2f).

Forms are forced with the controls that exist (`select`, SISR_WGRAD_QUADRANT_KERNEL, the queues, set_precision /
set_storage) and shapes sit on both sides of each selection rule, quoted where it is probed.  Each family ends with a
detector check: one input element moved by one granule, in what the kernel sees only, must make the comparison fail at
exactly the outputs that element feeds.
"""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

import _exact as X
import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
CL = torch.channels_last
NAN = float("nan")


def dev4(t, dtype=torch.float32):
    return t.to(DEV, dtype).contiguous(memory_format=CL)


def nan4(B, C, H, W, dtype=torch.float32):
    return torch.full((B, C, H, W), NAN, device=DEV, dtype=dtype).contiguous(memory_format=CL)


def dd(t):
    """float64 copy on the device (where the references run)"""
    return t.to(DEV, torch.float64)


def conv_budget(x, w, extras=(), **kw):
    """_exact.conv_budget evaluated on the device"""
    return X.conv_budget(dd(x), dd(w), extras=[dd(e) for e in extras if e is not None], **kw)


def wgrad_budget(x, dy, **kw):
    return X.wgrad_budget(dd(x), dd(dy), **kw)


@contextlib.contextmanager
def env(name, value):
    prev = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = prev


@contextlib.contextmanager
def precision(name, storage="0"):
    keep = (ops.PRECISION, ops.BF16_STORAGE)
    ops.set_precision(name)
    ops.set_storage(storage)
    try:
        yield
    finally:
        ops.set_precision(keep[0])
        ops.set_storage(keep[1])


def packed_with_transform(w):
    """(forward, input-gradient) packings of a 64 -> 64 weight by the step-level packing launch, Winograd transform
    U = G g G^T included (select 11 / 12 read it behind the direct packing)"""
    plan = ops._PackPlan([(w, 1)], w.device)
    plan.run()
    ops.invalidate_packs()
    pf, pd = plan.slices[0]
    assert pf.numel() == 64 * 64 * 9 + ops.WINOGRAD_FLOATS
    return pf, pd


# ============================================================================ 1. fp32 64-multiple conv (sisr_conv3x3_c64)
# Every epilogue / prologue option the host accepts.  "d" cases use the input-gradient packing (flipped, role-swapped).
CASES = ["bias", "bias_relu_gap", "res_alpha", "mask", "mask_affine", "affine_res", "shift_only", "mask_res", "out_scale",
         "gate_relu", "gate_res", "dot", "dot_res", "leaky", "leaky_mask"]
FP32_ONLY = {"leaky", "leaky_mask"}  # LeakyReLU codes exist on the fp32 kernels only (SFTMD)
BF16_REFUSED = {"shift_only"}  # in_shift without in_scale: the fp32 entry serves it from the general kernel only
# forms with kernels of their own in the bf16 / bf16x3 families only (the fp32 entry serves them from the general kernel)
BF16_EXTRA = ["affine", "mask_affine_res"]


class ConvData:
    """one set of exact operands for a (B, H, W) 64 -> 64 conv; zeros in `m` make ReLU' / LeakyReLU' ties"""

    def __init__(self, B, H, W, seed, x=None):
        self.B, self.H, self.W = B, H, W
        s = (B, 64, H, W)
        self.x = X.ints(s, seed) if x is None else x
        self.w = X.weights((64, 64, 3, 3), seed + 1)
        self.b = X.biases(64, seed + 2)
        self.res, self.skip, self.dot = X.ints(s, seed + 3), X.ints(s, seed + 4), X.ints(s, seed + 5)
        self.m = X.ints(s, seed + 6, zeros=0.3)  # exact zeros at a known share: the ties of the masks
        self.sc, self.sh, self.os = X.scales((B, 64), seed + 7), X.shifts((B, 64), seed + 8), X.scales((B, 64), seed + 9)
        self.dev = {k: dev4(getattr(self, k)) for k in ("x", "res", "skip", "dot", "m")}
        self.dev.update({k: getattr(self, k).to(DEV) for k in ("w", "b", "sc", "sh", "os")})


def conv_case(name, D):
    """-> (packing 'f' | 'd', kwargs for ops.conv_c64, exact y, exact summed partials or None, exact gate_out or None,
    prologue output u (the conv's operand) and the weight it meets, the extra epilogue terms)"""
    B = D.B
    v = lambda t: dd(t).view(B, 64, 1, 1)
    x, w = dd(D.x), dd(D.w)
    wt = w.flip(2, 3).transpose(0, 1)  # the input-gradient packing computes the transposed conv
    b, res, m, dev = dd(D.b).view(1, 64, 1, 1), dd(D.res), dd(D.m), D.dev
    pk, kw, u, wk, gap, gout, extras = "f", {}, x, w, None, None, []
    if name in ("mask", "mask_affine", "mask_res", "leaky_mask", "mask_affine_res"):
        pk, wk = "d", wt
    if name in ("mask_affine", "affine_res", "affine", "mask_affine_res"):
        u = x * v(D.sc) + v(D.sh)
        kw.update(in_scale=dev["sc"], in_shift=dev["sh"])
    if name == "shift_only":
        u = x + v(D.sh)
        kw.update(in_shift=dev["sh"])
    if name in ("gate_relu", "gate_res"):
        u = x * v(D.sc) + dd(D.skip)
        kw.update(in_scale=dev["sc"], gate_add=dev["skip"])
        gout = u
    acc = X.conv_ref(u, wk)
    if name in ("bias", "bias_relu_gap", "affine_res", "shift_only", "out_scale", "gate_relu", "gate_res", "leaky"):
        kw["bias"] = dev["b"]
        acc = acc + b
        extras.append(D.b)
    y = acc
    if name in ("bias_relu_gap", "out_scale", "gate_relu"):
        kw["relu"] = True
        y = F.relu(y)
    if name == "leaky":
        kw["relu"] = ops.LEAKY
        y = X.leaky_ref(y)  # v > 0 ? v : fl32(0.2f * v) -- the kernel's one deliberate rounding
    if name == "res_alpha":
        kw["alpha"] = X.ALPHA
        y = y * X.ALPHA
    if name == "out_scale":
        kw.update(out_scale=dev["os"], alpha=X.ALPHA)
        y = y * (X.ALPHA * v(D.os))
    if name in ("mask", "mask_affine", "mask_res", "mask_affine_res"):
        kw["mask"] = dev["m"]
        y = y * X.relu_mask(m)  # PyTorch's ReLU': 0 where the map is <= 0
    if name == "leaky_mask":
        kw.update(mask=dev["m"], relu=ops.LEAKY_MASK)
        y = X.fp32_round(y * X.leaky_mask(m))  # PyTorch's LeakyReLU': slope where the map is <= 0, one fp32 rounding
    if name in ("res_alpha", "affine_res", "mask_res", "gate_res", "dot_res", "mask_affine_res"):
        kw["res"] = dev["res"]
        y = y + res
        extras.append(D.res)
    if name == "bias_relu_gap":
        gap = y.sum(dim=(2, 3))
    if name in ("dot", "dot_res"):
        kw["dot"] = dev["dot"]
        gap = (y * dd(D.dot)).sum(dim=(2, 3))
    return pk, kw, y, gap, gout, u, wk, extras


def run_conv(x, pk, B, H, W, select, cin=64, cout=64, want_gap=False, want_gout=False, xview=None, y=None, yview=None,
             fn=None, **kw):
    y = nan4(B, cout, H, W) if y is None else y
    gap = torch.full((B, ops.gap_parts(H, W), cout), NAN, device=DEV) if want_gap else None
    gout = nan4(B, 64, H, W) if want_gout else None
    bias = kw.pop("bias", None)
    (fn or ops.conv_c64)(x, xview or hip.view_plain(H, W, cin), pk, bias, (1, 64), y, yview or hip.view_plain(H, W, cout),
                         B, H, W, cin, cout, gap=gap, gate_out=gout, select=select, **kw)
    return y, gap, gout


def check_conv_case(name, D, packs, select, winograd=False, out_cast=None):
    """run one case; returns a failure message or None"""
    pk, kw, y_ref, gap_ref, gout_ref, u, wk, extras = conv_case(name, D)
    conv_budget(u, wk, extras=extras, what=name)
    if winograd:
        X.winograd_budget(u, wk, what=name)
    if gap_ref is not None:
        X.assert_budget((y_ref.abs() * (dd(D.dot).abs() if "dot" in kw else 1)).sum(dim=(2, 3)), X.granule(y_ref), name + " partials")
    y, gap, gout = run_conv(D.dev["x"], packs[0] if pk == "f" else packs[1], D.B, D.H, D.W, select, want_gap=gap_ref is not None,
                            want_gout=gout_ref is not None, **kw)
    try:
        X.assert_exact(y, y_ref, f"{name} output")
        if gap_ref is not None:
            X.assert_exact(gap.double().sum(dim=1), gap_ref, f"{name} partial sums (summed over slots)")
        if gout_ref is not None:
            X.assert_exact(gout, gout_ref, f"{name} gate_out")
    except AssertionError as e:
        return str(e)
    return None


SMALL = [(1, 13, 9), (2, 6, 33), (2, 5, 1), (1, 3, 2), (1, 57, 86), (3, 9, 64)]  # ragged off 4 x 32 and 2 x 32, 1 / 2 wide
# select: 0 default (plain packing), 2 general kernel, 6 per-tile kernel, 7 persistent, 11 / 12 Winograd auto / forced
SELECTS = [0, 2, 6, 7, 11, 12]


@pytest.mark.parametrize("B,H,W", SMALL)
@pytest.mark.parametrize("select", SELECTS)
def test_fp32_conv_every_form_and_option(select, B, H, W):
    D = ConvData(B, H, W, seed=100 + B + H + W)
    packs = packed_with_transform(D.dev["w"]) if select in (11, 12) else ops.pack_pair(D.dev["w"])
    fails = [f for f in (check_conv_case(n, D, packs, select, winograd=select in (11, 12)) for n in CASES) if f]
    assert not fails, "\n".join(fails)


# The shapes at which the shared tile map, tile walk and fp32 halo staging (csrc/conv_tiles.h) take each branch:
#   (3, 8, 64)     12 full 4 x 32 tiles, a workgroup count that is no multiple of 8: the round-robin walk
#   (2, 7, 45)     ragged in both directions
#   (3, 100, 250)  600 tiles on 512 workgroups: the per-XCD walk (75 tiles per XCD, step 64), one or two tiles per workgroup
#   (1, 6, 64)     the tile's second strip is partly outside the image
# (tests/test_conv_w4_epilogue_gpu.py runs the Winograd kernel at the same four.)
WALK = [(3, 8, 64), (2, 7, 45), (3, 100, 250), (1, 6, 64)]


@pytest.mark.parametrize("B,H,W", WALK)
def test_fp32_persistent_conv_tile_walk(B, H, W):
    """conv3x3_c64_p4_kernel (select 7), every form and option, at the WALK shapes"""
    D = ConvData(B, H, W, seed=150 + B + H + W)
    packs = ops.pack_pair(D.dev["w"])
    fails = [f for f in (check_conv_case(n, D, packs, 7) for n in CASES) if f]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B", [7, 8, 9])
def test_fp32_conv_selection_thresholds(B):
    """persistent form: nblk = ceil(H/4)*ceil(W/32)*B >= 1024 (B = 7: 896 per-tile, 8: 1024, 9: 1152 = a ragged last round
    over 512 workgroups); Winograd form (select 11): B*H*W > 8*128^2 (B = 8 direct, 9 Winograd).  128 x 128 maps, every
    option, default / persistent / Winograd-auto selections."""
    D = ConvData(B, 128, 128, seed=200 + B)
    plain, tr = ops.pack_pair(D.dev["w"]), packed_with_transform(D.dev["w"])
    fails = []
    for select, packs in ((0, plain), (7, plain), (11, tr)):
        fails += [f"select {select}: {f}" for f in (check_conv_case(n, D, packs, select, winograd=select == 11) for n in CASES) if f]
    assert not fails, "\n".join(fails)


def test_fp32_conv_refused_combinations():
    """The host refuses exactly these; a silent change in what is accepted fails here (what is accepted runs above)."""
    D = ConvData(1, 8, 32, seed=300)
    pf, pd = ops.pack_pair(D.dev["w"])
    _, pt = packed_with_transform(D.dev["w"])
    dv = D.dev
    refused = {
        "gate_add without gate_out": dict(in_scale=dv["sc"], gate_add=dv["skip"]),
        "gate without in_scale": dict(gate_add=dv["skip"], gate_out=nan4(1, 64, 8, 32)),
        "gate with dot": dict(in_scale=dv["sc"], gate_add=dv["skip"], gate_out=nan4(1, 64, 8, 32), dot=dv["dot"]),
        "dot without partials": dict(dot=dv["dot"]),
        "dot with in_scale": dict(dot=dv["dot"], in_scale=dv["sc"]),
        "gate with mask": dict(in_scale=dv["sc"], gate_add=dv["skip"], gate_out=nan4(1, 64, 8, 32), mask=dv["m"]),
        "gate with in_shift": dict(in_scale=dv["sc"], in_shift=dv["sh"], gate_add=dv["skip"], gate_out=nan4(1, 64, 8, 32)),
        "gate with out_scale": dict(in_scale=dv["sc"], gate_add=dv["skip"], gate_out=nan4(1, 64, 8, 32), out_scale=dv["os"]),
        "LeakyReLU with mask": dict(relu=ops.LEAKY, mask=dv["m"]),
        "LeakyReLU with residual": dict(relu=ops.LEAKY, res=dv["res"]),
        "LeakyReLU with in_scale": dict(relu=ops.LEAKY, in_scale=dv["sc"]),
        "LeakyReLU' mask with residual": dict(relu=ops.LEAKY_MASK, mask=dv["m"], res=dv["res"]),
        "LeakyReLU' code without mask": dict(relu=ops.LEAKY_MASK),
        "relu code 3": dict(relu=3),
        "select 1": dict(select=1),
        "select 3": dict(select=3),
        "select 5": dict(select=5),
        "select 13 (diagnostic builds only)": dict(select=13),
        "sparse select with residual": dict(select=ops.SPARSE_BLOCK_DIAGONAL, res=dv["res"]),
    }
    for what, kw in refused.items():
        kw = dict(kw)
        select = kw.pop("select", 0)
        gap = torch.zeros(1, ops.gap_parts(8, 32), 64, device=DEV) if what == "dot with in_scale" else None
        with pytest.raises(RuntimeError):
            ops.conv_c64(dv["x"], hip.view_plain(8, 32, 64), pf, None, (1, 64), nan4(1, 64, 8, 32), hip.view_plain(8, 32, 64),
                         1, 8, 32, 64, 64, gap=gap, select=select, **kw)
        torch.cuda.synchronize()
    # Winograd selects on a 128 -> 64 conv
    x128 = dev4(X.ints((1, 128, 8, 32), seed=301))
    for sel in (11, 12):
        with pytest.raises(RuntimeError):
            ops.conv_c64(x128, hip.view_plain(8, 32, 128), pt, None, (1, 64), nan4(1, 64, 8, 32), hip.view_plain(8, 32, 64), 1, 8,
                         32, 128, 64, select=sel)


@pytest.mark.parametrize("select", [0, 2, 6])
def test_fp32_conv_multichunk_channels(select):
    """128 -> 192 (two input chunks, three output chunks), forward with bias / ReLU / partial sums and residual / alpha, and
    the 192 -> 128 input-gradient packing with a ReLU' mask."""
    B, H, W = 2, 9, 35
    x, w, b = X.ints((B, 128, H, W), 310), X.weights((192, 128, 3, 3), 311), X.biases(192, 312)
    res, dy, m = X.ints((B, 192, H, W), 313), X.ints((B, 192, H, W), 314), X.ints((B, 128, H, W), 315, zeros=0.3)
    pf, pd = ops.pack_pair(w.to(DEV))
    conv_budget(x, w, extras=(b, res))
    yr = F.relu(X.conv_ref(dd(x), dd(w), dd(b)))
    y, gap, _ = run_conv(dev4(x), pf, B, H, W, select, 128, 192, want_gap=True, bias=b.to(DEV), relu=True)
    X.assert_exact(y, yr, "128 -> 192 + bias + ReLU")
    X.assert_exact(gap.double().sum(dim=1), yr.sum(dim=(2, 3)), "128 -> 192 partial sums")
    y, _, _ = run_conv(dev4(x), pf, B, H, W, select, 128, 192, res=dev4(res), alpha=X.ALPHA)
    X.assert_exact(y, X.ALPHA * X.conv_ref(dd(x), dd(w)) + dd(res), "128 -> 192 * alpha + residual")
    conv_budget(dy, w.flip(2, 3).transpose(0, 1))
    y, _, _ = run_conv(dev4(dy), pd, B, H, W, select, 192, 128, mask=dev4(m))
    X.assert_exact(y, X.dgrad_ref(dd(dy), dd(w)) * X.relu_mask(dd(m)), "192 -> 128 input gradient, ReLU' mask")


def test_fp32_conv_reads_and_writes_stay_inside_the_views():
    """x: map 1 of a two-map stack (hip.view_maps) whose map 0 is NaN; a residual: channel chunk 1 of a 128-channel map whose
    chunk 0 is NaN; y: channel chunk 1 of a 128-channel buffer whose chunk 0 holds a sentinel that must survive."""
    B, H, W = 2, 13, 40
    D = ConvData(B, H, W, seed=320)
    pf, _ = ops.pack_pair(D.dev["w"])
    stack = torch.full((B, 2, H, W, 64), NAN, device=DEV)
    stack[:, 1] = D.dev["x"].permute(0, 2, 3, 1)
    rbuf = torch.full((B, 128, H, W), NAN, device=DEV).contiguous(memory_format=CL)
    rbuf[:, 64:] = D.dev["res"]
    ybuf = torch.full((B, 128, H, W), 1234.5, device=DEV).contiguous(memory_format=CL)
    v128 = hip.view_plain(H, W, 128)
    conv_budget(D.x, D.w, extras=(D.b, D.res))
    for select in (0, 2, 6):
        ybuf[:, 64:] = NAN
        ops.conv_c64(stack[:, 1], hip.view_maps(H, W, 2), pf, D.dev["b"], (1, 64), ybuf[:, 64:], v128, B, H, W, 64, 64,
                     res=rbuf[:, 64:], select=select)
        X.assert_exact(ybuf[:, 64:], X.conv_ref(dd(D.x), dd(D.w), dd(D.b)) + dd(D.res), f"select {select}: output in a view")
        assert (ybuf[:, :64] == 1234.5).all(), f"select {select}: wrote outside the output view"
        assert (stack[:, 0].isnan()).all()


@pytest.mark.parametrize("select,transform", [(0, False), (11, True), (6, False), (2, False)])
def test_fp32_conv_detector(select, transform):
    """x[b, c, h, w] + 1 (one granule) in what the kernel sees: exactly the 3 x 3 neighbourhood of (h, w) in sample b, all 64
    output channels, must fail (the weights have no zero, so every tap shows).  B = 9 at 128^2 with transform: Winograd."""
    B, H, W = (9, 128, 128) if transform else (2, 13, 40)
    x, w = X.ints((B, 64, H, W), 330), X.weights((64, 64, 3, 3), 331, nonzero=True)
    pf = packed_with_transform(w.to(DEV))[0] if transform else ops.pack_pair(w.to(DEV))[0]
    b0, c0, h0, w0 = B - 1, 17, H - 1, 5  # bottom border row: a 2 x 3 neighbourhood
    xs = x.clone()
    xs[b0, c0, h0, w0] += 1
    conv_budget(xs, w)
    y, _, _ = run_conv(dev4(xs), pf, B, H, W, select)
    bad = X.mismatch(y, X.conv_ref(dd(x), dd(w)))
    want = torch.zeros_like(bad)
    want[b0, :, max(h0 - 1, 0):h0 + 2, max(w0 - 1, 0):w0 + 2] = True
    assert torch.equal(bad, want), f"{int(bad.sum())} mismatches, {int(want.sum())} expected"


# ============================================================================ 2. fp32 weight gradient (sisr_wgrad3x3_c64)
def run_wgrad(x, dy, B, H, W, cin=64, cout=64, dw=None, db=None, fn=None, **kw):
    dw = torch.full((cout, cin, 3, 3), NAN, device=DEV) if dw is None else dw
    db = torch.full((cout,), NAN, device=DEV) if db is None else db
    (fn or ops.wgrad_c64)(x, hip.view_plain(H, W, cin), dy, hip.view_plain(H, W, cout), dw, db, B, H, W, cin, cout, **kw)
    return dw, db


def wgrad_exact(x, dy, sc=None, sh=None, alpha=1.0):
    """(dw, db) exact, dY' = dY * dy_scale + dy_shift"""
    dyp = dd(dy)
    if sc is not None:
        dyp = dyp * dd(sc).view(*sc.shape, 1, 1) + dd(sh).view(*sh.shape, 1, 1)
    wgrad_budget(x, dyp)
    return alpha * X.wgrad_ref(dd(x), dyp), alpha * dyp.sum(dim=(0, 2, 3)), dyp


FORMS = {"quadrant": "1", "default": None}  # SISR_WGRAD_QUADRANT_KERNEL (read per call) forces the quadrant form


@pytest.mark.parametrize("B,H,W", [(1, 128, 128), (2, 128, 128), (5, 128, 128), (1, 13, 9), (2, 9, 33), (1, 2, 1), (3, 17, 65)])
@pytest.mark.parametrize("form", list(FORMS))
def test_fp32_wgrad_forms(form, B, H, W):
    """dense form by default from tiles_all = B*ceil(H/8)*ceil(W/32)*pairs >= 128 on (128^2: B = 1 -> 64 tiles quadrant,
    B = 2 -> 128 dense); B = 5 at 128^2: K-split S = min(256, 320 tiles) = 256 does not divide the tile count.  Plain, and
    dy_scale / dy_shift with alpha, bias gradient each time; ragged off the 8 x 32 tile, 1 pixel wide."""
    x, dy = X.ints((B, 64, H, W), 400 + B), X.ints((B, 64, H, W), 401 + H)
    sc, sh = X.scales((B, 64), 402), X.shifts((B, 64), 403)
    with env("SISR_WGRAD_QUADRANT_KERNEL", FORMS[form]):
        for kw, opts in ((dict(), dict()), (dict(sc=sc, sh=sh, alpha=X.ALPHA), dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV), alpha=X.ALPHA))):
            dw_ref, db_ref, _ = wgrad_exact(x, dy, **kw)
            dw, db = run_wgrad(dev4(x), dev4(dy), B, H, W, **opts)
            X.assert_exact(dw, dw_ref, f"{form} dw {list(opts)}")
            X.assert_exact(db, db_ref, f"{form} db {list(opts)}")


@pytest.mark.parametrize("cin,cout,B,H,W", [(128, 192, 1, 40, 40), (128, 192, 2, 64, 64), (64, 256, 1, 128, 128)])
@pytest.mark.parametrize("form", list(FORMS))
def test_fp32_wgrad_multi_pair(form, cin, cout, B, H, W):
    """several (cin chunk, cout chunk) pairs: 60 / 192 / 256 tiles_all (quadrant by the rule / dense / dense multi-pair grid)"""
    x, dy = X.ints((B, cin, H, W), 410, lo=-1, hi=1), X.ints((B, cout, H, W), 411, lo=-1, hi=1)
    dw_ref, db_ref, _ = wgrad_exact(x, dy)
    with env("SISR_WGRAD_QUADRANT_KERNEL", FORMS[form]):
        dw, db = run_wgrad(dev4(x), dev4(dy), B, H, W, cin, cout)
    X.assert_exact(dw, dw_ref, "dw")
    X.assert_exact(db, db_ref, "db")


@pytest.mark.parametrize("B,H,W", WALK + [(3, 150, 300)])
def test_fp32_wgrad_tile_walk(B, H, W):
    """the default form at the WALK shapes: (3, 100, 250) is 312 tiles of 8 x 32 on 256 workgroups (dense kernel, per-XCD
    walk, a ragged last eighth), the others the quadrant kernel; (3, 150, 300) is more than 8 x 128^2 pixels: the Winograd
    form, 570 tiles on 256 workgroups, ragged both ways.  Plain and dy_scale / dy_shift."""
    x, dy = X.ints((B, 64, H, W), 420 + B), X.ints((B, 64, H, W), 421 + H)
    sc, sh = X.scales((B, 64), 422), X.shifts((B, 64), 423)
    for kw, opts in ((dict(), dict()), (dict(sc=sc, sh=sh), dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV)))):
        dw_ref, db_ref, _ = wgrad_exact(x, dy, **kw)
        dw, db = run_wgrad(dev4(x), dev4(dy), B, H, W, **opts)
        X.assert_exact(dw, dw_ref, f"dw {list(opts)}")
        X.assert_exact(db, db_ref, f"db {list(opts)}")


def test_fp32_wgrad_winograd_round_robin_walk():
    """128 -> 192 (six chunk pairs: a K-split of 42 workgroups, no multiple of 8) above the Winograd threshold"""
    B, H, W, cin, cout = 3, 150, 300, 128, 192
    x, dy = X.ints((B, cin, H, W), 430, lo=-1, hi=1), X.ints((B, cout, H, W), 431, lo=-1, hi=1)
    dw_ref, db_ref, _ = wgrad_exact(x, dy)
    dw, db = run_wgrad(dev4(x), dev4(dy), B, H, W, cin, cout)
    X.assert_exact(dw, dw_ref, "dw")
    X.assert_exact(db, db_ref, "db")


@pytest.mark.parametrize("cin,cout,units", [(64, 64, 0b0110), (64, 64, 0b1001), (64, 128, 0xC3), (128, 64, 0x3F),
                                            (128, 128, 0x9669)])
def test_fp32_wgrad_active_units(cin, cout, units):
    """active_units: bit ((cin_chunk * cout_chunks + cout_chunk) * 4 + ci_half * 2 + co_half) selects a 32 x 32 block; the
    active blocks are exact, the others keep their sentinel."""
    B, H, W = 2, 19, 45
    x, dy = X.ints((B, cin, H, W), 420), X.ints((B, cout, H, W), 421)
    dw_ref, db_ref, _ = wgrad_exact(x, dy)
    dw, db = run_wgrad(dev4(x), dev4(dy), B, H, W, cin, cout, active_units=units)
    on = torch.zeros(cout, cin, dtype=torch.bool)
    cq_n = cout // 64
    for u in range(cin // 64 * cq_n * 4):
        if units >> u & 1:
            cc, cq, cih, coh = (u >> 2) // cq_n, (u >> 2) % cq_n, (u >> 1) & 1, u & 1
            on[cq * 64 + coh * 32:cq * 64 + coh * 32 + 32, cc * 64 + cih * 32:cc * 64 + cih * 32 + 32] = True
    on = on.to(DEV)
    X.assert_exact(dw[on], dw_ref[on], "active blocks")
    assert dw[~on].isnan().all(), "a masked block was written"
    X.assert_exact(db, db_ref, "db")


@pytest.mark.parametrize("B", [8, 9])
def test_fp32_wgrad_batched_and_deferred(B):
    """batched weight gradient (WgradQueue, sisr_wgrad3x3_c64_batch) where WgradQueue.wanted: B*H*W <= 8*128^2 (B = 8 batched,
    9 not); jobs of mixed options (dy_scale / dy_shift, no bias).  Then the conv's backward inside deferred_wgrads(): queued
    at B = 8, launched directly at B = 9 -- exact either way."""
    H = W = 128
    assert ops.WgradQueue.wanted(B, H, W) == (B * H * W <= 8 * 128 * 128)
    xs = [X.ints((B, 64, H, W), 430 + k, lo=-1, hi=1) for k in range(3)]
    dys = [X.ints((B, 64, H, W), 440 + k, lo=-1, hi=1) for k in range(3)]
    sc, sh = X.scales((B, 64), 450), X.shifts((B, 64), 451)
    if ops.WgradQueue.wanted(B, H, W):
        q = ops.WgradQueue(B, H, W, torch.device(DEV))
        outs = []
        for k in range(3):
            dw, db = torch.full((64, 64, 3, 3), NAN, device=DEV), (torch.full((64,), NAN, device=DEV) if k != 1 else None)
            kw = dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV)) if k == 2 else {}
            q.add(dev4(xs[k]), dev4(dys[k]), dw, db, **kw)
            outs.append((dw, db))
        q.flush()
        for k, (dw, db) in enumerate(outs):
            dw_ref, db_ref, _ = wgrad_exact(xs[k], dys[k], *((sc, sh) if k == 2 else ()))
            X.assert_exact(dw, dw_ref, f"batched job {k} dw")
            if db is not None:
                X.assert_exact(db, db_ref, f"batched job {k} db")
    w = X.weights((64, 64, 3, 3), 452)
    wg = w.to(DEV).requires_grad_(True)
    bg = X.biases(64, 453).to(DEV).requires_grad_(True)
    xg = dev4(xs[0]).requires_grad_(True)
    with ops.deferred_wgrads():
        y = ops.conv3x3(xg, wg, bg)
        y.backward(dev4(dys[0]))
        queued = ops._DEFERRED is not None and len(ops._DEFERRED) > 0
    assert queued == ops.WgradQueue.wanted(B, H, W)
    dw_ref, db_ref, _ = wgrad_exact(xs[0], dys[0])
    X.assert_exact(wg.grad, dw_ref, "deferred dw")
    X.assert_exact(bg.grad, db_ref, "deferred db")


@pytest.mark.parametrize("form,B,H,W", [("default", 2, 128, 128), ("quadrant", 2, 128, 128), ("default", 5, 128, 128),
                                        ("default", 1, 17, 40)])
def test_fp32_wgrad_detector(form, B, H, W):
    """x[b, c, h, w] + 1 on the top border row: exactly dw[:, c] at the 6 taps whose shifted pixel is inside the map must
    fail (dy has no zero); the bias gradient must not."""
    x, dy = X.ints((B, 64, H, W), 460), X.nonzero_ints((B, 64, H, W), 461)
    b0, c0, h0, w0 = B - 1, 40, 0, 9
    xs = x.clone()
    xs[b0, c0, h0, w0] += 1
    dw_ref, db_ref, _ = wgrad_exact(x, dy)
    wgrad_budget(xs, dy)
    with env("SISR_WGRAD_QUADRANT_KERNEL", FORMS[form]):
        dw, db = run_wgrad(dev4(xs), dev4(dy), B, H, W)
    want = torch.zeros(64, 64, 3, 3, dtype=torch.bool, device=DEV)
    want[:, c0, :2, :] = True  # x[h, w] meets dY[h - ky + 1, w - kx + 1]: tap ky = 2 would need row -1
    assert torch.equal(X.mismatch(dw, dw_ref), want)
    X.assert_exact(db, db_ref, "db")


# ============================================================================ pixel shuffle and production sizes (autograd node)
def conv_node_exact(B, H, W, cin, cout, r, seed, lo=-2, zeros=None, what=""):
    """ops.conv3x3 forward and backward (input, weight, bias gradients) against the exact values"""
    x = X.ints((B, cin, H, W), seed, lo=lo, hi=-lo, zeros=zeros)
    w, b = X.weights((cout, cin, 3, 3), seed + 1), X.biases(cout, seed + 2)
    dy = X.ints((B, cout // (r * r), H * r, W * r), seed + 3, lo=lo, hi=-lo, zeros=zeros)
    conv_budget(x, w, extras=(b,), what=what + " forward")
    xg = (dev4(x) if cin % 64 == 0 else x.to(DEV)).requires_grad_(True)
    wg, bg = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.conv3x3(xg, wg, bg, shuffle=r)
    yr = X.conv_ref(dd(x), dd(w), dd(b))
    X.assert_exact(y, F.pixel_shuffle(yr, r) if r > 1 else yr, what + " forward")
    del yr
    y.backward(dev4(dy) if dy.shape[1] % 64 == 0 else dy.to(DEV))
    del y
    dyc = F.pixel_unshuffle(dd(dy), r) if r > 1 else dd(dy)  # the conv's own output gradient (the shuffle permutation)
    conv_budget(dyc, w.flip(2, 3).transpose(0, 1), what=what + " input gradient")
    X.assert_exact(xg.grad, X.dgrad_ref(dyc, dd(w)), what + " input gradient")
    wgrad_budget(x, dyc, what=what + " weight gradient")
    X.assert_exact(wg.grad, X.wgrad_ref(dd(x), dyc), what + " weight gradient")
    X.assert_exact(bg.grad, dyc.sum(dim=(0, 2, 3)), what + " bias gradient")


@pytest.mark.parametrize("r,B,H,W", [(2, 2, 7, 10), (3, 1, 5, 33), (2, 1, 1, 2), (2, 1, 128, 128), (2, 2, 128, 128)])
def test_pixel_shuffle_conv_and_gradients(r, B, H, W):
    """64 -> 64 r^2 with the fused PixelShuffle(r) store, its input gradient through the shuffle view and the weight gradient's
    shuffle permutation (64 -> 256 at 128^2: 4 pairs x 64 tiles, the dense multi-pair grid)"""
    conv_node_exact(B, H, W, 64, 64 * r * r, r, seed=500 + r + B, lo=-1, what=f"64 -> {64 * r * r} shuffle {r}")


@pytest.mark.parametrize("what,B,H,W,cin,cout,r", [("body 64 -> 64", 32, 128, 128, 64, 64, 1),
                                                   ("upsampler 1", 32, 128, 128, 64, 256, 2),
                                                   ("upsampler 2 (2^31-byte output)", 32, 256, 256, 64, 256, 2),
                                                   ("tail 64 -> 3", 32, 512, 512, 64, 3, 1),
                                                   ("head 3 -> 64", 32, 128, 128, 3, 64, 1)])
def test_production_sizes(what, B, H, W, cin, cout, r):
    """the bench step's shapes, forward, input gradient, weight gradient: {-1, 0, 1} data, zeros where the weight gradient's
    pixel count needs them (budget)"""
    zeros = 0.5 if B * H * W * r * r > (1 << 21) else None
    conv_node_exact(B, H, W, cin, cout, r, seed=510, lo=-1, zeros=zeros, what=what)
    torch.cuda.empty_cache()


# ============================================================================ 3 / 4. bf16 operand mode, bf16 storage, bf16x3
@pytest.mark.parametrize("B,H,W", [(1, 13, 9), (2, 5, 33), (2, 5, 1), (7, 128, 128), (8, 128, 128)])
@pytest.mark.parametrize("mode,select", [("bf16", 0), ("bf16", 1), ("bf16x3", 0)])
def test_bf16_conv_forms(mode, select, B, H, W):
    """bf16 operand mode (select 0: persistent tile loop from nblk >= 1024 -- B = 8 at 128^2, B = 7 below; 1: per-tile) and
    bf16x3 (three-plane split: the low planes of bf16-exact data are zero): every option the entries accept, exact."""
    D = ConvData(B, H, W, seed=600 + B + H)
    with precision(mode):
        packs = ops.pack_pair(D.dev["w"])
        assert packs[0].dtype == torch.bfloat16
        fails = []
        for n in CASES + (BF16_EXTRA if (B, H, W) == (1, 13, 9) else []):
            if n in FP32_ONLY or n in BF16_REFUSED:
                pk, kw, *_ = conv_case(n, D)
                with pytest.raises(RuntimeError):
                    run_conv(D.dev["x"], packs[0] if pk == "f" else packs[1], B, H, W, select, **kw)
                continue
            f = check_conv_case(n, D, packs, select)
            if f:
                fails.append(f)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,H,W", WALK)
@pytest.mark.parametrize("mode,select", [("bf16", 1), ("bf16x3", 0)])
def test_bf16_per_tile_conv_tile_walk(mode, select, B, H, W):
    """the per-tile bf16 and bf16x3 kernels (block map, float4 epilogue through the LDS transpose buffer) at the WALK shapes"""
    D = ConvData(B, H, W, seed=620 + B + H)
    with precision(mode):
        packs = ops.pack_pair(D.dev["w"])
        fails = [f for f in (check_conv_case(n, D, packs, select) for n in CASES + BF16_EXTRA
                             if n not in FP32_ONLY and n not in BF16_REFUSED) if f]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,H,W", [(1, 13, 9), (2, 16, 40), (9, 128, 128)])
def test_bf16_storage_conv_codes(B, H, W):
    """sisr_conv3x3_c64_bf16s, storage bits 1 = x / gate_add / gate_out, 2 = y, 4 = mask / dot, 8 = res bf16 maps: the codes
    the group node launches (1, 3, 4, 6, 7, 9, 11, 15).  bf16 inputs hold the exact data as it is; a bf16 output must be the
    one round-to-nearest-even of the exact value (the kernel's deliberate rounding)."""
    D = ConvData(B, H, W, seed=650 + B)
    d16 = {k: dev4(getattr(D, k), torch.bfloat16) for k in ("x", "res", "skip", "dot", "m")}
    dv = D.dev
    x, w = dd(D.x), dd(D.w)
    wt = w.flip(2, 3).transpose(0, 1)
    b, res, m, dot = dd(D.b).view(1, 64, 1, 1), dd(D.res), dd(D.m), dd(D.dot)
    sc, sh = dd(D.sc).view(B, 64, 1, 1), dd(D.sh).view(B, 64, 1, 1)
    u_gate = x * sc + dd(D.skip)
    u_aff = x * sc + sh
    with precision("bf16", "all"):
        pf, pd = ops.pack_pair(dv["w"])
        forms = [  # (storage, bf16 out, packing, x operand (bf16?), kwargs, exact y, exact partials, exact gate_out, operand)
            (3, True, pf, True, dict(bias=dv["b"], relu=True), F.relu(X.conv_ref(x, w) + b), None, None, x),
            (3, True, pf, True, dict(bias=dv["b"], gap=True), X.conv_ref(x, w) + b, "sum", None, x),
            (3, True, pf, True, dict(bias=dv["b"], relu=True, in_scale=dv["sc"], gate_add=d16["skip"], gate_out=True),
             F.relu(X.conv_ref(u_gate, w) + b), None, u_gate, u_gate),
            (1, False, pf, True, dict(bias=dv["b"], in_scale=dv["sc"], gate_add=d16["skip"], gate_out=True, res=dv["res"]),
             X.conv_ref(u_gate, w) + b + res, None, u_gate, u_gate),
            (4, False, pd, False, dict(gap=True, dot=d16["dot"]), X.conv_ref(x, wt), "dot", None, x),
            (4, False, pd, False, dict(gap=True, dot=d16["dot"], res=dv["res"]), X.conv_ref(x, wt) + res, "dot", None, x),
            (4, False, pd, False, dict(mask=d16["m"], in_scale=dv["sc"], in_shift=dv["sh"]),
             X.conv_ref(u_aff, wt) * X.relu_mask(m), None, None, u_aff),
            (6, True, pd, False, dict(gap=True, dot=d16["dot"]), X.conv_ref(x, wt), "dot", None, x),
            (15, True, pd, True, dict(gap=True, dot=d16["dot"], res=d16["res"]), X.conv_ref(x, wt) + res, "dot", None, x),
            (7, True, pd, True, dict(mask=d16["m"], in_scale=dv["sc"], in_shift=dv["sh"]),
             X.conv_ref(u_aff, wt) * X.relu_mask(m), None, None, u_aff),
            (11, True, pd, True, dict(res=d16["res"]), X.conv_ref(x, wt) + res, None, None, x),
            (9, False, pd, True, dict(res=d16["res"]), X.conv_ref(x, wt) + res, None, None, x),
        ]
        fails = []
        for k, (storage, out16, pk, x16, kw, y_ref, part, gout_ref, u) in enumerate(forms):
            conv_budget(u, w, extras=(D.b, D.res))
            if part is not None:
                X.assert_budget((y_ref.abs() * (dot.abs() if part == "dot" else 1)).sum(dim=(2, 3)), X.granule(y_ref), "partials")
            kw = dict(kw)
            y = nan4(B, 64, H, W, torch.bfloat16 if out16 else torch.float32)
            gap = torch.full((B, ops.gap_parts(H, W), 64), NAN, device=DEV) if kw.pop("gap", False) else None
            go = nan4(B, 64, H, W, torch.bfloat16) if kw.pop("gate_out", False) else None
            ops.conv_c64s(d16["x"] if x16 else dv["x"], pk, kw.pop("bias", None), y, B, H, W, storage, gap=gap, gate_out=go, **kw)
            try:
                X.assert_exact(y.double() if not out16 else y.float(), y_ref if not out16 else X.bf16_of(y_ref).double(),
                               f"storage {storage} form {k} output")
                if part is not None:
                    want = (y_ref * (dot if part == "dot" else 1)).sum(dim=(2, 3))  # taken from the fp32 values
                    X.assert_exact(gap.double().sum(dim=1), want, f"storage {storage} form {k} partials")
                if go is not None:
                    X.assert_exact(go.float(), X.bf16_of(gout_ref).double(), f"storage {storage} form {k} gate_out")
            except AssertionError as e:
                fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,H,W", [(1, 13, 9), (2, 40, 48), (3, 128, 128), (1, 2, 1)])
@pytest.mark.parametrize("mode,storage", [("bf16", 0), ("bf16", 1), ("bf16", 3), ("bf16x3", 0)])
def test_bf16_wgrad_forms(mode, storage, B, H, W):
    """bf16 weight gradient with fp32 maps (0), a bf16 x (1), bf16 x and dY (3); the bf16x3 split kernel: exact, with and
    without dy_scale / dy_shift"""
    x, dy = X.ints((B, 64, H, W), 700), X.ints((B, 64, H, W), 701)
    sc, sh = X.scales((B, 64), 702), X.shifts((B, 64), 703)
    xin = dev4(x, torch.bfloat16) if storage & 1 else dev4(x)
    dyin = dev4(dy, torch.bfloat16) if storage & 2 else dev4(dy)
    with precision(mode):
        for kw, opts in ((dict(), dict()), (dict(sc=sc, sh=sh), dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV)))):
            dw_ref, db_ref, _ = wgrad_exact(x, dy, **kw)
            dw, db = run_wgrad(xin, dyin, B, H, W, storage=storage, **opts)
            X.assert_exact(dw, dw_ref, f"{mode} storage {storage} dw")
            X.assert_exact(db, db_ref, f"{mode} storage {storage} db")


@pytest.mark.parametrize("B,H,W", WALK)
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_bf16_wgrad_tile_walk(mode, B, H, W):
    """the persistent bf16 and bf16x3 weight-gradient kernels at the WALK shapes, plain and dy_scale / dy_shift"""
    x, dy = X.ints((B, 64, H, W), 710 + B), X.ints((B, 64, H, W), 711 + H)
    sc, sh = X.scales((B, 64), 712), X.shifts((B, 64), 713)
    with precision(mode):
        for kw, opts in ((dict(), dict()), (dict(sc=sc, sh=sh), dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV)))):
            dw_ref, db_ref, _ = wgrad_exact(x, dy, **kw)
            dw, db = run_wgrad(dev4(x), dev4(dy), B, H, W, **opts)
            X.assert_exact(dw, dw_ref, f"{mode} dw {list(opts)}")
            X.assert_exact(db, db_ref, f"{mode} db {list(opts)}")


@pytest.mark.parametrize("mode,B", [("bf16", 8), ("bf16", 2), ("bf16x3", 2)])
def test_bf16_detectors(mode, B):
    """one granule on one input element: exactly its neighbourhood of the conv and its dw[:, c] slice of the weight
    gradient fail (persistent bf16 kernel at B = 8, per-tile at 2)"""
    H, W = 128, 128
    x, w = X.ints((B, 64, H, W), 710), X.weights((64, 64, 3, 3), 711, nonzero=True)
    dy = X.nonzero_ints((B, 64, H, W), 712, m=1)
    xs = x.clone()
    xs[0, 3, 64, 0] += 1  # left border column: a 3 x 2 neighbourhood, 6 taps
    conv_budget(xs, w)
    with precision(mode):
        pf, _ = ops.pack_pair(w.to(DEV))
        y, _, _ = run_conv(dev4(xs), pf, B, H, W, 0)
        bad = X.mismatch(y, X.conv_ref(dd(x), dd(w)))
        want = torch.zeros_like(bad)
        want[0, :, 63:66, 0:2] = True
        assert torch.equal(bad, want)
        dw_ref, _, _ = wgrad_exact(x, dy)
        wgrad_budget(xs, dy)
        dw, _ = run_wgrad(dev4(xs), dev4(dy), B, H, W)
        wantw = torch.zeros(64, 64, 3, 3, dtype=torch.bool, device=DEV)
        wantw[:, 3, :, :2] = True  # x[h, w] meets dY[h - ky + 1, w - kx + 1]: tap kx = 2 would need column -1
        assert torch.equal(X.mismatch(dw, dw_ref), wantw)


# ============================================================================ 5. packing: zero-padded weights
@pytest.mark.parametrize("co,ci", [(42, 84), (3, 64), (64, 32), (100, 128)])
def test_padded_weight_packing(co, ci):
    """_PackPlan packs a weight whose channel counts are not multiples of 64 as its zero-padded twin (PackJob co_real /
    ci_real): the conv over the padded geometry is exact, its padded output channels exactly 0, both packings."""
    cop, cip = (co + 63) // 64 * 64, (ci + 63) // 64 * 64
    B, H, W = 2, 11, 37
    w = X.weights((co, ci, 3, 3), 800 + co)
    wp = torch.zeros(cop, cip, 3, 3)
    wp[:co, :ci] = w
    plan = ops._PackPlan([(w.to(DEV), 1)], torch.device(DEV))
    plan.run()
    ops.invalidate_packs()
    pf, pd = plan.slices[0]
    x = torch.zeros(B, cip, H, W)
    x[:, :ci] = X.ints((B, ci, H, W), 801)
    dy = X.ints((B, cop, H, W), 802)
    conv_budget(x, wp)
    y, _, _ = run_conv(dev4(x), pf, B, H, W, 0, cip, cop)
    X.assert_exact(y, X.conv_ref(dd(x), dd(wp)), "forward packing")
    conv_budget(dy, wp.flip(2, 3).transpose(0, 1))
    dx, _, _ = run_conv(dev4(dy), pd, B, H, W, 0, cop, cip)
    X.assert_exact(dx, X.dgrad_ref(dd(dy), dd(wp)), "input-gradient packing")


# ============================================================================ 6. RGB side convs (cin3 / cout3 / corr3x3_c3)
@pytest.mark.parametrize("shape", [(2, 11, 19), (1, 1, 1), (1, 2, 31), (1, 3, 30), (1, 7, 61), (3, 64, 95), (2, 200, 333)])
@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 3), (3, 128), (128, 3)])
def test_rgb_side_convs(cin, cout, shape):
    """3 -> 64k (sisr_conv3x3_cin3; its input gradient is sisr_conv3x3_cout3) and 64k -> 3 (rgb_out_mfma_kernel, 3 x 30
    tiles: ragged off both edges; input gradient on cin3), weight gradients by sisr_corr3x3_c3"""
    B, H, W = shape
    conv_node_exact(B, H, W, cin, cout, 1, seed=900 + cin + H, what=f"{cin} -> {cout}")


@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 3)])
def test_rgb_detector(cin, cout):
    B, H, W = 2, 9, 61
    x, w = X.ints((B, cin, H, W), 910), X.weights((cout, cin, 3, 3), 911, nonzero=True)
    xs = x.clone()
    xs[1, 2, 4, 60] += 1  # right border column
    conv_budget(xs, w)
    with torch.no_grad():
        y = ops.conv3x3(dev4(xs) if cin == 64 else xs.to(DEV), w.to(DEV))
    bad = X.mismatch(y, X.conv_ref(dd(x), dd(w)))
    want = torch.zeros_like(bad)
    want[1, :, 3:6, 59:61] = True
    assert torch.equal(bad, want)


# ============================================================================ 7. SPARNet geometric convs (ops.refl_conv, REFL_GEO)
def refl_case(ci, co, up, stride, shape, seed, form=None, x_override=None):
    """ops.refl_conv forward / input / weight / bias gradients against the exact float64 pad(reflect) + nearest composition;
    the kernels see the maps zero-padded to 64-multiples"""
    B, H, W = shape
    Cp, cop = (ci + 63) // 64 * 64, (co + 63) // 64 * 64
    x = X.ints((B, ci, H, W), seed) if x_override is None else x_override
    w, b = X.weights((co, ci, 3, 3), seed + 1), X.biases(co, seed + 2)
    xr, wr, br = dd(x).requires_grad_(True), dd(w).requires_grad_(True), dd(b).requires_grad_(True)
    yr = X.geo_conv_ref(xr, wr, br, up=up, stride=stride)
    dy = X.ints(tuple(yr.shape), seed + 3)
    gx, gw, gb = torch.autograd.grad(yr, (xr, wr, br), dd(dy))
    # budget: the same linear maps on absolute values bound every partial sum
    xa, wa = dd(x).abs().requires_grad_(True), dd(w).abs().requires_grad_(True)
    ya = X.geo_conv_ref(xa, wa, dd(b).abs(), up=up, stride=stride)
    ax, aw = torch.autograd.grad(ya, (xa, wa), dd(dy).abs())
    gran = X.granule(x) * X.granule(w)
    X.assert_budget(ya, min(gran, X.granule(b)), "geo forward")
    X.assert_budget(ax, X.granule(dy) * X.granule(w), "geo input gradient")
    X.assert_budget(aw, X.granule(dy) * X.granule(x), "geo weight gradient")
    xp = torch.zeros(B, Cp, H, W)
    xp[:, :ci] = x
    xg = dev4(xp).requires_grad_(True)
    conv = torch.nn.Conv2d(ci, co, 3, stride).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    keep = ops.REFL_GEO
    ops.REFL_GEO = True
    try:
        with env("SISR_WGRAD_QUADRANT_KERNEL", form):
            y = ops.refl_conv(xg, conv.weight, conv.bias, up=up, stride=stride)
            cot = torch.zeros(tuple(y.shape))
            cot[:, :co] = dy
            y.backward(dev4(cot))
    finally:
        ops.REFL_GEO = keep
    return y, xg.grad, conv.weight.grad, conv.bias.grad, yr.detach(), gx, gw, gb


GEO = [(64, 64, 1, 1, (1, 4, 4)), (42, 84, 1, 2, (2, 32, 32)), (84, 42, 2, 1, (2, 8, 8)), (64, 128, 2, 1, (1, 33, 17)),
       (64, 64, 1, 2, (1, 70, 67)), (128, 128, 1, 2, (1, 7, 5)), (64, 64, 2, 1, (1, 2, 3)), (32, 3, 1, 1, (2, 20, 70)),
       (64, 64, 1, 1, (2, 128, 128)), (32, 32, 1, 1, (3, 128, 128)), (64, 64, 1, 2, (2, 127, 129))]


@pytest.mark.parametrize("ci,co,up,stride,shape", GEO)
@pytest.mark.parametrize("form", ["default", "quadrant"])
def test_sparnet_geometric_conv(form, ci, co, up, stride, shape):
    """up = 2 (nearest read in place) and stride = 2 (zero-stuffed dY) on odd sizes, padded channel counts; the geometric
    weight gradient in its dense form (2 x 128^2 x 64 -> 64: 128 tiles) and forced quadrant form"""
    y, gx, gw, gb, yr, gxr, gwr, gbr = refl_case(ci, co, up, stride, shape, seed=1000 + ci + co + up, form=FORMS[form])
    X.assert_exact(y[:, :co], yr, "geo forward")
    assert (y[:, co:] == 0).all()
    X.assert_exact(gx[:, :ci], gxr, "geo input gradient")
    X.assert_exact(gw, gwr, "geo weight gradient")
    X.assert_exact(gb, gbr, "geo bias gradient")


def test_sparnet_batched_geometric_weight_gradients():
    """WgradGeoQueue (sisr_wgrad3x3_c64_geo_batch) inside deferred_wgrads(): eleven convs of mixed sizes, channel padding and
    upsampling, exact"""
    cases = [(32, 32, 1, (2, 16, 16)), (64, 64, 1, (2, 8, 8)), (128, 128, 1, (2, 16, 16)), (64, 1, 1, (2, 16, 16)),
             (3, 32, 1, (1, 24, 40)), (64, 64, 2, (2, 4, 4)), (128, 64, 1, (2, 8, 8)), (64, 128, 2, (2, 8, 8)),
             (64, 64, 1, (2, 4, 4)), (32, 3, 1, (2, 9, 33)), (64, 64, 1, (2, 32, 32))]
    convs, xs, cots, refs = [], [], [], []
    for k, (ci, co, up, (B, H, W)) in enumerate(cases):
        Cp, cop = (ci + 63) // 64 * 64, (co + 63) // 64 * 64
        x, w, b = X.ints((B, ci, H, W), 1100 + k), X.weights((co, ci, 3, 3), 1120 + k), X.biases(co, 1140 + k)
        dy = X.ints((B, co, up * H, up * W), 1160 + k)
        wr, br = dd(w).requires_grad_(True), dd(b).requires_grad_(True)
        refs.append(torch.autograd.grad(X.geo_conv_ref(dd(x), wr, br, up=up), (wr, br), dd(dy)))
        wgrad_budget(X.geo_input(dd(x), up), dd(dy), padding=0)
        xp = torch.zeros(B, Cp, H, W)
        xp[:, :ci] = x
        cot = torch.zeros(B, cop, up * H, up * W)
        cot[:, :co] = dy
        xs.append(dev4(xp))
        cots.append(dev4(cot))
        c = torch.nn.Conv2d(ci, co, 3).to(DEV)
        with torch.no_grad():
            c.weight.copy_(w)
            c.bias.copy_(b)
        convs.append(c)
    keep = ops.REFL_GEO
    ops.REFL_GEO = True
    try:
        with ops.deferred_wgrads():
            total = 0.0
            for (ci, co, up, _), c, x, cot in zip(cases, convs, xs, cots):
                total = total + (ops.refl_conv(x, c.weight, c.bias, up=up, stride=1) * cot).sum()
            total.backward()
            assert len(ops._DEFERRED[("geo", 0)].jobs) == len(cases)
    finally:
        ops.REFL_GEO = keep
    for k, (c, (gw, gb)) in enumerate(zip(convs, refs)):
        X.assert_exact(c.weight.grad, gw, f"job {k} dw")
        X.assert_exact(c.bias.grad, gb, f"job {k} db")


def test_sparnet_detector():
    """one granule on one input element of a stride-1 reflection conv: the mismatches of the output and of the weight gradient
    are exactly where the exact results of the moved input differ (reflection makes a border element feed more outputs)"""
    ci, co, shape = 64, 64, (1, 20, 36)
    x = X.ints((1, ci) + shape[1:], 1200)
    xs = x.clone()
    xs[0, 5, 0, 17] += 1
    y, _, gw, _, yr, _, gwr, _ = refl_case(ci, co, 1, 1, shape, seed=1200, x_override=xs)
    _, _, _, _, yr0, _, gwr0, _ = refl_case(ci, co, 1, 1, shape, seed=1200, x_override=x)
    X.assert_exact(y[:, :co], yr, "moved input, own reference")
    assert torch.equal(X.mismatch(y[:, :co], yr0), yr != yr0) and int((yr != yr0).sum()) > 0
    assert torch.equal(X.mismatch(gw, gwr0), gwr != gwr0) and int((gwr != gwr0).sum()) > 0


# ============================================================================ 8. SFTMD: sparse select codes, LeakyReLU forms, conv9
@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (1, 9, 5), (4, 64, 64)])
def test_sftmd_sparse_selects(B, H, W):
    """select 8 (64 -> 128 block-diagonal, plain), 9 (128 -> 64, inputs >= 80 zero, LeakyReLU epilogue: one fp32 rounding of
    v * 0.2f), 10 (the transpose of 8, LeakyReLU' mask with exact zeros at the mask's boundary), both grid sizes"""
    wb = torch.zeros(128, 64, 3, 3)
    wb[:64, :32] = X.weights((64, 32, 3, 3), 1300)
    wb[64:, 32:] = X.weights((64, 32, 3, 3), 1301)
    wa = torch.zeros(64, 128, 3, 3)
    wa[:, :80] = X.weights((64, 80, 3, 3), 1302)
    bias = X.biases(128, 1303)
    t = X.ints((B, 64, H, W), 1304, zeros=0.3)
    cat = X.ints((B, 128, H, W), 1305)
    dy2 = X.ints((B, 128, H, W), 1306)
    pf, pdb = ops.pack_pair(wb.to(DEV))
    pa, _ = ops.pack_pair(wa.to(DEV))
    for sel in (0, ops.SPARSE_BLOCK_DIAGONAL):
        conv_budget(t, wb, extras=(bias,))
        y, _, _ = run_conv(dev4(t), pf, B, H, W, sel, 64, 128, bias=bias.to(DEV))
        X.assert_exact(y, X.conv_ref(dd(t), dd(wb), dd(bias)), f"select {sel}: 64 -> 128 block-diagonal")
    for sel in (0, ops.SPARSE_SECOND_CHUNK):
        conv_budget(cat, wa)
        y, _, _ = run_conv(dev4(cat), pa, B, H, W, sel, 128, 64, relu=ops.LEAKY)
        X.assert_exact(y, X.leaky_ref(X.conv_ref(dd(cat), dd(wa))), f"select {sel}: LeakyReLU epilogue")
    for sel in (0, ops.SPARSE_HALVES):
        conv_budget(dy2, wb.flip(2, 3).transpose(0, 1))
        y, _, _ = run_conv(dev4(dy2), pdb, B, H, W, sel, 128, 64, mask=dev4(t), relu=ops.LEAKY_MASK)
        X.assert_exact(y, X.fp32_round(X.dgrad_ref(dd(dy2), dd(wb)) * X.leaky_mask(dd(t))), f"select {sel}: LeakyReLU' mask")


@pytest.mark.parametrize("B,H,W", [(1, 7, 9), (2, 16, 33), (1, 3, 100), (2, 130, 200)])
def test_conv9_forward_and_gradients(B, H, W):
    """9 x 9 64 -> 3 conv (sisr_conv9_fwd), its input gradient masked by LeakyReLU' of the map that fed it (exact zeros in
    that map: ties), its weight / bias gradient"""
    L = hip.lib()
    x = X.ints((B, 64, H, W), 1400, lo=-1, hi=1, zeros=0.3)
    w, b = X.weights((3, 64, 9, 9), 1401), X.biases(3, 1402)
    dy = X.ints((B, 3, H, W), 1403)
    xa, wc, bc = dev4(x), w.to(DEV), b.to(DEV)
    conv_budget(x, w, extras=(b,), padding=4)
    y = torch.full((B, 3, H, W), NAN, device=DEV)
    hip.check(L.sisr_conv9_fwd(hip.ptr(xa), hip.ptr(wc), hip.ptr(bc), hip.ptr(y), B, H, W, hip.stream()), "conv9")
    X.assert_exact(y, X.conv_ref(dd(x), dd(w), dd(b)), "conv9 forward")
    dyd = dy.to(DEV)
    conv_budget(dy, w.flip(2, 3).transpose(0, 1), padding=4)
    dx = nan4(B, 64, H, W)
    hip.check(L.sisr_conv9_dgrad(hip.ptr(dyd), hip.ptr(wc), hip.ptr(xa), hip.ptr(dx), B, H, W, hip.stream()), "conv9 dgrad")
    X.assert_exact(dx, X.fp32_round(X.dgrad_ref(dd(dy), dd(w)) * X.leaky_mask(dd(x))), "conv9 input gradient")
    wgrad_budget(x, dy, padding=4, k=9)
    dw, db = torch.full_like(wc, NAN), torch.full((3,), NAN, device=DEV)
    nbytes = L.sisr_conv9_wgrad_workspace_bytes(B, H, W)
    ws = hip.workspace(xa.device, nbytes)
    hip.check(L.sisr_conv9_wgrad(hip.ptr(xa), hip.ptr(dyd), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), nbytes, B, H, W, hip.stream()),
              "conv9 wgrad")
    X.assert_exact(dw, X.wgrad_ref(dd(x), dd(dy), padding=4, k=9), "conv9 weight gradient")
    X.assert_exact(db, dd(dy).sum(dim=(0, 2, 3)), "conv9 bias gradient")


def test_sftmd_detector():
    """LeakyReLU' mask form (select 10): one granule on one dY element fails exactly the outputs it feeds"""
    B, H, W = 1, 16, 16
    wb = torch.zeros(128, 64, 3, 3)
    wb[:64, :32] = X.weights((64, 32, 3, 3), 1500, nonzero=True)
    wb[64:, 32:] = X.weights((64, 32, 3, 3), 1501, nonzero=True)
    t = X.nonzero_ints((B, 64, H, W), 1502)
    dy2 = X.ints((B, 128, H, W), 1503)
    _, pdb = ops.pack_pair(wb.to(DEV))
    ds = dy2.clone()
    ds[0, 70, 8, 15] += 1  # input-gradient channel 70 feeds output channels 32..63 only (the block structure)
    conv_budget(ds, wb.flip(2, 3).transpose(0, 1))
    y, _, _ = run_conv(dev4(ds), pdb, B, H, W, ops.SPARSE_HALVES, 128, 64, mask=dev4(t), relu=ops.LEAKY_MASK)
    bad = X.mismatch(y, X.fp32_round(X.dgrad_ref(dd(dy2), dd(wb)) * X.leaky_mask(dd(t))))
    want = torch.zeros_like(bad)
    want[0, 32:, 7:10, 14:16] = True
    assert torch.equal(bad, want)
