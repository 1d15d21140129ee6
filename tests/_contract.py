"""Case table of the autograd operators of ops.py (helper module, not collected; torch only, no HIP import).

One CASE per way an operator backed by a `torch.autograd.Function` is used: a builder of the smallest inputs at which its
kernels still take their interesting paths, the names of its differentiable inputs, and a float64 restatement of the
operation built from the ones the suite already has (_exact.conv_ref / geo_conv_ref, _basic.conv_act, the oracle's block
functions, torch's own float64 operators): float64 autograd over the restatement gives every gradient reference.

Two kinds of data:
  * EXACT: the dyadic operands of tests/_exact.py.  Every gradient here is multilinear in the tensors that enter it (each
    tensor at most once per product), so every term is a multiple of the PRODUCT of the operands' granules, and the
    restatement evaluated on absolute values bounds every partial sum; `budget` asserts that this fits _exact's 22 bits.
    Every correct kernel form then returns the float64 value bit for bit, whatever the launch regime.
  * a tolerance taken from the operator's existing test, named in `cite`.

tests/test_autograd_contract_cpu.py checks the table against ops.py (every Function has a case or an exclusion reason) and
runs every builder, restatement and budget on the host; tests/test_autograd_contract_gpu.py runs the contract.
"""
import importlib

import torch
import torch.nn.functional as F

import _basic as R
import _exact as X
from oracle import sisr_oracle as O

CL = torch.channels_last
B = 2
SIZES = [(13, 9), (9, 33), (2, 1)]  # tile remainders of the conv kernels (test_exact_gpu.SMALL), the 2 x 1 corner
SIZES2 = [(13, 9), (9, 33)]         # operators that need 2 x 2 pixels (reflection padding, pooled attention, statistics),
                                    # and those whose kernels no existing test runs below a few pixels
RSIZES = [(9, 21), (5, 7), (37, 70)]  # _basic.SIZES, the Y-channel / RGB ends' own set (first: the one the contract runs at)
assert sorted(RSIZES) == sorted(R.SIZES)

EXACT = "exact"


def close(r, a):
    """test_hip_gpu.close: |got - want| <= atol * max(1, max|want|) + rtol * |want|, elementwise"""
    return ("close", r, a)


def rel(tol):
    """test_sparnet._rel / test_sftmd_gpu.rel: ||got - want|| / ||want|| < tol"""
    return ("rel", tol)


def allclose(r, a):
    """np.testing.assert_allclose(rtol, atol): |got - want| <= atol + rtol * |want|"""
    return ("allclose", r, a)


def crit(out, inp, par, cite, **by_name):
    return dict(out=out, inp=inp, par=par, cite=cite, by_name=by_name)


# the criteria the existing operator-level tests use, by the test that sets them
RUN_BLOCK = crit(close(2e-4, 3e-5), close(5e-4, 5e-5), close(1e-3, 1e-4),
                 "test_hip_gpu.run_block (test_g1_calayer / _rcab / _qrcab / _paraca / _qca / _palayer / _paramresblock)")
NET_VS_ORACLE = crit(close(5e-4, 5e-5), close(2e-3, 2e-4), close(2e-3, 2e-4),
                     "test_hip_gpu.net_vs_oracle (test_rcan_reduced_vs_oracle, test_qrcan_reduced_vs_oracle: the group node)")
HAN_BLOCK = crit(close(5e-4, 5e-5), close(5e-4, 5e-5), close(1e-3, 1e-4), "test_hip_gpu.test_g1_han_modules")
SOCA_BLOCK = crit(close(3e-4, 3e-5), close(5e-4, 5e-5), close(1e-3, 1e-4), "test_san_gpu.test_s1_soca")
NL_BLOCK = crit(close(2e-4, 2e-5), close(5e-4, 5e-5), rel(2e-5),
                "test_san_gpu.test_nonlocal_block_kernels_vs_the_reference_formulation")
NL_ATTN = crit(close(2e-5, 2e-6), close(1e-4, 1e-5), close(1e-4, 1e-5), "test_san_gpu.test_nonlocal_attention_kernel")
SFT_LAYER = crit(rel(2e-6), rel(5e-6), rel(5e-6), "test_sftmd_gpu.test_sft_layer_matches_the_four_conv_formulation")
SFTMD_NET = crit(allclose(2e-4, 2e-5), rel(5e-5), rel(5e-5), "test_sftmd_gpu.test_other_scales_vs_oracle")
BN_F64 = crit(rel(2e-6), rel(1e-5), rel(1e-5), "test_sparnet.test_hip_batch_norm_act_against_float64")
SPAR_F64 = crit(rel(2e-6), rel(2e-6), rel(2e-6), "test_sparnet.test_hip_spatial_attention_product_against_float64",
                logits=rel(5e-6), identity=rel(1e-7))


class Case:
    """name; functions: the ops.py Function classes the case runs; build(H, W, k) -> {name: CPU fp32 tensor} with the
    cotangent as "cot" (k = 0 / 1: two data sets over the SAME parameters); apply(ops, t) -> output; ref(t) -> float64
    output (differentiable); diff: differentiable inputs; params: those of them that are parameters (leaves an optimiser would
    hold); sink: the parameters whose gradient buffer comes from ops._grad_buf (or the scatter path of meta_gate_many);
    maps: inputs laid out channels-last on the device (cot_map: the cotangent too); consts: scalar factors of the operation,
    for the granule; crit: EXACT or a criterion dict; sizes: (H, W) list, the first is where the contract tests run."""

    def __init__(self, name, functions, build, apply, ref, diff, params=(), sink=(), maps=(), cot_map=True, consts=(),
                 crit=EXACT, sizes=SIZES, rel_scale=None, ref_device=None):
        self.name, self.functions, self.build, self.apply, self.ref = name, tuple(functions), build, apply, ref
        self.diff, self.params, self.sink, self.maps = tuple(diff), tuple(params), tuple(sink), tuple(maps)
        self.cot_map, self.consts, self.crit, self.sizes = cot_map, tuple(consts), crit, list(sizes)
        self.rel_scale = rel_scale or {}
        self.ref_device = ref_device  # "cpu": the restatement builds host tensors of its own (the oracle's sqrtm)
        assert set(self.params) <= set(self.diff) and set(self.sink) <= set(self.params), name

    @property
    def exact(self):
        return self.crit == EXACT

    @property
    def main(self):
        return self.sizes[0]

    def role(self, name):
        return "par" if name in self.params else "inp"

    def __repr__(self):
        return self.name


# ----------------------------------------------------------------------------- running a restatement
def reference(case, t, device="cpu"):
    """float64 output and {name: gradient} of the case's restatement on the tensors `t` (any dtype / device)"""
    device = case.ref_device or device
    t64 = {}
    for n, v in t.items():
        if v is None:
            t64[n] = None
            continue
        d = v.detach().to(device, torch.float64).contiguous()
        t64[n] = d.requires_grad_(True) if n in case.diff else d
    out = case.ref(t64)
    grads = torch.autograd.grad(out, [t64[n] for n in case.diff], t64["cot"], allow_unused=True)
    return out.detach(), {n: (g if g is not None else torch.zeros_like(t64[n])) for n, g in zip(case.diff, grads)}


def budget(case, *ts):
    """EXACT cases: bits of fp32 significand the largest partial sum of the forward pass or of any gradient can need on the
    tensors `ts`, asserted to fit _exact.BUDGET_BITS.  Magnitude: the restatement on absolute values (every ReLU then
    passes, every mask is one); granule: the product of the granules of everything that enters a product.  Several dicts:
    independent applications whose gradients autograd adds (kept gradients, a weight applied twice) -- the magnitudes add,
    the terms keep the granule of one application."""
    assert case.exact
    mag, gran = 0.0, 1.0
    for t in ts:
        ta = {n: (v.abs() if v is not None else None) for n, v in t.items()}
        out, grads = reference(case, ta)
        mag += max([float(out.abs().max())] + [float(g.abs().max()) for g in grads.values() if g.numel()])
        g1 = 1.0
        for v in t.values():
            if v is not None:
                g1 *= X.granule(v)
        for c in case.consts:
            g1 *= X.granule(torch.tensor(float(c)))
        gran = min(gran, g1)
    return X.assert_budget(mag, gran, case.name)


def compare(case, role, name, got, want, what, wants=None):
    """the baseline's criterion: exact, or the cited tolerance of the role (out / inp / par), per-name overrides first;
    wants: every gradient reference of the run (a relative error may be taken on the scale of another input's gradient)"""
    want = want.to(got.device)
    if case.exact:
        return X.assert_exact(got, want, what)
    spec = case.crit["by_name"].get(name, case.crit[role])
    g, w = got.detach().double(), want.double()
    if spec[0] == "rel":
        scale = wants[case.rel_scale[name]].double().norm() if name in case.rel_scale else w.norm()
        err = float((g - w).norm() / (scale + 1e-30))
        assert err < spec[1], f"{what}: relative error {err:.3e} >= {spec[1]:.1e} ({case.crit['cite']})"
        return
    rtol, atol = spec[1], spec[2]
    if spec[0] == "close":
        atol = atol * max(1.0, float(w.abs().max()))
    bad = (g - w).abs() > atol + rtol * w.abs()
    bad |= torch.isnan(g)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside rtol {rtol:g} / atol {atol:g}; "
                                 f"worst |got - want| = {float((g - w).abs().max()):.3e} ({case.crit['cite']})")


def subsets(case):
    """the requires-grad subsets the contract runs: every subset up to four differentiable inputs; for larger operators each
    input frozen alone, each trainable alone, activations only and parameters only (and everything, the baseline)"""
    d = list(case.diff)
    if len(d) <= 4:
        return [tuple(n for i, n in enumerate(d) if m >> i & 1) for m in range(1 << len(d))]
    out = [tuple(d)] + [tuple(n for n in d if n != f) for f in d] + [(n,) for n in d]
    out += [tuple(n for n in d if n not in case.params), tuple(case.params)]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


# ----------------------------------------------------------------------------- data
def xi(shape, seed):
    return X.ints(shape, seed, -1, 1)


def wq(shape, seed):
    """weights k / 8, |k| <= 2"""
    return X.weights(shape, seed, kmax=2)


def wh(shape, seed, zeros=0.5):
    """sparse weights in {-1/2, 0, 1/2}: the deep chains, whose granule is the product over every layer"""
    return X.ints(shape, seed, -1, 1, zeros=zeros) / 2


def bi(n, seed):
    return X.ints((n,), seed, -1, 1)


def rn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ru(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# Soft data meets float64 only up to rounding, and a rectifier turns rounding into a jump: a pre-activation within fp32
# noise of zero may get another mask on the device than in float64 (one such element shows as ~3e-3 in a gradient:
# test_hip_gpu.test_reduced_net_gradients_against_float64_oracle).  The restatements record the smallest |pre-activation| of
# every conv they rectify here; the host test requires PROBE_FLOOR, ten times the fp32 noise (~3e-7) of these 576-term sums
# of magnitude ~1, for both data sets of every size.
PROBE, PROBE_FLOOR = [], 3e-6


def _rect(v, slope=None):
    PROBE.append(float(v.detach().abs().min()))
    return F.relu(v) if slope is None else F.leaky_relu(v, slope)


# data seeds of the soft cases that rectify conv outputs, chosen so that the floor above holds
SEED = {"res_block_ca": 303, "res_block_ca_meta": 303, "gated_group_meta": 521, "gated_group_ca": 521, "sft_layer": 1212,
        "sftmd_head": 1238, "sftmd_tail": 1302}

CASES = []


def family(ops, name):
    """the module `name` beside ops.py (ops_sftmd, ...): private nodes are not re-exported by ops"""
    return importlib.import_module("." + name, ops.__package__)


def case(*a, **k):
    c = Case(*a, **k)
    assert c.name not in [o.name for o in CASES]
    CASES.append(c)
    return c


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ============================================================================ 3 x 3 convs (_Conv3x3: three kinds)
def _conv(name, cin, cout, r=1, residual=False, alpha=1.0, sizes=SIZES, img_in=False, img_out=False):
    def build(H, W, k):
        s = 100 + 17 * k
        t = dict(x=xi((B, cin, H, W), s), w=wq((cout, cin, 3, 3), 1), b=bi(cout, 2),
                 cot=xi((B, cout // (r * r), H * r, W * r), s + 1))
        if residual:
            t["res"] = xi((B, cout, H, W), s + 2)
        return t

    def apply(ops, t):
        return ops.conv3x3(t["x"], t["w"], t["b"], residual=t.get("res"), alpha=alpha, shuffle=r)

    def ref(t):
        y = X.conv_ref(t["x"], t["w"], t["b"])
        if alpha != 1.0:
            y = y * alpha
        if residual:
            y = y + t["res"]
        return F.pixel_shuffle(y, r) if r > 1 else y

    diff = ("x", "w", "b") + (("res",) if residual else ())
    maps = (() if img_in else ("x",)) + (("res",) if residual else ())
    return case(name, ["_Conv3x3"], build, apply, ref, diff, params=("w", "b"), sink=("w", "b"), maps=maps,
                cot_map=not img_out, consts=(alpha,), sizes=sizes)


_conv("conv3x3_c64", 64, 64, residual=True, alpha=0.5)   # fused epilogue; alpha != 1: never queued by deferred_wgrads()
_conv("conv3x3_plain", 64, 64)                           # the queue-eligible form: weight and bias ride in one queued launch
_conv("conv3x3_c128", 128, 64)                      # two input chunks: the multi-chunk K loop and weight-gradient pairs
_conv("conv3x3_shuffle", 64, 256, r=2)              # fused PixelShuffle(2) store, four output chunks
_conv("conv3x3_cin3", 3, 64, sizes=RSIZES, img_in=True)
_conv("conv3x3_cout3", 64, 3, sizes=RSIZES, img_out=True)


# ============================================================================ residual blocks (_ResBlock, _ConvReluConv)
def _block_params(C, seed=10, w=wh):
    return dict(w1=w((C, C, 3, 3), seed), b1=bi(C, seed + 1), w2=w((C, C, 3, 3), seed + 2), b2=bi(C, seed + 3))


def _pair(t, x, alpha=1.0, k=""):
    y = X.conv_ref(_rect(X.conv_ref(x, t["w1" + k], t["b1" + k])), t["w2" + k], t["b2" + k])
    return y if alpha == 1.0 else y * alpha


def _res_block_exact(name, C, meta):
    def build(H, W, k):
        s = 200 + 17 * k
        t = dict(x=xi((B, C, H, W), s), cot=xi((B, C, H, W), s + 1), **_block_params(C))
        if meta:  # the gate's gradient sums dy * r over every pixel: sparser maps keep it inside the budget
            t["x"], t["cot"] = (X.ints((B, C, H, W), s + j, -1, 1, zeros=0.7) for j in (0, 1))
            t["m"] = X.ints((B, 64), s + 2, 1, 3)  # integer gates 1..3: the granule stays the convs'
        return t

    def apply(ops, t):
        return ops.res_block(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], m=t.get("m"), res_scale=0.5)

    def ref(t):  # ResBlock (oracle.res_block) / ParamResBlock (oracle.param_res_block) with the gate given
        r = _pair(t, t["x"], 0.5)
        return (r * t["m"][:, :, None, None] if meta else r) + t["x"]

    P = ("w1", "b1", "w2", "b2")
    return case(name, ["_ResBlock"], build, apply, ref, ("x",) + P + (("m",) if meta else ()), params=P, sink=("w1", "w2"),
                maps=("x",), consts=(0.5,))


_res_block_exact("res_block_plain", 64, False)
_res_block_exact("res_block_plain128", 128, False)   # EDSR-256's form: multi-chunk convs and weight gradients
_res_block_exact("res_block_meta", 64, True)          # the gate is the meta-attention vector alone


def _ca_params(seed, C=64, Rr=4):
    return dict(caw1=rn((Rr, C, 1, 1), seed, 0.2), cab1=rn((Rr,), seed + 1, 0.1), caw2=rn((C, Rr, 1, 1), seed + 2, 0.3),
                cab2=rn((C,), seed + 3, 0.1))


def _ca_gate(t, r, k=""):
    sd = {"ca.conv_du.0.weight": t["caw1" + k], "ca.conv_du.0.bias": t["cab1" + k],
          "ca.conv_du.2.weight": t["caw2" + k], "ca.conv_du.2.bias": t["cab2" + k]}
    return O.ca_gate(sd, "ca", r)


def _soft_block(seed):
    return dict(w1=rn((64, 64, 3, 3), seed, 0.05), b1=rn((64,), seed + 1, 0.1), w2=rn((64, 64, 3, 3), seed + 2, 0.05),
                b2=rn((64,), seed + 3, 0.1))


def _res_block_ca(name, meta):
    def build(H, W, k):
        s = SEED[name] + 17 * k
        t = dict(x=rn((B, 64, H, W), s, 0.5), cot=rn((B, 64, H, W), s + 1), **_soft_block(20), **_ca_params(30))
        if meta:
            t["m"] = torch.sigmoid(rn((B, 64), s + 2))
        return t

    def apply(ops, t):
        return ops.res_block(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], ca=(t["caw1"], t["cab1"], t["caw2"], t["cab2"]),
                             m=t.get("m"))

    def ref(t):  # oracle.rcab / oracle.qrcab('standard', q_layer) with the meta gate given
        r = _pair(t, t["x"])
        g = _ca_gate(t, r)
        return r * (g * t["m"][:, :, None, None] if meta else g) + t["x"]

    P = ("w1", "b1", "w2", "b2", "caw1", "cab1", "caw2", "cab2")
    return case(name, ["_ResBlock"], build, apply, ref, ("x",) + P + (("m",) if meta else ()), params=P, sink=("w1", "w2"),
                maps=("x",), crit=RUN_BLOCK)


_res_block_ca("res_block_ca", False)
_res_block_ca("res_block_ca_meta", True)

case("res_block_convs", ["_ConvReluConv"],
     lambda H, W, k: dict(x=xi((B, 64, H, W), 400 + 17 * k), cot=xi((B, 64, H, W), 401 + 17 * k), **_block_params(64, 40)),
     lambda ops, t: ops.res_block_convs(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], alpha=0.5),
     lambda t: _pair(t, t["x"], 0.5), ("x", "w1", "b1", "w2", "b2"), params=("w1", "b1", "w2", "b2"),
     sink=("w1", "b1", "w2", "b2"), maps=("x",), consts=(0.5,))


# ============================================================================ residual groups (_GatedGroup)
def _group(name, ca, nblocks=2):
    """ca False: QEDSR's blocks (gate = meta vector, alpha = res_scale in conv2's epilogue); ca True: RCAN / QRCAN blocks
    (channel attention, a meta gate on the first block only).  Five convs deep: the product of five layers' granules and
    magnitudes leaves the exact-data budget (45 bits at 64 channels), so both run on soft data to the cited tolerance."""
    keys = [str(k) for k in range(nblocks)]
    alpha = 1.0 if ca else 0.5

    def build(H, W, k):
        s = SEED[name] + 17 * k
        if ca:
            t = dict(x=rn((B, 64, H, W), s, 0.5), cot=rn((B, 64, H, W), s + 1), wt=rn((64, 64, 3, 3), 50, 0.05),
                     bt=rn((64,), 51, 0.1), m0=torch.sigmoid(rn((B, 64), s + 2)))
            for i, q in enumerate(keys):
                t.update({n + q: v for n, v in {**_soft_block(60 + 10 * i), **_ca_params(160 + 10 * i)}.items()})
        else:
            t = dict(x=rn((B, 64, H, W), s, 0.5), cot=rn((B, 64, H, W), s + 1), wt=rn((64, 64, 3, 3), 50, 0.05),
                     bt=rn((64,), 51, 0.1))
            for i, q in enumerate(keys):
                t.update({n + q: v for n, v in _soft_block(60 + 10 * i).items()})
                t["m" + q] = torch.sigmoid(rn((B, 64), s + 3 + i))
        return t

    def blocks(t):
        out = []
        for q in keys:
            gate = (t["caw1" + q], t["cab1" + q], t["caw2" + q], t["cab2" + q]) if ca else None
            out.append((t["w1" + q], t["b1" + q], t["w2" + q], t["b2" + q], gate, t.get("m" + q)))
        return out

    def apply(ops, t):
        return ops.gated_group(t["x"], blocks(t), t["wt"], t["bt"], alpha=alpha)

    def ref(t):  # oracle.residual_group / q_residual_group / the QEDSR body, gates given
        u = t["x"]
        for q in keys:
            r = _pair(t, u, alpha, q)
            g = _ca_gate(t, r, q) if ca else 1.0
            if t.get("m" + q) is not None:
                g = g * t["m" + q][:, :, None, None]
            u = r * g + u
        return X.conv_ref(u, t["wt"], t["bt"]) + t["x"]

    P = ["wt", "bt"]
    for q in keys:
        P += [n + q for n in ("w1", "b1", "w2", "b2")] + ([n + q for n in ("caw1", "cab1", "caw2", "cab2")] if ca else [])
    gates = ["m0"] if ca else ["m" + q for q in keys]
    return case(name, ["_GatedGroup"], build, apply, ref, ["x"] + gates + P, params=P, sink=P, maps=("x",),
                crit=NET_VS_ORACLE, sizes=SIZES2)


_group("gated_group_meta", False)
_group("gated_group_ca", True)


# ============================================================================ plain chains and SPARNet's conv (_ConvChain, _ReflConv)
def _chain(name, widths):
    n = len(widths) - 1
    acts = [1] * (n - 1) + [0]

    def build(H, W, k):
        s = 600 + 17 * k
        t = dict(x=xi((B, 64, H, W), s), cot=xi((B, 64, H, W), s + 1))
        if widths[0] < 64:
            t["x"][:, widths[0]:] = 0
        if widths[-1] < 64:
            t["cot"][:, widths[-1]:] = 0
        for i in range(n):
            t[f"w{i}"], t[f"b{i}"] = wh((widths[i + 1], widths[i], 3, 3), 70 + 2 * i), bi(widths[i + 1], 71 + 2 * i)
        return t

    def apply(ops, t):
        return ops.conv_chain(t["x"], [(t[f"w{i}"], t[f"b{i}"], acts[i]) for i in range(n)])

    def ref(t):  # the C / CR stacks of oracle.srmd on a zero-padded map
        y = t["x"][:, :widths[0]]
        for i in range(n):
            y = X.conv_ref(y, t[f"w{i}"], t[f"b{i}"])
            y = _rect(y) if acts[i] else y
        return F.pad(y, (0, 0, 0, 0, 0, 64 - widths[-1]))

    P = [f"{c}{i}" for i in range(n) for c in "wb"]
    full = all(c == 64 for c in widths)
    return case(name, ["_ConvChain"], build, apply, ref, ["x"] + P, params=P, sink=[f"w{i}" for i in range(n)] if full else (),
                maps=("x",))


_chain("conv_chain", [64, 64, 64])
_chain("conv_chain_padded", [64, 48, 64])  # weights zero-padded per step, gradients cropped back


def _refl(name, up):
    def build(H, W, k):
        s = 700 + 17 * k
        return dict(x=xi((B, 64, H, W), s), w=wq((64, 64, 3, 3), 80), b=bi(64, 81), cot=xi((B, 64, H * up, W * up), s + 1))

    return case(name, ["_ReflConv"], build, lambda ops, t: ops.refl_conv(t["x"], t["w"], t["b"], up=up, stride=1),
                lambda t: X.geo_conv_ref(t["x"], t["w"], t["b"], up=up, stride=1), ("x", "w", "b"), params=("w", "b"),
                sink=("w", "b"), maps=("x",), sizes=SIZES2)


_refl("refl_conv", 1)
_refl("refl_conv_up2", 2)


# ============================================================================ SRCNN / VDSR (_ConvY2F, _ConvF2Y, _ConvKxK)
K5 = 5
case("conv_y2f", ["_ConvY2F"],
     lambda H, W, k: dict(x=xi((B, 1, H, W), 800 + 17 * k), w=wq((64, 1, K5, K5), 90), b=bi(64, 91),
                          cot=xi((B, 64, H, W), 801 + 17 * k)),
     lambda ops, t: ops.conv_y2f(t["x"], t["w"], t["b"], relu=True),
     lambda t: R.conv_act(t["x"], t["w"], t["b"], True), ("w", "b"), params=("w", "b"), sink=("w", "b"), sizes=RSIZES)
case("conv_f2y", ["_ConvF2Y"],
     lambda H, W, k: dict(x=xi((B, 64, H, W), 810 + 17 * k), w=wq((1, 64, K5, K5), 92), b=bi(1, 93),
                          res=xi((B, 1, H, W), 811 + 17 * k), cot=xi((B, 1, H, W), 812 + 17 * k)),
     lambda ops, t: ops.conv_f2y(t["x"], t["w"], t["b"], t["res"]),
     lambda t: R.conv_act(t["x"], t["w"], t["b"], False, t["res"]), ("x", "w", "b", "res"), params=("w", "b"),
     sink=("w", "b"), maps=("x",), cot_map=False, sizes=RSIZES)
case("conv_kxk", ["_ConvKxK"],
     lambda H, W, k: dict(x=xi((B, 64, H, W), 820 + 17 * k), w=wq((64, 64, K5, K5), 94), b=bi(64, 95),
                          cot=xi((B, 64, H, W), 821 + 17 * k)),
     lambda ops, t: ops.conv_kxk(t["x"], t["w"], t["b"], relu=True),
     lambda t: R.conv_act(t["x"], t["w"], t["b"], True), ("x", "w", "b"), params=("w", "b"), sink=("w", "b"), maps=("x",),
     sizes=RSIZES)


# ============================================================================ HAN (_StackMaps, _ConvStack, _LAM, _CSAM)
NMAPS = 3


def _stack_to_nchw(stack):
    b, n, h, w, c = stack.shape
    return stack.permute(0, 1, 4, 2, 3).reshape(b, n * c, h, w)


case("stack_maps", ["_StackMaps"],
     lambda H, W, k: dict(**{f"m{i}": xi((B, 64, H, W), 900 + 17 * k + i) for i in range(NMAPS)},
                          cot=xi((B, NMAPS, H, W, 64), 905 + 17 * k)),
     lambda ops, t: ops.stack_maps([t[f"m{i}"] for i in range(NMAPS)]),
     lambda t: torch.stack([t[f"m{i}"].permute(0, 2, 3, 1) for i in range(NMAPS)], 1),
     [f"m{i}" for i in range(NMAPS)], maps=[f"m{i}" for i in range(NMAPS)], cot_map=False)
case("conv3x3_stack", ["_ConvStack"],
     lambda H, W, k: dict(stack=xi((B, NMAPS, H, W, 64), 910 + 17 * k), w=wq((64, 64 * NMAPS, 3, 3), 100), b=bi(64, 101),
                          res=xi((B, 64, H, W), 911 + 17 * k), cot=xi((B, 64, H, W), 912 + 17 * k)),
     lambda ops, t: ops.conv3x3_stack(t["stack"], t["w"], t["b"], residual=t["res"]),
     lambda t: X.conv_ref(_stack_to_nchw(t["stack"]), t["w"], t["b"]) + t["res"], ("stack", "w", "b", "res"),
     params=("w", "b"), maps=("res",))


def _lam_ref(t):
    b, n, h, w, c = t["stack"].shape
    out = O.lam_module({"la.gamma": t["gamma"]}, "la", t["stack"].permute(0, 1, 4, 2, 3))
    return out.reshape(b, n, c, h, w).permute(0, 1, 3, 4, 2)


case("lam", ["_LAM"],
     lambda H, W, k: dict(stack=rn((B, NMAPS, H, W, 64), 920 + 17 * k, 0.05), gamma=torch.tensor([0.5]),
                          cot=rn((B, NMAPS, H, W, 64), 921 + 17 * k)),
     lambda ops, t: ops.lam(t["stack"], t["gamma"]), _lam_ref, ("stack", "gamma"), params=("gamma",), cot_map=False,
     crit=HAN_BLOCK, sizes=SIZES2)
case("csam", ["_CSAM"],
     lambda H, W, k: dict(x=rn((B, 64, H, W), 930 + 17 * k, 0.5), w=rn((1, 1, 3, 3, 3), 110, 0.3), b=rn((1,), 111, 0.1),
                          gamma=torch.tensor([0.37]), cot=rn((B, 64, H, W), 931 + 17 * k)),
     lambda ops, t: ops.csam(t["x"], t["w"], t["b"], t["gamma"]),
     lambda t: O.csam_module({"c.conv.weight": t["w"], "c.conv.bias": t["b"], "c.gamma": t["gamma"]}, "c", t["x"]),
     ("x", "w", "b", "gamma"), params=("w", "b", "gamma"), maps=("x",), crit=HAN_BLOCK)


# ============================================================================ stand-alone gates
def _meta_params(seed, M=10, Hd=32, C=64, k=""):
    return {"v1" + k: rn((Hd, M, 1, 1), seed, 0.3), "c1" + k: rn((Hd,), seed + 1, 0.1), "v2" + k: rn((C, Hd, 1, 1), seed + 2, 0.3),
            "c2" + k: rn((C,), seed + 3, 0.1)}


def _meta_ref(t, k=""):
    sd = {"q.attribute_integrator.0.weight": t["v1" + k], "q.attribute_integrator.0.bias": t["c1" + k],
          "q.attribute_integrator.2.weight": t["v2" + k], "q.attribute_integrator.2.bias": t["c2" + k]}
    return O.para_ca_gate(sd, "q", t["md"], nonlinearity=True).flatten(1)


case("meta_gate", ["_MetaGate"],
     lambda H, W, k: dict(md=rn((B, 10, 1, 1), 1000 + 17 * k, 0.3), cot=rn((B, 64), 1001 + 17 * k), **_meta_params(120)),
     lambda ops, t: ops.meta_gate(t["md"], t["v1"], t["c1"], t["v2"], t["c2"], True), _meta_ref,
     ("md", "v1", "c1", "v2", "c2"), params=("v1", "c1", "v2", "c2"), cot_map=False, crit=RUN_BLOCK, sizes=[(13, 9)])
_MANY = [n + q for q in "01" for n in ("v1", "c1", "v2", "c2")]
case("meta_gate_many", ["_MetaGateMany"],
     lambda H, W, k: dict(md=rn((B, 10, 1, 1), 1010 + 17 * k, 0.3), cot=rn((2, B, 64), 1011 + 17 * k),
                          **_meta_params(130, k="0"), **_meta_params(140, k="1")),
     lambda ops, t: torch.stack(ops.meta_gate_many(t["md"], [tuple(t[n + q] for n in ("v1", "c1", "v2", "c2")) for q in "01"],
                                                   True)),
     lambda t: torch.stack([_meta_ref(t, q) for q in "01"]), _MANY, params=_MANY, sink=_MANY, cot_map=False, crit=RUN_BLOCK,
     sizes=[(13, 9)])


def _qca_ref(t):  # oracle.qca_layer('max_concat') up to the gate, times the folded-in meta gate
    y = torch.cat((t["pool"], t["md"]), dim=1)
    y = torch.sigmoid(F.conv2d(F.relu(F.conv2d(y, t["w0"], t["b0"])), t["w1"], t["b1"]))
    return y * t["mul"][:, :, None, None]


case("qca_gate", ["_GateMlp"],
     lambda H, W, k: dict(pool=rn((B, 64, 1, 1), 1020 + 17 * k, 0.5), md=rn((B, 10, 1, 1), 1021 + 17 * k, 0.3),
                          mul=torch.sigmoid(rn((B, 64), 1022 + 17 * k)), w0=rn((4, 74, 1, 1), 150, 0.2), b0=rn((4,), 151, 0.1),
                          w1=rn((64, 4, 1, 1), 152, 0.3), b1=rn((64,), 153, 0.1), cot=rn((B, 64, 1, 1), 1023 + 17 * k)),
     lambda ops, t: ops._GateMlp.apply(t["pool"], t["md"], t["mul"], ops.QCA_STYLES["max_concat"], t["w0"], t["b0"], t["w1"],
                                       t["b1"]),
     _qca_ref, ("pool", "md", "mul", "w0", "b0", "w1", "b1"), params=("w0", "b0", "w1", "b1"), cot_map=False, crit=RUN_BLOCK,
     sizes=[(13, 9)])
case("ca_layer", ["_CALayer"],
     lambda H, W, k: dict(x=rn((B, 64, H, W), 1030 + 17 * k, 0.5), cot=rn((B, 64, H, W), 1031 + 17 * k), **_ca_params(170)),
     lambda ops, t: ops.ca_layer(t["x"], t["caw1"], t["cab1"], t["caw2"], t["cab2"]),
     lambda t: t["x"] * _ca_gate(t, t["x"]), ("x", "caw1", "cab1", "caw2", "cab2"),
     params=("caw1", "cab1", "caw2", "cab2"), maps=("x",), crit=RUN_BLOCK)
case("pa_layer", ["_PALayer"],
     lambda H, W, k: dict(x=rn((B, 64, H, W), 1040 + 17 * k, 0.5), w1=rn((8, 64, 1, 1), 180, 0.2), b1=rn((8,), 181, 0.1),
                          w2=rn((1, 8, 1, 1), 182, 0.3), b2=rn((1,), 183, 0.1), cot=rn((B, 64, H, W), 1041 + 17 * k)),
     lambda ops, t: ops.pa_layer(t["x"], t["w1"], t["b1"], t["w2"], t["b2"]),
     lambda t: O.pa_layer({"p.pa.0.weight": t["w1"], "p.pa.0.bias": t["b1"], "p.pa.2.weight": t["w2"], "p.pa.2.bias": t["b2"]},
                          "p", t["x"]),
     ("x", "w1", "b1", "w2", "b2"), params=("w1", "b1", "w2", "b2"), maps=("x",), crit=RUN_BLOCK)
case("gate_mul", ["_GateMul"],
     lambda H, W, k: dict(t=xi((B, 64, H, W), 1050 + 17 * k), g=X.scales((B, 64, 1, 1), 1051 + 17 * k),
                          x=xi((B, 64, H, W), 1052 + 17 * k), cot=xi((B, 64, H, W), 1053 + 17 * k)),
     lambda ops, t: ops.gate_mul(t["t"], t["g"], t["x"]), lambda t: t["t"] * t["g"] + t["x"], ("t", "g", "x"),
     maps=("t", "x"))
case("add_residual", ["_AddResidual"],
     lambda H, W, k: dict(t=xi((B, 64, H, W), 1060 + 17 * k), x=xi((B, 64, H, W), 1061 + 17 * k),
                          cot=xi((B, 64, H, W), 1062 + 17 * k)),
     lambda ops, t: ops.add_residual(t["t"], t["x"]), lambda t: t["t"] + t["x"], ("t", "x"), maps=("t", "x"))
case("scale_add", ["_ScaleAdd"],
     lambda H, W, k: dict(a=xi((B, 64, H, W), 1070 + 17 * k), r=xi((B, 64, H, W), 1071 + 17 * k), gamma=torch.tensor([0.5]),
                          cot=xi((B, 64, H, W), 1072 + 17 * k)),
     lambda ops, t: ops.scale_add(t["a"], t["r"], t["gamma"]), lambda t: t["a"] + t["gamma"] * t["r"], ("a", "r", "gamma"),
     params=("gamma",), maps=("a", "r"))


# ============================================================================ SAN (_SOCA, _NonLocalAttention, _NonLocalBlock)
case("soca", ["_SOCA"],
     lambda H, W, k: dict(x=rn((B, 64, H, W), 1100 + 17 * k, 0.5), cot=rn((B, 64, H, W), 1101 + 17 * k), **_ca_params(190)),
     lambda ops, t: ops.soca(t["x"], t["caw1"], t["cab1"], t["caw2"], t["cab2"]),
     lambda t: O.soca({"s.conv_du.0.weight": t["caw1"], "s.conv_du.0.bias": t["cab1"], "s.conv_du.2.weight": t["caw2"],
                       "s.conv_du.2.bias": t["cab2"]}, "s", t["x"]),
     ("x", "caw1", "cab1", "caw2", "cab2"), params=("caw1", "cab1", "caw2", "cab2"), maps=("x",), crit=SOCA_BLOCK,
     sizes=SIZES2, ref_device="cpu")
case("nonlocal_attention", ["_NonLocalAttention"],
     lambda H, W, k: dict(theta=rn((B, H * W, 8), 1110 + 17 * k), phi=rn((B, 12, 8), 1111 + 17 * k),
                          g=rn((B, 12, 8), 1112 + 17 * k), cot=rn((B, H * W, 8), 1113 + 17 * k)),
     lambda ops, t: ops.nonlocal_attention(t["theta"], t["phi"], t["g"]),
     lambda t: torch.softmax(t["theta"] @ t["phi"].transpose(1, 2), dim=-1) @ t["g"], ("theta", "phi", "g"), cot_map=False,
     crit=NL_ATTN, sizes=SIZES2)
_NLP = ("wt", "bt", "wp", "bp", "wg", "bg", "ww", "bw")


def _nl(name, quadrants):
    def build(H, W, k):
        s = 1120 + 17 * k
        t = dict(x=rn((B, 64, H, W), s), cot=rn((B, 64, H, W), s + 1))
        for i, n in enumerate(("t", "p", "g")):
            t["w" + n], t["b" + n] = rn((8, 64, 1, 1), 200 + 2 * i, 0.3), rn((8,), 201 + 2 * i, 0.3)
        t["ww"], t["bw"] = rn((64, 8, 1, 1), 210, 0.3), rn((64,), 211, 0.3)
        return t

    def ref(t):
        sd = {"n.non_local.theta.weight": t["wt"], "n.non_local.theta.bias": t["bt"], "n.non_local.phi.0.weight": t["wp"],
              "n.non_local.phi.0.bias": t["bp"], "n.non_local.g.0.weight": t["wg"], "n.non_local.g.0.bias": t["bg"],
              "n.non_local.W.weight": t["ww"], "n.non_local.W.bias": t["bw"]}
        return O.nonlocal_ca(sd, "n", t["x"]) if quadrants else O.nonlocal_block(sd, "n.non_local", t["x"])

    # phi's bias shifts every logit of a row alike: its exact gradient is 0, so it is compared on the scale of phi's weight
    # gradient, as the cited test does
    return case(name, ["_NonLocalBlock"], build,
                lambda ops, t: family(ops, "ops_attention")._NonLocalBlock.apply(t["x"], quadrants, *[t[n] for n in _NLP]), ref, ("x",) + _NLP,
                params=_NLP, maps=("x",), crit=NL_BLOCK, sizes=SIZES2, rel_scale={"bp": "wp"})


_nl("nonlocal_block", False)
_nl("nonlocal_block_quadrants", True)


# ============================================================================ SFTMD (_SftLayer, _ConcatSft, _SftmdHead, _SftmdTail)
MD = 10
_SFT = ("mw1", "mb1", "aw1", "ab1", "mw2", "mb2", "aw2", "ab2")


def _sft_build(H, W, k):
    s = SEED["sft_layer"] + 17 * k
    t = dict(x=rn((B, 64, H, W), s), md=ru((B, MD, H, W), s + 1), cot=rn((B, 64, H, W), s + 2))
    for i, p in enumerate(("m", "a")):
        t[p + "w1"], t[p + "b1"] = rn((32, 64 + MD, 3, 3), 220 + 4 * i, 0.04), rn((32,), 221 + 4 * i, 0.04)
        t[p + "w2"], t[p + "b2"] = rn((64, 32, 3, 3), 222 + 4 * i, 0.06), rn((64,), 223 + 4 * i, 0.06)
    return t


def _sft_ref(t):  # StandardSft as the reference writes it (test_sft_layer_matches_the_four_conv_formulation), + the block's ReLU
    cat = torch.cat((t["x"], t["md"]), 1)
    mul = torch.sigmoid(X.conv_ref(_rect(X.conv_ref(cat, t["mw1"], t["mb1"]), 0.2), t["mw2"], t["mb2"]))
    add = X.conv_ref(_rect(X.conv_ref(cat, t["aw1"], t["ab1"]), 0.2), t["aw2"], t["ab2"])
    return _rect(t["x"] * mul + add)


case("sft_layer", ["_SftLayer"], _sft_build,
     lambda ops, t: family(ops, "ops_sftmd")._SftLayer.apply(t["x"], ops.nchw_to_nhwc_pad(t["md"], 64), True, MD, *[t[n] for n in _SFT]), _sft_ref,
     ("x",) + _SFT, params=_SFT, maps=("x",), crit=SFT_LAYER, sizes=SIZES2)
case("concat_sft", ["_ConcatSft"],
     lambda H, W, k: dict(x=xi((B, 64, H, W), 1210 + 17 * k), md=xi((B, MD, H, W), 1211 + 17 * k),
                          w=wq((64, 64 + MD, 3, 3), 230), b=bi(64, 231), cot=xi((B, 64, H, W), 1212 + 17 * k)),
     lambda ops, t: family(ops, "ops_sftmd")._ConcatSft.apply(t["x"], ops.nchw_to_nhwc_pad(t["md"], 64), t["w"], t["b"]),
     lambda t: X.conv_ref(torch.cat((t["x"], t["md"]), 1), t["w"], t["b"]), ("x", "w", "b"), params=("w", "b"), maps=("x",))
_HEAD = ("w1", "b1", "w2", "b2", "w3", "b3")


def _head_ref(t):  # oracle.sftmd's first three convs
    y = _rect(X.conv_ref(t["x"], t["w1"], t["b1"]), 0.2)
    return X.conv_ref(_rect(X.conv_ref(y, t["w2"], t["b2"]), 0.2), t["w3"], t["b3"])


case("sftmd_head", ["_SftmdHead"],
     lambda H, W, k: dict(x=ru((B, 3, H, W), SEED["sftmd_head"] + 17 * k), w1=rn((64, 3, 3, 3), 240, 0.2), b1=rn((64,), 241, 0.1),
                          w2=rn((64, 64, 3, 3), 242, 0.05), b2=rn((64,), 243, 0.1), w3=rn((64, 64, 3, 3), 244, 0.05),
                          b3=rn((64,), 245, 0.1), cot=rn((B, 64, H, W), SEED["sftmd_head"] + 1 + 17 * k)),
     lambda ops, t: family(ops, "ops_sftmd")._SftmdHead.apply(t["x"], *[t[n] for n in _HEAD]), _head_ref, _HEAD, params=_HEAD, sink=("w2", "w3"),
     crit=SFTMD_NET, sizes=RSIZES[:2])  # (at 37 x 70 two convs rectify 660 000 sums: no seed keeps them all off zero)
_TAIL = ("wm", "bm", "wu", "bu", "wo", "bo")


def _tail_ref(t):  # oracle.sftmd's conv_mid -> conv, PixelShuffle(2), LeakyReLU -> 9 x 9 conv -> clamp
    m = X.conv_ref(t["fea"], t["wm"], t["bm"])
    u = _rect(F.pixel_shuffle(X.conv_ref(m, t["wu"], t["bu"]), 2), 0.2)
    return X.conv_ref(u, t["wo"], t["bo"]).clamp(0, 1)


case("sftmd_tail", ["_SftmdTail"],
     lambda H, W, k: dict(fea=rn((B, 64, H, W), SEED["sftmd_tail"] + 17 * k, 0.5), wm=rn((64, 64, 3, 3), 250, 0.05), bm=rn((64,), 251, 0.1),
                          wu=rn((256, 64, 3, 3), 252, 0.05), bu=rn((256,), 253, 0.1), wo=rn((3, 64, 9, 9), 254, 0.01),
                          bo=torch.full((3,), 0.5), cot=rn((B, 3, 2 * H, 2 * W), SEED["sftmd_tail"] + 1 + 17 * k)),
     lambda ops, t: family(ops, "ops_sftmd")._SftmdTail.apply(t["fea"], 1, *[t[n] for n in _TAIL]), _tail_ref, ("fea",) + _TAIL, params=_TAIL,
     sink=("wm", "wu"), maps=("fea",), cot_map=False, crit=SFTMD_NET, sizes=SIZES2)


# ============================================================================ SPARNet (_BatchNormAct, _GroupNorm, _Act, _SparCombine, _Spar3d)
def _affine(seed):
    return dict(gamma=ru((64,), seed) + 0.5, beta=rn((64,), seed + 1, 0.3))


case("batch_norm_act", ["_BatchNormAct"],
     lambda H, W, k: dict(x=rn((B, 64, H, W), 1300 + 17 * k, 1.7) + 0.4, cot=rn((B, 64, H, W), 1301 + 17 * k), **_affine(260)),
     lambda ops, t: family(ops, "ops_sparnet")._BatchNormAct.apply(t["x"], t["gamma"], t["beta"], None, None, True, 0.0, 1e-5, 0.2),
     lambda t: F.leaky_relu(F.batch_norm(t["x"], None, None, t["gamma"], t["beta"], True, 0.0, 1e-5), 0.2),
     ("x", "gamma", "beta"), params=("gamma", "beta"), maps=("x",), crit=BN_F64, sizes=SIZES2)
# group statistics are the batch-norm kernels' arithmetic over another index set; the per-kernel bounds of
# test_spar_han_gpu are rounding models of single launches, so the operator is held to its sibling's float64 criterion
case("group_norm", ["_GroupNorm"],
     lambda H, W, k: dict(x=rn((B, 64, H, W), 1310 + 17 * k, 1.7) + 0.4, cot=rn((B, 64, H, W), 1311 + 17 * k), **_affine(270)),
     lambda ops, t: ops.group_norm(t["x"], t["gamma"], t["beta"], 2, 1e-5),
     lambda t: F.group_norm(t["x"], 32, t["gamma"], t["beta"], 1e-5), ("x", "gamma", "beta"), params=("gamma", "beta"),
     maps=("x",), crit=dict(BN_F64, cite=BN_F64["cite"] + " (the sibling normalisation)"), sizes=SIZES2)
case("prelu", ["_Act"],  # dyadic slopes: exact, as test_spar_han_gpu's ops.prelu test
     lambda H, W, k: dict(x=X.nonzero_ints((B, 64, H, W), 1320 + 17 * k, 2), a=X.ints((64,), 280, 1, 3) / 4,
                          cot=xi((B, 64, H, W), 1321 + 17 * k)),
     lambda ops, t: ops.prelu(t["x"], t["a"]), lambda t: F.prelu(t["x"], t["a"]), ("x", "a"), params=("a",), maps=("x",))

case("spar_combine", ["_SparCombine"],  # logits: channels 1.. are the conv's padding and must be ignored
     lambda H, W, k: dict(x=rn((B, 64, H, W), 1330 + 17 * k), logits=rn((B, 64, H, W), 1331 + 17 * k),
                          identity=rn((B, 64, H, W), 1332 + 17 * k), cot=rn((B, 64, H, W), 1333 + 17 * k)),
     lambda ops, t: ops.spar_combine(t["x"], t["logits"], t["identity"]),
     lambda t: t["x"] * torch.sigmoid(t["logits"][:, :1]) + t["identity"], ("x", "logits", "identity"),
     maps=("x", "logits", "identity"), crit=SPAR_F64)
case("spar_combine3d", ["_Spar3d"],  # the elementwise form of the same product: its sibling's float64 criterion
     lambda H, W, k: dict(x=rn((B, 64, H, W), 1340 + 17 * k), logits=rn((B, 64, H, W), 1341 + 17 * k),
                          identity=rn((B, 64, H, W), 1342 + 17 * k), cot=rn((B, 64, H, W), 1343 + 17 * k)),
     lambda ops, t: ops.spar_combine3d(t["x"], t["logits"], t["identity"]),
     lambda t: t["x"] * torch.sigmoid(t["logits"]) + t["identity"], ("x", "logits", "identity"),
     maps=("x", "logits", "identity"), crit=dict(SPAR_F64, cite=SPAR_F64["cite"] + " (the sibling product)"))


# ============================================================================ what has no case, and why
EXCLUDED = {
    "_PadAxis": "no parameters and one input (the zero-padding step of pad_param; pinned by test_glue_gpu)",
    "_Map64": "no parameters and one differentiable input (the metadata map takes no gradient)",
    "_PixelNorm": "no parameters and one input",
    "_NearestUp": "no parameters and one input",
    "_ShuffleRGB": "no parameters and one input",
    "_PixelShuffleCL": "no parameters and one input",
    "_GlobalAvgPool": "no parameters and one input",
    "_FrozenFeatures": "one differentiable input; its weights are frozen by construction (FrozenChain refuses trainable ones)",
    "_L1Loss": "no parameters and one differentiable input (the target takes no gradient), scalar output",
    "_MSELoss": "no parameters and one differentiable input (the target takes no gradient), scalar output",
    "_SsimMean": "no parameters and one differentiable input (the target is refused if it requires grad), scalar output",
    "_MsSsimMean": "no parameters and one differentiable input (the target is refused if it requires grad), scalar output",
    "_ConvKxKS2": "convs.py's stride-2 node: its contract is held by tests/test_convs_contract_gpu.py",
    "_Conv1x1": "convs.py's pointwise node: its contract is held by tests/test_convs_contract_gpu.py",
    "_SpectralL1": "no parameters and one differentiable input (the target is refused if it requires grad), scalar output",
    "_DenseBlock": "ops_dense.py's block node, ten parameters on one stack: its contract is held by tests/test_dense_contract_gpu.py",
    "_DenseSkip": "ops_dense.py's skip between stacks: its contract is held by tests/test_dense_contract_gpu.py",
    "_MapMean": "no parameters and one input (pool.py's global mean; pinned against float64 by test_predictor_gpu)",
    "DegradeValid": "no parameters and one differentiable input (K is refused if it requires grad); held by test_consistency_gpu.py",
}

# the operators whose weight-gradient buffers come from ops._grad_buf: each must have a case with a `sink`
GRAD_BUF_USERS = ("_Conv3x3", "_ResBlock", "_GatedGroup", "_ConvReluConv", "_ConvChain", "_ReflConv", "_SftmdHead",
                  "_SftmdTail", "_ConvY2F", "_ConvF2Y", "_ConvKxK")
# ... and the EXCLUDED ones that take such buffers too: the file that runs their sink and shared-weight cases
GRAD_BUF_USERS_ELSEWHERE = {"_ConvKxKS2": "tests/test_convs_contract_gpu.py", "_Conv1x1": "tests/test_convs_contract_gpu.py",
                            "_DenseBlock": "tests/test_dense_contract_gpu.py"}
