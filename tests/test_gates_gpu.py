"""The attention-gate, pixel-sum, gated-residual, pixel-attention and L1 kernels against float64 (pytest -m gpu).

The native entry points are called directly (shapes, partial counts and null arguments chosen freely), then once through
each ops wrapper.  References are tests/_gates.py (checked against the oracle's autograd by tests/test_gates_cpu.py).
Every output buffer starts as NaN, so an element the kernel never writes fails.  Two tiers:

1. Exact (zero tolerance).  Outputs that are only sums and products of operands, on dyadic data (tests/_exact.py), each
   comparison preceded by a budget check (every partial sum fits fp32's significand, so any summation order is exact):
   the pixel partials and their reduction (`scale` is one fp32 multiply of the exact sum: the reference is
   fl32(exact) * fl32(scale) in fp32), the gated residual, the CA gate's s / hid, every backward fed dyadic saved
   activations (CA gate, its parameter-gradient batch, meta gate, gate MLP: a sigmoid output s is an input there and
   s * (1 - s) is exact for s in {1/4, 1/2, 3/4}), the L1 value and gradient.
2. Bounded.  Everything behind expf: |got - ref| <= c * 2^-24 * mag, mag the same float64 computation on absolute values
   (tests/_gates.py, `A=True`), c per family:
     C_SIG = 8      a sigmoid of an exact argument (expf, 1 + e, 1 / .), times at most one more factor;
     C_SOFTMAX = 64 the softmax style: the sigmoid, exp, and an up-to-512-term sequential fp32 sum;
     C_CHAIN = 64   backward passes fed the kernels' own sigmoid outputs (fp32 contractions of up to 300 terms behind);
     C_PA = 64      pixel attention's backward (per-block partials of up to 49157 pixels, then 1024 block sums);
     C_L1 = 2       the L1 gradient sign / n as the kernel forms 1 / n (1.0f / (float)n); its value C_L1 + 1.
   The golden block tests bound these kernels at 2e-4 to 1e-3 of the max; 64 * 2^-24 = 3.8e-6 of the magnitude.

Each family has a detector: one input or weight element moved in what the kernel sees only must make the exact comparison
mismatch at exactly the outputs that element feeds, or make the bounded comparison fail.
"""
import ctypes
import types

import pytest
import torch

import _exact as X
import _gates as G
import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
NAN = float("nan")
ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -4
C_SIG, C_SOFTMAX, C_CHAIN, C_PA = 8, 64, 64, 64
C_L1 = 2 + 2 ** -20  # the L1 gradient fl32(1 / fl32(n)): two roundings; its value one more


def lib():
    return hip.lib()


def P(t):
    return hip.ptr(t)


def S():
    return hip.stream()


def nan(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def dev(t):
    return t.to(DEV, torch.float32).contiguous()


def dd(t):
    return t.to(DEV, torch.float64)


def mm_budget(a, b, what, extra=None):
    """budget of the contraction a @ b [+ extra] of exact operands (partial sums are multiples of gran(a) * gran(b))"""
    a, b = dd(a), dd(b)
    mag = a.abs() @ b.abs()
    gran = X.granule(a) * X.granule(b)
    if extra is not None:
        mag, gran = mag + dd(extra).abs(), min(gran, X.granule(extra))
    return X.assert_budget(mag, gran, what)


def val_budget(t, what):
    """an elementwise product that must itself be exact in fp32"""
    return X.assert_budget(dd(t).abs(), X.granule(dd(t)), what)


def sparse_ints(shape, seed, per_col, n):
    """ints in {-1, 0, 1} with about per_col non-zeros along an axis of length n"""
    return X.ints(shape, seed, -1, 1, zeros=max(0.3, 1.0 - per_col / n))


def expect_detected(got_map, want_map, what):
    assert bool(want_map.any()), f"{what}: the perturbation changes no output (test bug)"
    assert torch.equal(got_map.cpu(), want_map.cpu()), \
        f"{what}: {int(got_map.sum())} mismatches, {int(want_map.sum())} expected, or at other outputs"


# ============================================================================ 1. CA gate (C = 64)
INV_HW = 1.0 / 16  # a power of two: s = fl32(S) * inv_hw is exact


class CaData:
    def __init__(self, parts, R, B, with_mul, seed):
        self.parts, self.R, self.B = parts, R, B
        self.part = X.ints((B, parts, 64), seed, -1, 1, zeros=0.3 if parts <= 512 else 0.9)
        self.w1, self.b1 = X.weights((R, 64), seed + 1), X.biases(R, seed + 2)
        self.w2, self.b2 = X.weights((64, R), seed + 3), X.biases(64, seed + 4)
        self.mul = X.scales((B, 64), seed + 5) if with_mul else None
        # backward: dyadic saved activations (ca in {1/4, 1/2, 3/4}, hid >= 0 with zeros, s k/4), sparse dg partials
        self.dgpart = sparse_ints((B, parts, 64), seed + 6, 8, parts)
        self.ca = X.ints((B, 64), seed + 7, 1, 3) / 4
        self.hid = X.ints((B, R), seed + 8, 0, 2, zeros=0.3) / 2
        self.s = X.ints((B, 64), seed + 9, -1, 1) / 4
        self.bw1, self.bw2 = X.ints((R, 64), seed + 10, -1, 1) / 8, X.ints((64, R), seed + 11, -1, 1) / 8
        self.d = {k: dev(v) for k, v in vars(self).items() if torch.is_tensor(v)}
        self.d["mul"] = dev(self.mul) if with_mul else None


def ca_fwd_exact_ref(D, part=None):
    part = D.part if part is None else part
    s = dd(part).sum(1) * INV_HW
    ref = G.ca_fwd_ref(s, dd(D.w1), dd(D.b1), dd(D.w2), dd(D.b2), None if D.mul is None else dd(D.mul))
    ref["s"] = s
    return ref


def ca_fwd_run(D, part=None, w=None):
    B, R = D.B, D.R
    out = dict(s=nan(B, 64), hid=nan(B, R), ca=nan(B, 64), g=nan(B, 64))
    w1, b1, w2, b2 = w if w is not None else (D.d["w1"], D.d["b1"], D.d["w2"], D.d["b2"])
    rc = lib().sisr_ca_gate_fwd(P(D.d["part"] if part is None else part), D.parts, B, INV_HW, P(w1), P(b1), P(w2), P(b2),
                                64, R, P(D.d["mul"]), P(out["s"]), P(out["hid"]), P(out["ca"]), P(out["g"]), S())
    hip.check(rc, "sisr_ca_gate_fwd")
    return out


def ca_bwd_run(D, params=True, counter=None, dgpart=None):
    B, R = D.B, D.R
    o = dict(shift=nan(B, 64), dmul=nan(B, 64) if D.mul is not None else None, ws=nan(B, 80))
    if params:
        o.update(dw1=nan(R, 64), db1=nan(R), dw2=nan(64, R), db2=nan(64))
    d = D.d
    rc = lib().sisr_ca_gate_bwd(P(d["dgpart"] if dgpart is None else dgpart), D.parts, B, INV_HW, P(d["bw1"]), P(d["bw2"]),
                                64, R, P(d["s"]), P(d["hid"]), P(d["ca"]), P(d["mul"]), P(o["shift"]), P(o["dmul"]),
                                P(o.get("dw1")), P(o.get("db1")), P(o.get("dw2")), P(o.get("db2")), P(o["ws"]),
                                (counter or hip.gate_counter(torch.device(DEV))) if params else None, S())
    hip.check(rc, "sisr_ca_gate_bwd")
    return o


def ca_bwd_exact_ref(D, dgpart=None):
    dg = dd(D.dgpart if dgpart is None else dgpart).sum(1)
    ref = G.ca_bwd_ref(dg, dd(D.ca), dd(D.hid), dd(D.s), dd(D.bw1), dd(D.bw2), None if D.mul is None else dd(D.mul), INV_HW)
    dca = dg * dd(D.mul) if D.mul is not None else dg
    val_budget(dca * dd(D.ca) * (1 - dd(D.ca)), "CA dz2")
    mm_budget(ref["dz2"], dd(D.bw2), "CA dh = W2^T dz2")
    mm_budget(ref["dz1"], dd(D.bw1), "CA ds = W1^T dz1")
    mm_budget(ref["dz2"].T, dd(D.hid), "CA dw2")
    mm_budget(ref["dz1"].T, dd(D.s), "CA dw1")
    return ref


def params_batch(jobs_list, B, R):
    jobs = (hip.CaParamJob * len(jobs_list))()
    for k, j in enumerate(jobs_list):
        for f in ("dz", "hid", "s", "dw1", "db1", "dw2", "db2"):
            setattr(jobs[k], f, P(j[f]))
    return lib().sisr_ca_gate_bwd_params_batch(ctypes.addressof(jobs), len(jobs_list), B, R, S())


# (parts, R, B, mul).  block_sum_parts: thread group k = 0..15 takes its 16-load unrolled round while k + 240 < parts,
# then single rows: parts 1 / 15 / 16 / 17 (groups idle or one row), 240 | 241 (group 0's first unrolled round), 256 | 257
# (every group's round / one row past), 497 (group 0: a second round, 256 + 240 < 497), 4096 (16 rounds).
# R <= 4 takes the register ("pre") path, R > 4 the loop path; R <= 16 accepted (17 refused: test below).
# ca_gate_bwd_params' dot_b: 8-wide batch blocks while bb + 8 <= B, then a remainder loop: B 7 | 8 | 9, 33 = 4 * 8 + 1.
CA_CASES = [(1, 4, 2, False), (15, 1, 1, True), (16, 3, 7, False), (17, 4, 8, True), (240, 5, 9, False), (241, 8, 33, True),
            (256, 16, 2, False), (257, 4, 3, True), (497, 3, 2, False), (4096, 16, 2, True),
            (20, 1, 9, True), (20, 3, 33, False), (20, 4, 7, True), (20, 5, 8, False), (20, 8, 1, True), (20, 16, 9, True)]


@pytest.mark.parametrize("parts,R,B,with_mul", CA_CASES)
def test_ca_gate_forward(parts, R, B, with_mul):
    D = CaData(parts, R, B, with_mul, seed=parts * 7 + R)
    ref = ca_fwd_exact_ref(D)
    mag = G.ca_fwd_mag(ref["s"], dd(D.w1), dd(D.b1), dd(D.w2), dd(D.b2))
    X.assert_budget(dd(D.part).abs().sum(1), 1.0, "CA pixel sum")
    X.assert_budget(mag["pre"], X.granule(ref["s"]) * X.granule(dd(D.w1)), "CA pre")
    X.assert_budget(mag["z"], min(X.granule(ref["hid"]) * X.granule(dd(D.w2)), X.granule(dd(D.b2))), "CA z")
    out = ca_fwd_run(D)
    X.assert_exact(out["s"], ref["s"], "s")
    X.assert_exact(out["hid"], ref["hid"], "hid")
    G.assert_bounded(out["ca"], ref["ca"], ref["ca"], C_SIG, "ca")
    G.assert_bounded(out["g"], ref["g"], ref["g"].abs(), C_SIG, "g")


@pytest.mark.parametrize("parts,R,B,with_mul", CA_CASES)
def test_ca_gate_backward_in_kernel_and_deferred(parts, R, B, with_mul):
    """exact on dyadic saved activations; the in-kernel parameter gradients equal the deferred form +
    sisr_ca_gate_bwd_params_batch bit for bit (both run ca_gate_bwd_params)"""
    D = CaData(parts, R, B, with_mul, seed=parts * 5 + R + 1)
    ref = ca_bwd_exact_ref(D)
    o = ca_bwd_run(D)
    X.assert_exact(o["shift"], ref["shift"], "shift")
    if with_mul:
        X.assert_exact(o["dmul"], ref["dmul"], "dmul")
    X.assert_exact(o["ws"][:, :64], ref["dz2"], "workspace dz2")
    X.assert_exact(o["ws"][:, 64:64 + R], ref["dz1"], "workspace dz1")
    for k in ("dw1", "db1", "dw2", "db2"):
        X.assert_exact(o[k], ref[k], k)
    q = ca_bwd_run(D, params=False)
    for k in ("shift", "dmul"):
        if o[k] is not None:
            assert torch.equal(q[k], o[k]), k
    assert torch.equal(q["ws"][:, :64 + R], o["ws"][:, :64 + R])
    pb = dict(dz=q["ws"], hid=D.d["hid"], s=D.d["s"], dw1=nan(R, 64), db1=nan(R), dw2=nan(64, R), db2=nan(64))
    hip.check(params_batch([pb], B, R), "sisr_ca_gate_bwd_params_batch")
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.equal(pb[k], o[k]), f"{k}: deferred + params_batch differs from the in-kernel form"


def test_ca_gate_counter_resets_between_launches():
    """two back-to-back in-kernel backward launches with different B on the same gate counter: both right (the last block
    returns the device-scope counter to zero; a stale count would elect no block, or the wrong one, in the second launch)"""
    counter = hip.gate_counter(torch.device(DEV))
    Ds = [CaData(33, 4, 9, True, seed=900), CaData(40, 8, 2, False, seed=910), CaData(17, 3, 33, False, seed=920)]
    outs = [ca_bwd_run(D, counter=counter) for D in Ds]
    for D, o in zip(Ds, outs):
        ref = ca_bwd_exact_ref(D)
        for k in ("shift", "dw1", "db1", "dw2", "db2"):
            X.assert_exact(o[k], ref[k], f"B={D.B} {k}")
    torch.cuda.synchronize()
    assert int(hip._counters[torch.device(DEV).index][0]) == 0, "the gate counter was not returned to zero"


@pytest.mark.parametrize("njobs", [1, 2, 32])
def test_ca_params_batch_on_synthetic_rows(njobs):
    """sisr_ca_gate_bwd_params_batch fed synthetic dyadic [B][80] dz rows (dz2 | dz1), hid, s: every job exact"""
    B, R = 9, 5
    jobs, refs = [], []
    for k in range(njobs):
        dz = X.ints((B, 80), 1000 + k, -2, 2) / 16
        hid, s = X.ints((B, R), 1100 + k, 0, 2) / 2, X.ints((B, 64), 1200 + k) / 4
        dz2, dz1 = dd(dz[:, :64]), dd(dz[:, 64:64 + R])
        refs.append(dict(dw2=dz2.T @ dd(hid), dw1=dz1.T @ dd(s), db2=dz2.sum(0), db1=dz1.sum(0)))
        jobs.append(dict(dz=dev(dz), hid=dev(hid), s=dev(s), dw1=nan(R, 64), db1=nan(R), dw2=nan(64, R), db2=nan(64)))
    hip.check(params_batch(jobs, B, R), "sisr_ca_gate_bwd_params_batch")
    for j, r in zip(jobs, refs):
        for k in ("dw1", "db1", "dw2", "db2"):
            X.assert_exact(j[k], r[k], k)


def test_ca_gate_refusals():
    """R <= 16 (CA_WS_ROW = 80 = 64 + 16): 17 refused by the forward, backward and the batch; at most CA_PB = 32 jobs"""
    D = CaData(4, 16, 2, False, seed=5)
    z = nan(2, 80)
    L = lib()
    assert L.sisr_ca_gate_bwd_params_batch_max() == 32
    assert L.sisr_ca_gate_fwd(P(D.d["part"]), 4, 2, 1.0, P(z), P(z), P(z), P(z), 64, 17, None, P(z), P(z), P(z), P(z), S()) \
        == ERR_UNSUPPORTED
    assert L.sisr_ca_gate_bwd(P(D.d["part"]), 4, 2, 1.0, P(z), P(z), 64, 17, P(z), P(z), P(z), None, P(z), None, None, None,
                              None, None, P(z), None, S()) == ERR_UNSUPPORTED
    job = dict(dz=z, hid=z, s=z, dw1=z, db1=z, dw2=z, db2=z)
    assert params_batch([job], 2, 17) == ERR_ARG
    assert params_batch([job] * 33, 2, 4) == ERR_ARG
    assert L.sisr_ca_gate_fwd(P(D.d["part"]), 4, 2, 1.0, P(z), P(z), P(z), P(z), 128, 4, None, P(z), P(z), P(z), P(z), S()) \
        == ERR_UNSUPPORTED


def test_ca_gate_detectors():
    D = CaData(257, 5, 9, True, seed=77)
    ref = ca_fwd_exact_ref(D)
    # exact tier: one partial moved by 1 (row 256: the single row behind the unrolled rounds) -> s[b, c] and the hid it feeds
    pert = D.part.clone()
    pert[3, 256, 10] += 1
    rp = ca_fwd_exact_ref(D, pert)
    out = ca_fwd_run(D, part=dev(pert))
    for k in ("s", "hid"):
        expect_detected(X.mismatch(out[k], ref[k]), (rp[k] != ref[k]).cpu(), f"CA forward {k}")
    # bounded tier: b2[c] moved by 1/8 -> ca[:, c] outside the bound
    b2 = D.b2.clone()
    b2[7] += 0.125
    out = ca_fwd_run(D, w=(D.d["w1"], D.d["b1"], D.d["w2"], dev(b2)))
    ok = G.bound_ok(out["ca"], ref["ca"], ref["ca"], C_SIG).cpu()
    assert not bool(ok[:, 7].any()) and bool(ok[:, :7].all())
    # backward, exact: one dg partial moved -> shift[b] where the W1^T W2^T chain reaches, workspace row b, every dw / db
    pert = D.dgpart.clone()
    pert[4, 100, 3] += 1
    rb, rp = ca_bwd_exact_ref(D), ca_bwd_exact_ref(D, pert)
    o = ca_bwd_run(D, dgpart=dev(pert))
    for k in ("shift", "dmul", "dw1", "db1", "dw2", "db2"):
        expect_detected(X.mismatch(o[k], rb[k]), (rp[k] != rb[k]).cpu(), f"CA backward {k}")


def test_ca_gate_chain_bounded():
    """the kernels' own forward outputs fed to the backward (the backward through the sigmoid), against float64"""
    D = CaData(64, 4, 8, True, seed=31)
    ref = ca_fwd_exact_ref(D)
    out = ca_fwd_run(D)
    dgpart = sparse_ints((8, 64, 64), 32, 8, 64)
    dg = dd(dgpart).sum(1)
    B, R = 8, 4
    o = dict(shift=nan(B, 64), dmul=nan(B, 64), ws=nan(B, 80), dw1=nan(R, 64), db1=nan(R), dw2=nan(64, R), db2=nan(64))
    dgp = dev(dgpart)  # named: a temporary of the call expression could share its block with another
    hip.check(lib().sisr_ca_gate_bwd(P(dgp), 64, B, INV_HW, P(D.d["w1"]), P(D.d["w2"]), 64, R, P(out["s"]),
                                     P(out["hid"]), P(out["ca"]), P(D.d["mul"]), P(o["shift"]), P(o["dmul"]), P(o["dw1"]),
                                     P(o["db1"]), P(o["dw2"]), P(o["db2"]), P(o["ws"]), hip.gate_counter(torch.device(DEV)),
                                     S()), "sisr_ca_gate_bwd")
    args = (dg, ref["ca"], ref["hid"], ref["s"], dd(D.w1), dd(D.w2), dd(D.mul), INV_HW)
    r, m = G.ca_bwd_ref(*args), G.ca_bwd_ref(*args, A=True)
    for k in ("shift", "dmul", "dw1", "db1", "dw2", "db2"):
        G.assert_bounded(o[k], r[k], m[k], C_CHAIN, f"CA chain {k}")


# ============================================================================ 2. pixel sums
# (hw, C, B, with t).  sisr_gate_dg_parts: parts = ceil(hw / 512) capped at 128 -> 512 | 513 (1 | 2 partials),
# 65536 | 65537 (128 partials of 512 | the cap: 513 pixels each), 200000 (1563 each); each block walks its slice in rows of
# 16 pixels (hw 15 | 16 | 17); blockIdx.z = 64-channel chunk (C 64 .. 4096 = 64 chunks; 96 and 4160 refused).
DG_CASES = [(1, 64, 2, True), (15, 128, 3, False), (16, 192, 1, True), (17, 4096, 1, True), (511, 64, 2, False),
            (512, 128, 1, True), (513, 4096, 1, False), (1025, 192, 2, True), (65536, 64, 1, True), (65537, 128, 1, False),
            (200000, 64, 1, True)]


def dg_run(dy, t, B, hw, C):
    parts = lib().sisr_gate_dg_parts(hw)
    part = nan(B, parts, C)
    hip.check(lib().sisr_gate_dg_partial(P(dy), P(t), P(part), B, hw, C, S()), "sisr_gate_dg_partial")
    return part, parts


@pytest.mark.parametrize("hw,C,B,with_t", DG_CASES)
def test_gate_dg_partial(hw, C, B, with_t):
    dy = X.ints((B, hw, C), hw + C)
    t = X.ints((B, hw, C), hw + C + 1) if with_t else None
    part, parts = dg_run(dev(dy), dev(t) if with_t else None, B, hw, C)
    assert parts == G.dg_parts(hw)
    X.assert_budget(4.0 * -(-hw // parts), 1.0, "dg partial")
    X.assert_exact(part, G.dg_partial_ref(dd(dy), dd(t) if with_t else None, parts), "dg partials")


def test_gate_dg_partial_refusals_and_detector():
    L = lib()
    a = nan(4160 * 4)
    assert L.sisr_gate_dg_partial(P(a), None, P(a), 1, 4, 96, S()) == ERR_UNSUPPORTED
    assert L.sisr_gate_dg_partial(P(a), None, P(a), 1, 2, 4160, S()) == ERR_UNSUPPORTED
    assert L.sisr_gate_dg_partial(P(a[1:]), None, P(a), 1, 2, 64, S()) == ERR_ALIGN
    B, hw, C = 2, 1025, 128
    dy, t = X.ints((B, hw, C), 5), X.ints((B, hw, C), 6)
    t[1, 700, 70] = 0
    ref = G.dg_partial_ref(dd(dy), dd(t), G.dg_parts(hw))
    dy[1, 700, 70], t[1, 700, 70] = 2, 1  # pixel 700 is in partial 700 // 342 = 2 (3 partials of ceil(1025 / 3) pixels)
    part, _ = dg_run(dev(dy), dev(t), B, hw, C)
    want = torch.zeros(ref.shape, dtype=torch.bool)
    want[1, 2, 70] = True
    expect_detected(X.mismatch(part, ref).cpu(), want, "dg partial")


def sp_run(part, parts, B, C, scale, out=None):
    out = nan(B * C) if out is None else out
    hip.check(lib().sisr_sum_partials(P(part), parts, B, C, scale, P(out), S()), "sisr_sum_partials")
    return out


# (parts, B, C, scale, offset).  sum_partials takes the c4 kernel iff C % 4 == 0, both pointers 16-byte aligned and
# B <= 65535 (its grid's y dimension), the generic kernel otherwise: C 4 / 60 / 64 / 68 / 4096 (c4) | 130 (generic); a
# 1-float offset (generic); B 65535 (c4) | 65536 (generic).  scale 1/3 is rounded: one fp32 multiply of the exact sum.
SP_CASES = [(3, 2, 4, 1.0, 0), (17, 3, 60, 1.0 / 16, 0), (128, 2, 64, 1.0 / 3, 0), (5, 1, 68, 0.5, 0), (1, 2, 130, 1.0 / 3, 0),
            (33, 1, 4096, 1.0 / 7, 0), (9, 2, 64, 1.0 / 3, 1), (16, 3, 68, 1.0, 1), (3, 65535, 4, 1.0 / 3, 0),
            (3, 65536, 4, 1.0 / 3, 0)]


@pytest.mark.parametrize("parts,B,C,scale,offset", SP_CASES)
def test_sum_partials(parts, B, C, scale, offset):
    part = X.ints((B, parts, C), parts * 3 + C)
    buf = torch.full((B * parts * C + 4,), NAN, device=DEV)
    buf[offset:offset + part.numel()] = dev(part).view(-1)
    out = torch.full((B * C + 4,), NAN, device=DEV)
    sp_run(buf[offset:], parts, B, C, scale, out[offset:])
    exact = dd(part).sum(1)
    X.assert_budget(dd(part).abs().sum(1), 1.0, "sum of partials")
    X.assert_exact(out[offset:offset + B * C].view(B, C), G.sum_partials_fp32(exact, scale), "sum_partials")


def test_sum_partials_detector_and_global_avg_pool():
    B, parts, C = 3, 40, 68
    part = X.ints((B, parts, C), 8)
    ref = G.sum_partials_fp32(dd(part).sum(1), 0.25)
    for off in (0, 1):  # c4 and generic kernel
        pert = part.clone()
        pert[2, 39, 67] += 1
        buf = torch.full((pert.numel() + 4,), NAN, device=DEV)
        buf[off:off + pert.numel()] = dev(pert).view(-1)
        out = sp_run(buf[off:], parts, B, C, 0.25).view(B, C)
        want = torch.zeros(B, C, dtype=torch.bool)
        want[2, 67] = True
        expect_detected(X.mismatch(out, ref).cpu(), want, f"sum_partials (offset {off})")
    # ops.global_avg_pool: gate_dg_partial (t = NULL) + sum_partials with scale 1 / (H W)
    x = X.ints((2, 128, 3, 5), 9)
    got = ops.global_avg_pool(dev(x).contiguous(memory_format=torch.channels_last))
    X.assert_exact(got.view(2, 128), G.sum_partials_fp32(dd(x).sum(dim=(2, 3)), 1.0 / 15), "global_avg_pool")


# ============================================================================ 3. gated residual
def res_run(t, g, sh, x, B, hw, C):
    y = nan(B * hw * C)
    rc = lib().sisr_gate_residual_fwd(P(t), P(g), P(sh), P(x), P(y), B, hw, C, S())
    hip.check(rc, "sisr_gate_residual_fwd")
    return y.view(B, hw, C)


COMBOS = [(g, s, x) for g in (0, 1) for s in (0, 1) for x in (0, 1)]


@pytest.mark.parametrize("C", [4, 64, 128, 260])
@pytest.mark.parametrize("has_g,has_s,has_x", COMBOS)
def test_gate_residual_exact(C, has_g, has_s, has_x):
    B, hw = 3, 37
    t, x = X.ints((B, hw, C), C), X.ints((B, hw, C), C + 1)
    g, sh = X.scales((B, C), C + 2), X.shifts((B, C), C + 3)
    args = [t, g if has_g else None, sh if has_s else None, x if has_x else None]
    y = res_run(*[dev(a) if a is not None else None for a in args], B, hw, C)
    X.assert_exact(y, G.residual_ref(*[dd(a) if a is not None else None for a in args]), "gated residual")


@pytest.mark.parametrize("has_g,has_s,has_x", COMBOS)
def test_gate_residual_rounding(has_g, has_s, has_x):
    """random fp32 data: the gated skip (g, x, no shift) is fl(fl(t * g) + x) bit for bit (sisr_mul_add4: contraction off);
    the other forms may be contracted, so each rounding is bounded by half an ulp of its running magnitude"""
    B, hw, C = 2, 50, 64
    gen = torch.Generator().manual_seed(3)
    t, x = torch.randn(B, hw, C, generator=gen), torch.randn(B, hw, C, generator=gen)
    g, sh = torch.rand(B, C, generator=gen) + 0.5, torch.randn(B, C, generator=gen)
    args = [t, g if has_g else None, sh if has_s else None, x if has_x else None]
    y = res_run(*[dev(a) if a is not None else None for a in args], B, hw, C)
    if has_g and has_x and not has_s:
        assert torch.equal(y.cpu(), (t * g[:, None]) + x), "gated skip is not fl(fl(t * g) + x)"
    nops = has_g + has_s + has_x
    dargs = [dd(a) if a is not None else None for a in args]
    G.assert_bounded(y, G.residual_ref(*dargs), G.residual_ref(*dargs, A=True), nops * (1 + 2 ** -20), "residual")


def test_gate_residual_grid_cap_refusals_detector():
    """at most 2048 blocks of 256 float4: 2^19 float4 (hw 32768 at C 64) is one pass, hw 32769 needs the grid-stride loop"""
    C = 64
    for hw in (32768, 32769):
        t, x, g, sh = X.ints((1, hw, C), 1), X.ints((1, hw, C), 2), X.scales((1, C), 3), X.shifts((1, C), 4)
        y = res_run(dev(t), dev(g), dev(sh), dev(x), 1, hw, C)
        X.assert_exact(y, G.residual_ref(dd(t), dd(g), dd(sh), dd(x)), f"gated residual hw={hw}")
    L = lib()
    a = nan(1024)
    assert L.sisr_gate_residual_fwd(P(a), None, None, None, P(a), 1, 4, 6, S()) == ERR_ARG
    assert L.sisr_gate_residual_fwd(P(a[1:]), None, None, None, P(a), 1, 4, 64, S()) == ERR_ALIGN
    assert L.sisr_gate_residual_fwd(P(a), P(a[2:]), None, None, P(a), 1, 4, 64, S()) == ERR_ALIGN
    t, x, g = X.ints((2, 40, 64), 5), X.ints((2, 40, 64), 6), X.scales((2, 64), 7)
    ref = G.residual_ref(dd(t), dd(g), None, dd(x))
    tp = t.clone()
    tp[1, 33, 9] += 1
    y = res_run(dev(tp), dev(g), None, dev(x), 2, 40, 64)
    want = torch.zeros(2, 40, 64, dtype=torch.bool)
    want[1, 33, 9] = True
    expect_detected(X.mismatch(y, ref).cpu(), want, "gated residual")
    # and one pass through ops.gate_mul (the same launch, NCHW channels-last views)
    tc = dev(t.view(2, 5, 8, 64).permute(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last)
    xc = dev(x.view(2, 5, 8, 64).permute(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last)
    yo = ops.gate_mul(tc, dev(g).view(2, 64, 1, 1), xc)
    X.assert_exact(yo.permute(0, 2, 3, 1).reshape(2, 40, 64), ref, "ops.gate_mul")


# ============================================================================ 4. meta gates (ParaCALayer)
class MetaData:
    def __init__(self, B, M, Hd, C, relu, seed):
        self.B, self.M, self.Hd, self.C, self.relu = B, M, Hd, C, relu
        self.md = X.ints((B, M), seed, -1, 1)
        self.v1, self.c1 = X.weights((Hd, M), seed + 1, kmax=2), X.biases(Hd, seed + 2) / 2
        self.v2 = X.ints((C, Hd), seed + 3, -1, 1, zeros=max(0.5, 1 - 16 / Hd)) / 8
        self.c2 = X.biases(C, seed + 4)
        # backward: dyadic saved m in {1/4, 1/2, 3/4} and hid (>= 0 with zeros when relu)
        self.dm = X.ints((B, C), seed + 5, -1, 1)
        self.m = X.ints((B, C), seed + 6, 1, 3) / 4
        self.hid = X.ints((B, Hd), seed + 7, 0 if relu else -2, 2, zeros=0.3) / 2
        self.bv1, self.bv2 = X.ints((Hd, M), seed + 8, -1, 1) / 8, X.ints((C, Hd), seed + 9, -1, 1) / 8
        self.d = {k: dev(v) for k, v in vars(self).items() if torch.is_tensor(v)}


def meta_fwd_run(D, c2=None):
    hid, m = nan(D.B, D.Hd), nan(D.B, D.C)
    d = D.d
    hip.check(lib().sisr_meta_gate_fwd(P(d["md"]), D.B, D.M, D.Hd, D.C, P(d["v1"]), P(d["c1"]), P(d["v2"]),
                                       P(d["c2"] if c2 is None else c2), int(D.relu), P(hid), P(m), S()), "sisr_meta_gate_fwd")
    return hid, m


def meta_bwd_run(D, with_dmd, dm=None, m=None, hid=None, v1=None, v2=None):
    B, M, Hd, C = D.B, D.M, D.Hd, D.C
    o = dict(dv1=nan(Hd, M), dc1=nan(Hd), dv2=nan(C, Hd), dc2=nan(C), dmd=nan(B, M) if with_dmd else None,
             ws=nan(B * (Hd + C)))
    d = D.d
    rc = lib().sisr_meta_gate_bwd(P(d["dm"] if dm is None else dm), P(d["m"] if m is None else m),
                                  P(d["hid"] if hid is None else hid), P(d["md"]), B, M, Hd, C,
                                  P(d["bv1"] if v1 is None else v1), P(d["bv2"] if v2 is None else v2), int(D.relu),
                                  P(o["dv1"]), P(o["dc1"]), P(o["dv2"]), P(o["dc2"]), P(o["dmd"]), P(o["ws"]), S())
    hip.check(rc, "sisr_meta_gate_bwd")
    return o


# (B, M, Hd, C, relu).  Forward: hidden units j = tid, tid + 256 (Hd 255 | 256 | 257), channels likewise (C 300).
META_FWD = [(1, 1, 1, 64, True), (32, 10, 16, 128, False), (33, 11, 255, 300, True), (1, 20, 256, 64, False),
            (32, 33, 257, 128, True), (1, 10, 257, 300, False), (33, 1, 16, 300, True)]


@pytest.mark.parametrize("B,M,Hd,C,relu", META_FWD)
def test_meta_gate_forward(B, M, Hd, C, relu):
    D = MetaData(B, M, Hd, C, relu, seed=B + M * 3 + Hd * 5 + C)
    ref = G.meta_fwd_ref(dd(D.md), dd(D.v1), dd(D.c1), dd(D.v2), dd(D.c2), relu)
    mag = G.meta_fwd_mag(dd(D.md), dd(D.v1), dd(D.c1), dd(D.v2), dd(D.c2))
    X.assert_budget(mag["pre"], min(X.granule(dd(D.v1)), X.granule(dd(D.c1))), "meta pre")
    X.assert_budget(mag["z"], min(X.granule(ref["hid"]) * X.granule(dd(D.v2)), X.granule(dd(D.c2))), "meta z")
    hid, m = meta_fwd_run(D)
    X.assert_exact(hid, ref["hid"], "meta hid")
    G.assert_bounded(m, ref["m"], ref["m"], C_SIG, "meta m")


# (B, M, Hd, C, relu, dmd).  Backward: dz2 over c = tid, tid + 256 (C 300); dz1 over j likewise (Hd 257 -- only small C
# fits the LDS rule then); dmd over k < M.  LDS rule: (Hd + C + C*Hd + Hd*M) * 4 <= 60000: (48, 100, 100) is exactly
# 60000 bytes and accepted; one step past (M 49 or Hd 101) is refused (test below).
META_BWD = [(1, 1, 1, 64, True, True), (32, 10, 16, 128, False, False), (33, 11, 16, 300, True, True),
            (1, 20, 40, 64, True, False), (32, 33, 100, 64, False, True), (33, 1, 257, 4, True, True),
            (33, 48, 100, 100, True, True)]


@pytest.mark.parametrize("B,M,Hd,C,relu,with_dmd", META_BWD)
def test_meta_gate_backward(B, M, Hd, C, relu, with_dmd):
    D = MetaData(B, M, Hd, C, relu, seed=7 + B + M * 3 + Hd * 5 + C)
    ref = G.meta_bwd_ref(dd(D.dm), dd(D.m), dd(D.hid), dd(D.md), dd(D.bv1), dd(D.bv2), relu)
    val_budget(dd(D.dm) * dd(D.m) * (1 - dd(D.m)), "meta dz2")
    mm_budget(ref["dz2"], dd(D.bv2), "meta dh")
    mm_budget(ref["dz1"], dd(D.bv1), "meta dmd")
    mm_budget(ref["dz2"].T, dd(D.hid), "meta dv2")
    mm_budget(ref["dz1"].T, dd(D.md), "meta dv1")
    o = meta_bwd_run(D, with_dmd)
    for k in ("dv1", "dc1", "dv2", "dc2") + (("dmd",) if with_dmd else ()):
        X.assert_exact(o[k], ref[k], f"meta {k}")
    X.assert_exact(o["ws"][:B * C].view(B, C), ref["dz2"], "meta workspace dz2")
    X.assert_exact(o["ws"][B * C:].view(B, Hd), ref["dz1"], "meta workspace dz1")


@pytest.mark.parametrize("relu", [True, False])
def test_meta_gate_chain_relu_tie(relu):
    """kernel forward -> kernel backward, bounded against float64; with relu, hidden pre-activations exactly 0 in the data
    get dz1 = 0 (PyTorch's ReLU' at 0)"""
    D = MetaData(9, 10, 32, 64, relu, seed=400)
    ref = G.meta_fwd_ref(dd(D.md), dd(D.v1), dd(D.c1), dd(D.v2), dd(D.c2), relu)
    hid, m = meta_fwd_run(D)
    o = meta_bwd_run(D, True, m=m, hid=hid, v1=D.d["v1"], v2=D.d["v2"])
    args = (dd(D.dm), ref["m"], ref["hid"], dd(D.md), dd(D.v1), dd(D.v2), relu)
    r, mg = G.meta_bwd_ref(*args), G.meta_bwd_ref(*args, A=True)
    for k in ("dv1", "dc1", "dv2", "dc2", "dmd"):
        G.assert_bounded(o[k], r[k], mg[k], C_CHAIN, f"meta chain {k}")
    if relu:
        tie = (ref["pre"] == 0).cpu()
        assert bool(tie.any()), "no hidden pre-activation is exactly 0 (test bug)"
        assert bool((o["ws"][9 * 64:].view(9, 32).cpu()[tie] == 0).all())


def test_meta_gate_refusals_and_detectors():
    L = lib()
    a = nan(70000)
    for M, Hd, C, ok in ((48, 100, 100, True), (49, 100, 100, False), (48, 101, 100, False)):
        assert (Hd + C + C * Hd + Hd * M) * 4 == 60000 if ok else (Hd + C + C * Hd + Hd * M) * 4 > 60000
        rc = L.sisr_meta_gate_bwd(P(a), P(a), P(a), P(a), 1, M, Hd, C, P(a), P(a), 1, P(a), P(a), P(a), P(a), None, P(a), S())
        assert rc == (0 if ok else ERR_UNSUPPORTED), (M, Hd, C, rc)
    assert L.sisr_meta_gate_fwd(P(a), 1, 1, 4097, 4, P(a), P(a), P(a), P(a), 1, P(a), P(a), S()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    D = MetaData(5, 10, 16, 64, True, seed=500)
    ref = G.meta_fwd_ref(dd(D.md), dd(D.v1), dd(D.c1), dd(D.v2), dd(D.c2), True)
    c2 = D.c2.clone()
    c2[11] += 0.125
    _, m = meta_fwd_run(D, c2=dev(c2))
    ok = G.bound_ok(m, ref["m"], ref["m"], C_SIG).cpu()
    assert not bool(ok[:, 11].any()) and bool(ok[:, :11].all()), "meta forward detector"
    rb = G.meta_bwd_ref(dd(D.dm), dd(D.m), dd(D.hid), dd(D.md), dd(D.bv1), dd(D.bv2), True)
    dm = D.dm.clone()
    dm[2, 40] += 1
    rp = G.meta_bwd_ref(dd(dm), dd(D.m), dd(D.hid), dd(D.md), dd(D.bv1), dd(D.bv2), True)
    o = meta_bwd_run(D, True, dm=dev(dm))
    for k in ("dv1", "dc1", "dv2", "dc2", "dmd"):
        expect_detected(X.mismatch(o[k], rb[k]), (rp[k] != rb[k]).cpu(), f"meta backward {k}")


@pytest.mark.parametrize("L", [1, 3, 200])
def test_meta_gate_many_equals_single_layers(L):
    """ops.meta_gate_many: every layer bitwise equal to the single-layer launches on that layer's parameters; the scatter
    backward (GRAD_SINK set, as FlatAdam sets it) bitwise equal to the plain one"""
    B, M, Hd, C, relu = 4, 10, 32, 64, True
    md = dev(X.ints((B, M), 1, -1, 1))
    layers = []
    for l in range(L):
        D = MetaData(B, M, Hd, C, relu, seed=600 + 11 * l)
        layers.append(tuple(D.d[k].clone().requires_grad_(True) for k in ("v1", "c1", "v2", "c2")))
    dm = dev(X.ints((L, B, C), 2, -1, 1))
    ms = ops.meta_gate_many(md, layers, relu)
    torch.autograd.backward(list(ms), list(dm.unbind(0)))
    plain = [[p.grad.clone() for p in lay] for lay in layers]
    for l in (0, L // 2, L - 1):
        v1, c1, v2, c2 = (p.detach() for p in layers[l])
        hid, m = nan(B, Hd), nan(B, C)
        hip.check(lib().sisr_meta_gate_fwd(P(md), B, M, Hd, C, P(v1), P(c1), P(v2), P(c2), 1, P(hid), P(m), S()), "fwd")
        assert torch.equal(ms[l], m), f"layer {l} gate"
        g = dict(dv1=nan(Hd, M), dc1=nan(Hd), dv2=nan(C, Hd), dc2=nan(C), ws=nan(B * (Hd + C)))
        dml = dm[l].contiguous()
        hip.check(lib().sisr_meta_gate_bwd(P(dml), P(m), P(hid), P(md), B, M, Hd, C, P(v1), P(v2), 1,
                                           P(g["dv1"]), P(g["dc1"]), P(g["dv2"]), P(g["dc2"]), None, P(g["ws"]), S()), "bwd")
        for k, want in zip(("dv1", "dc1", "dv2", "dc2"), plain[l]):
            assert torch.equal(g[k], want), f"layer {l} {k}"
    for lay in layers:
        for p in lay:
            p.grad = None
    sinks = {}
    try:
        for lay in layers:
            for p in lay:
                sinks[p.data_ptr()] = torch.full_like(p, NAN)
                ops.GRAD_SINK[p.data_ptr()] = sinks[p.data_ptr()]
        ms = ops.meta_gate_many(md, layers, relu)
        torch.autograd.backward(list(ms), list(dm.unbind(0)))
    finally:
        for k in sinks:
            ops.GRAD_SINK.pop(k, None)
    for lay, want in zip(layers, plain):
        for p, w in zip(lay, want):
            assert p.grad.data_ptr() == sinks[p.data_ptr()].data_ptr(), "scatter path not taken"
            assert torch.equal(p.grad, w), "scatter gradient differs from the plain one"


# ============================================================================ 5. gate MLP (QCALayer styles, wide CA gate)
def style_widths(style, C, M):
    if style == "extended_attention":
        return [(32, C + M), (16, 32 + M), (4, 16 + M), (C, 4)]
    if style == "mini_concat":
        return [(4, C), (C, 4 + M)]
    if style == "modulate":
        return [(4, C), (C, 4)]
    if style == "wide":
        return [(C // 16, C), (C, C // 16)]
    return [(4, C + M), (C, 4)]


def spec_of(style):
    return ([(0, 0, 1), (0, 0, 2)], 0) if style == "wide" else ops.QCA_STYLES[style]


class MlpData:
    def __init__(self, style, B, C, M, seed, with_mul, relu_md=False):
        self.style, self.B, self.C, self.M = style, B, C, M
        self.spec = spec_of(style)
        self.pool = X.ints((B, C), seed, -2, 2) / 2
        self.md = X.ints((B, M), seed + 1, -2, 2) if M else torch.zeros(B, 0)
        self.ws = [X.ints((n, i), seed + 2 + k, -1, 1, zeros=0.3) / 8 for k, (n, i) in enumerate(style_widths(style, C, M))]
        self.bs = [X.biases(n, seed + 10 + k) for k, (n, _) in enumerate(style_widths(style, C, M))]
        self.mul = X.scales((B, C), seed + 20) if with_mul else None
        # backward: dyadic saved activations (relu outputs >= 0 with zeros, linear outputs signed, sigmoid outputs k/4)
        acts = [self.pool]
        for k, (cat, relu_in, act) in enumerate(self.spec[0]):
            n = self.ws[k].shape[0]
            lo, den = (0, 2) if act == 1 else (-2, 2) if act == 0 else (1, 4)
            acts.append(X.ints((B, n), seed + 30 + k, lo, 3 if act == 2 else 2, zeros=0.3 if act != 2 else None) / den)
        self.acts = acts
        self.yfin = X.ints((B, C), seed + 40, 1, 3) / 4
        self.dy = X.ints((B, C), seed + 41, -1, 1)


def mlp_desc(D, ws, bs):
    d = hip.GateMlpDesc()
    prev = ws[0].shape[1] - (D.M if D.spec[0][0][0] else 0)
    for k, (cat, relu_in, act) in enumerate(D.spec[0]):
        d.w[k], d.b[k] = P(ws[k]), P(bs[k])
        d.nin[k], d.nout[k], d.cat[k], d.relu_in[k], d.act[k] = prev, ws[k].shape[0], cat, relu_in, act
        prev = ws[k].shape[0]
    d.L, d.M, d.C, d.final_mode = len(D.spec[0]), D.M, prev, D.spec[1]
    return d


def mlp_fwd_run(D, ws=None, bs=None):
    ws = ws or [dev(w) for w in D.ws]
    bs = bs or [dev(b) for b in D.bs]
    d = mlp_desc(D, ws, bs)
    aw = D.C + sum(w.shape[0] for w in ws)
    acts, yfin, y = nan(D.B, aw), nan(D.B, D.C), nan(D.B, D.C)
    # every operand named: temporaries of one call expression may be handed the same block by the caching allocator
    pool, md, mul = dev(D.pool), dev(D.md) if D.M else None, dev(D.mul) if D.mul is not None else None
    rc = lib().sisr_gate_mlp_fwd(P(pool), P(md), P(mul), D.B,
                                 ctypes.addressof(d), P(acts), P(yfin), P(y), S())
    hip.check(rc, "sisr_gate_mlp_fwd")
    return acts, yfin, y


def mlp_bwd_run(D, with_dmd, with_dmul, acts=None, yfin=None, dy=None):
    ws, bs = [dev(w) for w in D.ws], [dev(b) for b in D.bs]
    d = mlp_desc(D, ws, bs)
    B = D.B
    acts = acts if acts is not None else dev(torch.cat(D.acts, dim=1))
    yfin = yfin if yfin is not None else dev(D.yfin)
    o = dict(dpool=nan(B, D.C), dmd=nan(B, D.M) if with_dmd else None,
             dmul=nan(B, D.C) if with_dmul else None, ws=nan(B, sum(w.shape[0] for w in ws)),
             dws=[torch.full_like(w, NAN) for w in ws], dbs=[torch.full_like(b, NAN) for b in bs])
    PA = ctypes.c_void_p * hip.GM_MAXL
    dwa, dba = PA(*[P(t) for t in o["dws"]]), PA(*[P(t) for t in o["dbs"]])
    dy = dev(D.dy) if dy is None else dy
    md, mul = dev(D.md) if D.M else None, dev(D.mul) if D.mul is not None else None
    rc = lib().sisr_gate_mlp_bwd(P(dy), P(md), P(mul), B, ctypes.addressof(d), P(acts), P(yfin),
                                 P(o["ws"]), P(o["dpool"]), P(o["dmd"]), P(o["dmul"]), dwa, dba, S())
    hip.check(rc, "sisr_gate_mlp_bwd")
    return o


def mlp_bwd_budget(D, ref):
    acts = [dd(a) for a in D.acts]
    md = dd(D.md)
    for k, (cat, relu_in, act) in enumerate(D.spec[0]):
        dz = ref["dzs"][k]
        val_budget(dz, f"gate MLP dz{k}")
        mm_budget(dz, dd(D.ws[k]), f"gate MLP layer {k} input gradient")
        inp = torch.cat([acts[k], md], dim=1) if cat else acts[k]
        mm_budget(dz.T, inp, f"gate MLP dW{k}")


# (style, B, M, mul, dmd, dmul).  Layer widths of a style at C = 64 (modulate: M == C); the wide CA gate at C 128 / 256 /
# 512 (hidden C / 16, M = 1 unused); B 1 / 9 / 33.  The widest layer input GM_MAXW = 544 (512 + 32) is probed below.
MLP_CASES = [("modulate", 1, 64, True, True, True), ("modulate", 9, 64, False, False, False),
             ("max_concat", 9, 10, True, True, False), ("max_concat", 33, 1, False, True, False),
             ("softmax", 1, 32, False, True, False), ("softmax", 33, 10, True, False, True),
             ("mini_concat", 9, 10, False, True, False), ("mini_concat", 1, 1, True, True, True),
             ("extended_attention", 9, 10, True, True, True), ("extended_attention", 33, 32, False, True, False),
             ("wide", 9, 0, False, False, False), ("wide", 1, 0, True, False, True), ("wide", 33, 0, False, False, False)]
WIDE_C = {0: 128, 1: 256, 2: 512}


def mlp_case(i):
    style, B, M, mul, dmd, dmul = MLP_CASES[i]
    C = WIDE_C[sum(1 for c in MLP_CASES[:i] if c[0] == "wide")] if style == "wide" else 64
    return MlpData(style, B, C, M if style != "wide" else 0, seed=50 * i + 3, with_mul=mul), dmd, dmul


@pytest.mark.parametrize("i", range(len(MLP_CASES)), ids=[f"{c[0]}-B{c[1]}-M{c[2]}" for c in MLP_CASES])
def test_gate_mlp_forward(i):
    D, _, _ = mlp_case(i)
    ref = G.mlp_fwd_ref(dd(D.pool), dd(D.md), [dd(w) for w in D.ws], [dd(b) for b in D.bs], D.spec,
                        None if D.mul is None else dd(D.mul))
    mags = G.mlp_fwd_mag(dd(D.pool), dd(D.md), [dd(w) for w in D.ws], [dd(b) for b in D.bs], D.spec)
    acts, yfin, y = mlp_fwd_run(D)
    off = D.C
    L = len(D.spec[0])
    for k in range(L):
        n = D.ws[k].shape[0]
        if D.spec[0][k][2] != 2:
            inp = torch.cat([ref["acts"][k], dd(D.md)], 1) if D.spec[0][k][0] else ref["acts"][k]
            X.assert_budget(mags[k], min(X.granule(inp) * X.granule(dd(D.ws[k])), X.granule(dd(D.bs[k]))), f"layer {k}")
            X.assert_exact(acts[:, off:off + n], ref["acts"][k + 1], f"gate MLP layer {k} output")
        else:
            G.assert_bounded(acts[:, off:off + n], ref["acts"][k + 1], ref["acts"][k + 1], C_SIG, f"layer {k} sigmoid")
        off += n
    X.assert_exact(acts[:, :D.C], dd(D.pool), "acts: pooled input")
    c = C_SOFTMAX if D.spec[1] == 1 else C_SIG
    G.assert_bounded(yfin, ref["yfin"], ref["yfin"].abs(), c, "yfin")
    G.assert_bounded(y, ref["y"], ref["y"].abs(), c + (C_SIG if D.mul is not None else 0), "y")


@pytest.mark.parametrize("i", range(len(MLP_CASES)), ids=[f"{c[0]}-B{c[1]}-M{c[2]}" for c in MLP_CASES])
def test_gate_mlp_backward(i):
    D, with_dmd, with_dmul = mlp_case(i)
    with_dmd = with_dmd and D.M > 0
    with_dmul = with_dmul and D.mul is not None
    ref = G.mlp_bwd_ref(dd(D.dy), dd(D.md), None if D.mul is None else dd(D.mul), [dd(w) for w in D.ws], D.spec,
                        [dd(a) for a in D.acts], dd(D.yfin))
    mlp_bwd_budget(D, ref)
    o = mlp_bwd_run(D, with_dmd, with_dmul)
    X.assert_exact(o["dpool"], ref["dpool"], "d pool")
    if with_dmd:
        X.assert_exact(o["dmd"], ref["dmd"], "d metadata")
    if with_dmul:
        X.assert_exact(o["dmul"], ref["dmul"], "d mul")
    X.assert_exact(o["ws"], torch.cat(ref["dzs"], 1), "workspace dz")
    for k in range(len(D.ws)):
        X.assert_exact(o["dws"][k], ref["dws"][k], f"dW{k}")
        X.assert_exact(o["dbs"][k], ref["dbs"][k], f"db{k}")


def test_gate_mlp_mini_concat_masked_metadata_and_detectors():
    """mini_concat: ReLU(cat(., md)) -- metadata <= 0 gets exactly 0 gradient; detectors of both tiers"""
    D = MlpData("mini_concat", 4, 64, 6, seed=900, with_mul=False)
    D.md = torch.tensor([[-2.0, 0.0, 1.0, -1.0, 2.0, 0.0], [0.0, 1.0, -1.0, 0.0, 0.0, 2.0],
                         [1.0, 1.0, 1.0, -1.0, -1.0, 0.0], [-1.0, -2.0, 0.0, 2.0, 1.0, 1.0]])
    D.acts[1][1] = 0.5  # sample 1: every pre_concat output positive (its ReLU passes the gradient) ...
    D.ws[1][5] = 0.125  # ... and channel 5 reaches each of them: the detector's dy[1, 5] feeds d pool[1, :]
    ref = G.mlp_bwd_ref(dd(D.dy), dd(D.md), None, [dd(w) for w in D.ws], D.spec, [dd(a) for a in D.acts], dd(D.yfin))
    o = mlp_bwd_run(D, True, False)
    X.assert_exact(o["dmd"], ref["dmd"], "d metadata")
    assert bool((o["dmd"].cpu()[D.md <= 0] == 0).all()) and bool((o["dmd"].cpu()[D.md > 0] != 0).any())
    dy = D.dy.clone()
    dy[1, 5] += 1
    rp = G.mlp_bwd_ref(dd(dy), dd(D.md), None, [dd(w) for w in D.ws], D.spec, [dd(a) for a in D.acts], dd(D.yfin))
    o = mlp_bwd_run(D, True, False, dy=dev(dy))
    for k in ("dpool", "dmd"):
        expect_detected(X.mismatch(o[k], ref[k]), (rp[k] != ref[k]).cpu(), f"gate MLP backward {k}")
    expect_detected(X.mismatch(o["dws"][1], ref["dws"][1]), (rp["dws"][1] != ref["dws"][1]).cpu(), "gate MLP dW1")
    fr = G.mlp_fwd_ref(dd(D.pool), dd(D.md), [dd(w) for w in D.ws], [dd(b) for b in D.bs], D.spec)
    bs = [dev(b) for b in D.bs]
    bs[1][20] += 0.125
    _, yfin, _ = mlp_fwd_run(D, bs=bs)
    ok = G.bound_ok(yfin, fr["yfin"], fr["yfin"], C_SIG).cpu()
    assert not bool(ok[:, 20].any()) and bool(ok[:, :20].all()), "gate MLP forward detector"


def test_gate_mlp_refusals_and_widest_input():
    """GM_MAXW = 544: a 512 + 32 concatenated input accepted (and right), 512 + 33 refused; modulate needs M == C"""
    D = MlpData("max_concat", 2, 512, 32, seed=950, with_mul=False)
    D.ws[0] = X.ints((32, 544), 951, -1, 1, zeros=0.7) / 8
    D.ws[1] = X.ints((512, 32), 952, -1, 1, zeros=0.7) / 8
    D.bs = [X.biases(32, 953), X.biases(512, 954)]
    ref = G.mlp_fwd_ref(dd(D.pool), dd(D.md), [dd(w) for w in D.ws], [dd(b) for b in D.bs], D.spec)
    acts, yfin, _ = mlp_fwd_run(D)
    X.assert_exact(acts[:, 512:544], ref["acts"][1], "544-wide layer")
    G.assert_bounded(yfin, ref["yfin"], ref["yfin"], C_SIG, "544-wide yfin")
    D33 = MlpData("max_concat", 2, 512, 33, seed=960, with_mul=False)
    ws = [dev(X.ints((32, 545), 961) / 8), dev(X.ints((512, 32), 962) / 8)]
    d = mlp_desc(D33, ws, [dev(torch.zeros(32)), dev(torch.zeros(512))])
    a = nan(2, 2000)
    assert lib().sisr_gate_mlp_fwd(P(a), P(a), None, 2, ctypes.addressof(d), P(a), P(a), P(a), S()) == ERR_UNSUPPORTED
    Dm = MlpData("modulate", 2, 64, 10, seed=970, with_mul=False)
    d = mlp_desc(Dm, [dev(w) for w in Dm.ws], [dev(b) for b in Dm.bs])
    assert lib().sisr_gate_mlp_fwd(P(a), P(a), None, 2, ctypes.addressof(d), P(a), P(a), P(a), S()) == ERR_UNSUPPORTED


def test_gate_mlp_chain_through_ops_qca_gate():
    """ops.qca_gate (softmax style, with the meta gate folded in): forward and backward against float64, bounded"""
    D = MlpData("softmax", 9, 64, 10, seed=990, with_mul=True)
    convs = [types.SimpleNamespace(weight=dev(w).view(w.shape[0], w.shape[1], 1, 1).requires_grad_(True),
                                   bias=dev(b).requires_grad_(True)) for w, b in zip(D.ws, D.bs)]
    pool = dev(D.pool).view(9, 64, 1, 1).requires_grad_(True)
    md = dev(D.md).view(9, 10, 1, 1).requires_grad_(True)
    mul = dev(D.mul).requires_grad_(True)
    y = ops.qca_gate(pool, md, "softmax", convs, mul)
    fr = G.mlp_fwd_ref(dd(D.pool), dd(D.md), [dd(w) for w in D.ws], [dd(b) for b in D.bs], D.spec, dd(D.mul))
    G.assert_bounded(y.view(9, 64), fr["y"], fr["y"], C_SOFTMAX + C_SIG, "qca_gate forward")
    y.backward(dev(D.dy).view(9, 64, 1, 1))
    args = (dd(D.dy), dd(D.md), dd(D.mul), [dd(w) for w in D.ws], D.spec, fr["acts"], fr["yfin"])
    r, m = G.mlp_bwd_ref(*args), G.mlp_bwd_ref(*args, A=True)
    G.assert_bounded(pool.grad.view(9, 64), r["dpool"], m["dpool"], C_CHAIN, "qca_gate d pool")
    G.assert_bounded(md.grad.view(9, 10), r["dmd"], m["dmd"], C_CHAIN, "qca_gate d metadata")
    G.assert_bounded(mul.grad, r["dmul"], m["dmul"], C_CHAIN, "qca_gate d mul")
    for k, cv in enumerate(convs):
        G.assert_bounded(cv.weight.grad.view(r["dws"][k].shape), r["dws"][k], m["dws"][k], C_CHAIN, f"qca_gate dW{k}")
        G.assert_bounded(cv.bias.grad, r["dbs"][k], m["dbs"][k], C_CHAIN, f"qca_gate db{k}")


# ============================================================================ 6. pixel attention (64 -> 8 -> 1)
def pa_data(npix, seed):
    x = X.ints((npix, 64), seed, -1, 1, zeros=0.3)
    x[npix // 2] = 0  # this pixel's hidden pre-activations are b1: exactly 0 where b1 is
    w1, b1 = X.weights((8, 64), seed + 1, kmax=2), X.biases(8, seed + 2)
    b1[::2] = 0
    w2, b2 = X.weights((8,), seed + 3), X.biases(1, seed + 4)
    dy = X.ints((npix, 64), seed + 5, -1, 1)
    return x, w1, b1, w2, b2, dy


def pa_run(x, w1, b1, w2, b2, dy=None):
    npix = x.shape[0]
    if dy is None:
        y = nan(npix, 64)
        hip.check(lib().sisr_pa_fwd(P(x), P(w1), P(b1), P(w2), P(b2), P(y), npix, 64, 8, S()), "sisr_pa_fwd")
        return y
    o = dict(dx=nan(npix, 64), dw1=nan(8, 64), db1=nan(8), dw2=nan(8), db2=nan(1))
    ws = torch.empty(lib().sisr_pa_bwd_workspace_bytes(npix) // 4, device=DEV)
    hip.check(lib().sisr_pa_bwd(P(x), P(w1), P(b1), P(w2), P(b2), P(dy), P(o["dx"]), P(o["dw1"]), P(o["db1"]), P(o["dw2"]),
                                P(o["db2"]), P(ws), npix, 64, 8, S()), "sisr_pa_bwd")
    return o


# npix: 16 pixels per block and round (1 / 15 / 16 / 17), min(ceil(npix / 16), 1024) blocks: 16383 / 16384 fill the grid
# once, 16385 and 3 * 16384 + 5 take the grid-stride loop (the last round partly dead).
@pytest.mark.parametrize("npix", [1, 15, 16, 17, 16383, 16384, 16385, 3 * 16384 + 5])
def test_pa_forward_backward(npix):
    x, w1, b1, w2, b2, dy = pa_data(npix, seed=npix % 1000 + 3)
    D = [dev(t) for t in (x, w1, b1, w2, b2, dy)]
    ref = G.pa_fwd_ref(*[dd(t) for t in (x, w1, b1, w2, b2)])
    mag = G.pa_fwd_mag(*[dd(t) for t in (x, w1, b1, w2, b2)])
    X.assert_budget(mag["z"], X.granule(dd(w1)) * X.granule(dd(w2)) / 8, "PA z")
    assert bool((ref["pre"] == 0).any())
    y = pa_run(*D[:5])
    G.assert_bounded(y, ref["y"], ref["y"].abs(), C_SIG, "PA y")
    o = pa_run(*D)
    args = [dd(t) for t in (x, w1, b1, w2, b2, dy)]
    r, m = G.pa_bwd_ref(*args), G.pa_bwd_ref(*args, A=True)
    for k in ("dx", "dw1", "db1", "dw2", "db2"):
        G.assert_bounded(o[k], r[k], m[k], C_PA, f"PA {k}")


def test_pa_detector_and_ops_pa_layer():
    x, w1, b1, w2, b2, dy = pa_data(1000, seed=17)
    ref = G.pa_fwd_ref(*[dd(t) for t in (x, w1, b1, w2, b2)])
    w2p = w2.clone()
    w2p[3] += 0.125
    y = pa_run(dev(x), dev(w1), dev(b1), dev(w2p), dev(b2))
    assert not bool(G.bound_ok(y, ref["y"], ref["y"].abs(), C_SIG).all()), "PA forward detector"
    args = [dd(t) for t in (x, w1, b1, w2, b2, dy)]
    r, m = G.pa_bwd_ref(*args), G.pa_bwd_ref(*args, A=True)
    o = pa_run(dev(x), dev(w1), dev(b1), dev(w2p), dev(b2), dev(dy))
    for k in ("dx", "dw1", "db1"):
        assert not bool(G.bound_ok(o[k], r[k], m[k], C_PA).all()), f"PA backward detector {k}"
    # ops.pa_layer: B = 2, 20 x 25 pixels, channels-last maps
    xm = dev(x).view(2, 20, 25, 64).permute(0, 3, 1, 2).requires_grad_(True)
    params = [dev(w1).view(8, 64, 1, 1), dev(b1), dev(w2).view(1, 8, 1, 1), dev(b2)]
    params = [p.requires_grad_(True) for p in params]
    yo = ops.pa_layer(xm, *params)
    G.assert_bounded(yo.permute(0, 2, 3, 1).reshape(1000, 64), ref["y"], ref["y"].abs(), C_SIG, "ops.pa_layer")
    yo.backward(dev(dy).view(2, 20, 25, 64).permute(0, 3, 1, 2))
    G.assert_bounded(xm.grad.permute(0, 2, 3, 1).reshape(1000, 64), r["dx"], m["dx"], C_PA, "ops.pa_layer dx")
    for p, k in zip(params, ("dw1", "db1", "dw2", "db2")):
        G.assert_bounded(p.grad.view(r[k].shape), r[k], m[k], C_PA, f"ops.pa_layer {k}")


# ============================================================================ 7. L1 loss
def l1_run(a, b):
    loss, grad = nan(1), torch.full_like(a, NAN)
    ws = torch.empty(lib().sisr_l1_loss_workspace_bytes() // 4, device=DEV)
    hip.check(lib().sisr_l1_loss(P(a), P(b), a.numel(), P(loss), P(grad), P(ws), S()), "sisr_l1_loss")
    return loss, grad


def inv_n(n):
    """the kernel's 1 / n: 1.0f / (float)n, two roundings (n = 2^24 + 3 itself rounds to 2^24 + 4 in fp32)"""
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)


# n: min(ceil(n / 256), 512) blocks of 256 threads: 255 / 256 / 257 (one block | two), 131072 = 512 * 256 (every thread
# one element) | 131073 (the grid-stride loop), 2^24 + 3 (128 elements a thread).  Exact ties (a == b) everywhere.
@pytest.mark.parametrize("n", [1, 255, 256, 257, 131072, 131073, 2 ** 24 + 3])
def test_l1_loss(n):
    gen = torch.Generator().manual_seed(n % 9973)
    a = torch.randint(-2, 3, (n,), generator=gen).float()
    b = a + torch.randint(-1, 2, (n,), generator=gen).float() * (torch.rand(n, generator=gen) < 0.2).float()
    a[0], b[0] = 1.0, 1.0
    S_ = (dd(a) - dd(b)).abs().sum()
    X.assert_budget(S_, 1.0, "L1 sum")
    loss, grad = l1_run(dev(a), dev(b))
    inv = inv_n(n)
    X.assert_exact(loss, (S_.float().cpu() * inv).double().view(1), "L1 value: fl(S * inv_n)")
    d = dd(a) - dd(b)
    X.assert_exact(grad, torch.sign(d) * float(inv), "L1 gradient: sign * inv_n")
    v, g = G.l1_ref(dd(a), dd(b))
    G.assert_bounded(loss, v.view(1), v.view(1), C_L1 + 1, "L1 value against float64")
    G.assert_bounded(grad, g, g.abs(), C_L1, "L1 gradient against float64")
    assert bool((grad[d == 0] == 0).all())


def test_l1_detector_and_ops_l1_loss():
    n = 5000
    a, b = X.ints((n,), 1), X.ints((n,), 2)
    b[123] = a[123]
    v, g = G.l1_ref(dd(a), dd(b))
    ap = a.clone()
    ap[123] += 1
    loss, grad = l1_run(dev(ap), dev(b))
    want = torch.zeros(n, dtype=torch.bool)
    want[123] = True
    inv = float(inv_n(n))
    expect_detected(X.mismatch(grad, torch.sign(dd(a) - dd(b)) * inv).cpu(), want, "L1 gradient")
    assert not bool(G.bound_ok(loss, v.view(1), v.view(1), C_L1 + 1).all()), "L1 value detector"
    at = dev(a).view(2, 2500).requires_grad_(True)
    lo = ops.l1_loss(at, dev(b).view(2, 2500))
    lo.backward()
    G.assert_bounded(lo.view(1), v.view(1), v.view(1), C_L1 + 1, "ops.l1_loss")
    X.assert_exact(at.grad.view(-1), torch.sign(dd(a) - dd(b)) * inv, "ops.l1_loss gradient")


# ============================================================================ 8. ops.ca_layer (the CA block wrapper)
def test_ops_ca_layer_chain():
    """ops.ca_layer at C = 64: pixel sums + gate forward + gate multiply, and its backward, against float64 (bounded)"""
    B, R, H, W = 3, 4, 8, 4
    x = X.ints((B, 64, H, W), 1, -1, 1, zeros=0.3)
    w1, b1, w2, b2 = X.weights((R, 64), 2), X.biases(R, 3), X.weights((64, R), 4), X.biases(64, 5)
    dy = X.ints((B, 64, H, W), 6, -1, 1)
    xm = dev(x).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ps = [dev(w1).view(R, 64, 1, 1), dev(b1), dev(w2).view(64, R, 1, 1), dev(b2)]
    ps = [p.requires_grad_(True) for p in ps]
    y = ops.ca_layer(xm, *ps)
    s = dd(x).mean(dim=(2, 3))
    f = G.ca_fwd_ref(s, dd(w1), dd(b1), dd(w2), dd(b2))
    yr = dd(x) * f["ca"].view(B, 64, 1, 1)
    G.assert_bounded(y, yr, yr.abs(), C_SIG, "ops.ca_layer forward")
    y.backward(dev(dy).contiguous(memory_format=torch.channels_last))
    dg = (dd(dy) * dd(x)).sum(dim=(2, 3))
    args = (dg, f["ca"], f["hid"], s, dd(w1), dd(w2), None, 1.0 / (H * W))
    r, m = G.ca_bwd_ref(*args), G.ca_bwd_ref(*args, A=True)
    dxr = dd(dy) * f["ca"].view(B, 64, 1, 1) + r["shift"].view(B, 64, 1, 1)
    dxm = dd(dy).abs() * f["ca"].view(B, 64, 1, 1) + m["shift"].view(B, 64, 1, 1)
    G.assert_bounded(xm.grad, dxr, dxm, C_CHAIN, "ops.ca_layer dx")
    for p, k in zip(ps, ("dw1", "db1", "dw2", "db2")):
        G.assert_bounded(p.grad.view(r[k].shape), r[k], m[k], C_CHAIN, f"ops.ca_layer {k}")
