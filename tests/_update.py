"""Float64 references of the optional parts of the update step (helper module, not collected; torch only, no HIP import):
the global gradient norm and its clip coefficient, and the Adam pass with a device-side gradient scale, decoupled weight decay
and the exponential moving average of the weights (csrc/update.hip, optim.FlatAdam).

tests/test_update_cpu.py checks them against float64 torch.optim.AdamW, clip_grad_norm_ and swa_utils' EMA update;
tests/test_update_gpu.py compares the kernels with them.  As in tests/_glue.py, `A=True` evaluates the same computation on
absolute values with every subtraction turned into an addition: the magnitude each fp32 rounding of the kernel is relative
to, so a bound reads |got - ref| <= c * 2^-24 * mag.
"""
import torch

from _glue import _d, f32


def sumsq_ref(*gs):
    """sum of g^2 over all the given fp32 tensors, every product and sum in float64 (a Python float)"""
    return float(sum((_d(g) ** 2).sum() for g in gs))


def norm_ref(*gs):
    return float(torch.tensor(sumsq_ref(*gs), dtype=torch.float64).sqrt())


def clip_coef_ref(norm, max_norm, rounded=True):
    """min(1, max_norm / (norm + 1e-6)) in float64 on the float64 norm, then rounded once to fp32 (rounded=False: not at
    all).  The comparison is written so that a NaN stays one, as torch.clamp(max=1) keeps it."""
    c = float(max_norm) / (float(norm) + 1e-6)
    c = 1.0 if c > 1.0 else c
    return f32(c) if rounded else c


def update_ref(p, g, m, v, e, beta2, omb1, omb2, eps, step_size, bc2_sqrt, grad_scale, dev_scale=None, decay=1.0, omd=None,
               A=False):
    """the kernel's lines in float64 on the fp32 inputs and scalars as passed:
        gg = g grad_scale [dev_scale];  p0 = p decay;  m' = m + (gg - m) omb1;  v' = v beta2 + gg gg omb2;
        p' = p0 - step_size (m' / (sqrt(v') / bc2_sqrt + eps));  [e' = e + (p' - e) omd]
    (tests/_glue.py adam_ref's five lines, the decay multiply, the device scale and the average).  e / omd None: no average.
    A: |m| + (|gg| + |m|) omb1,  |p| decay + step_size (that / denominator)  and  |e| + (A(p') + |e|) omd."""
    p, g, m, v, e = map(_d, (p, g, m, v, e))
    gg = g * grad_scale
    if dev_scale is not None:
        gg = gg * dev_scale
    if A:
        p, gg, m = p.abs(), gg.abs(), m.abs()
        e = None if e is None else e.abs()
    p0 = p * decay
    m1 = m + (gg + m if A else gg - m) * omb1
    v1 = v * beta2 + gg * gg * omb2
    upd = step_size * (m1 / (v1.sqrt() / bc2_sqrt + eps))
    p1 = p0 + upd if A else p0 - upd
    out = dict(m=m1, v=v1, p=p1)
    if e is not None and omd is not None:
        out["e"] = e + (p1 + e if A else p1 - e) * omd
    return out


def ema_ref(p, e, omd, A=False):
    """the average-only line: e + (p - e) omd;  A: |e| + (|p| + |e|) omd"""
    p, e = _d(p), _d(e)
    if A:
        return e.abs() + (p.abs() + e.abs()) * omd
    return e + (p - e) * omd
