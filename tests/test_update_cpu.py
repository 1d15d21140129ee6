"""The update step's optional parts without a GPU: the float64 references of tests/_update.py against torch's own float64
statements (torch.optim.AdamW(foreach=False), clip_grad_norm_, swa_utils' EMA update), the handlers' argument checks and
the checkpoint schema of a handler that uses none of the options."""
import math

import pytest
import torch

import sisr_amd
from sisr_amd import handlers

import _glue as R
import _update as U

CPU = torch.device("cpu")


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def rel(got, want):
    want = want.detach()
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())


# ----------------------------------------------------------------------------- the references against torch
def test_update_reference_follows_torch_adamw_clip_and_ema_over_three_steps_with_a_skipped_parameter():
    """three parameters, three steps, parameter 1 without a gradient in step 2; clip_grad_norm_ on the float64 gradients
    (clipping in steps 1 and 2, a coefficient of 1 in step 3), AdamW's decoupled decay, and the EMA update of
    torch.optim.swa_utils after every step on every parameter: norm, coefficient, parameters, moments and averages <= 1e-12
    relative"""
    lr, b1, b2, eps, wd, max_norm, decay = 1e-3, 0.9, 0.999, 1e-8, 0.05, 0.5, 0.9
    ps = [torch.nn.Parameter(rnd(n, seed=10 + n)) for n in (7, 33, 5)]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    ema_fn = torch.optim.swa_utils.get_ema_multi_avg_fn(decay)
    avg = [p.detach().clone() for p in ps]
    mine = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), e=p.detach().clone(), t=0) for p in ps]
    coefs = []
    for step in range(3):
        for k, p in enumerate(ps):
            p.grad = None if (k == 1 and step == 1) else rnd(*p.shape, seed=100 * step + k, scale=1e-3 if step == 2 else 1.0)
        live = [k for k, p in enumerate(ps) if p.grad is not None]
        norm = U.norm_ref(*[ps[k].grad for k in live])
        coef = U.clip_coef_ref(norm, max_norm, rounded=False)
        grads = {k: ps[k].grad.clone() for k in live}
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(norm - float(total)) <= 1e-12 * float(total)
        coefs.append(coef)
        for k, s in enumerate(mine):
            if k not in live:
                s["e"] = U.ema_ref(s["p"], s["e"], 1 - decay)
                continue
            s["t"] += 1
            sc = R.adam_scalars(lr, b1, b2, eps, s["t"], rounded=False)
            kw = dict(dev_scale=coef, decay=1 - lr * wd, omd=1 - decay)
            out = U.update_ref(s["p"], grads[k], s["m"], s["v"], s["e"], **sc, **kw)
            mag = U.update_ref(s["p"], grads[k], s["m"], s["v"], s["e"], **sc, **kw, A=True)
            assert all(bool((mag[n] >= out[n].abs()).all()) for n in "mvpe")
            assert rel(grads[k] * coef, ps[k].grad) <= 1e-12
            s.update(out)
        opt.step()
        with torch.no_grad():
            ema_fn(avg, [p.detach() for p in ps], step + 1)
    assert coefs[0] < 1 and coefs[1] < 1 and coefs[2] == 1.0
    for k, p in enumerate(ps):
        st = opt.state[p]
        assert int(st["step"]) == mine[k]["t"] == (2 if k == 1 else 3)
        for got, want, what in ((mine[k]["p"], p, "p"), (mine[k]["m"], st["exp_avg"], "m"), (mine[k]["v"], st["exp_avg_sq"], "v"),
                                (mine[k]["e"], avg[k], "e")):
            assert rel(got, want) <= 1e-12, (k, what)


def test_clip_coefficient_reference():
    assert U.clip_coef_ref(2.0, 1.0, rounded=False) == 1.0 / (2.0 + 1e-6)
    assert U.clip_coef_ref(2.0, 1.0) == R.f32(1.0 / (2.0 + 1e-6))
    assert U.clip_coef_ref(0.5, 1.0) == 1.0 and U.clip_coef_ref(0.0, 0.1) == 1.0
    assert math.isnan(U.clip_coef_ref(float("nan"), 1.0)) and U.clip_coef_ref(float("inf"), 1.0) == 0.0
    g = [torch.tensor([3.0, 0.0, -4.0]), torch.tensor([12.0])]
    assert U.sumsq_ref(*g) == 169.0 and U.norm_ref(*g) == 13.0


def test_with_the_additions_off_the_reference_is_the_adam_reference():
    p, g, m, v = (rnd(19, seed=s).float() for s in (1, 2, 3, 4))
    v = v.abs()
    sc = R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, 5, grad_scale=0.37)
    a, b = U.update_ref(p, g, m, v, None, **sc), R.adam_ref(p, g, m, v, **sc)
    assert set(a) == set(b) and all(torch.equal(a[n], b[n]) for n in "mvp")


# ----------------------------------------------------------------------------- entry points
def test_norm_entry_points_size_their_workspace_and_refuse_bad_arguments_before_any_device_call():
    """one double per workgroup of a range: ceil(n / 4 / 256) of them, at least 1 and at most 1024 (the grid strides above
    1 048 576 floats).  Refusals happen on the host and launch nothing, so this runs without a GPU (the pointers are host
    stand-ins that must never be dereferenced)."""
    import ctypes as C
    L = sisr_amd.hip.lib()
    wsb = L.sisr_sumsq_workspace_bytes
    assert [wsb(n) for n in (0, -4, 1, 3, 1024, 1027, 1028, 2048, 2052)] == [0, 0, 8, 8, 8, 8, 16, 16, 24]
    cap = 1024 * 256 * 4
    assert wsb(cap - 4) == wsb(cap) == wsb(cap + 4) == wsb(100 * cap) == 1024 * 8 and wsb(cap - 1024) == 1023 * 8
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    a += (-a) % 16
    ERR_ARG, ERR_ALIGN = -1, -2
    assert L.sisr_sumsq_partial(None, 8, a, None) == ERR_ARG and L.sisr_sumsq_partial(a, 8, None, None) == ERR_ARG
    assert L.sisr_sumsq_partial(a, 0, a, None) == ERR_ARG and L.sisr_sumsq_partial(a, -8, a, None) == ERR_ARG
    assert L.sisr_sumsq_partial(a + 4, 8, a, None) == ERR_ALIGN and L.sisr_sumsq_partial(a, 8, a + 4, None) == ERR_ALIGN
    f = L.sisr_clip_coef
    for k in (0, 3, 4, 5):
        args = [a, 4, 1.0, a, a, a, None]
        args[k] = None
        assert f(*args) == ERR_ARG, k
    for bad in (0.0, -1.0, float("nan")):
        assert f(a, 4, bad, a, a, a, None) == ERR_ARG, bad
    assert f(a, 0, 1.0, a, a, a, None) == ERR_ARG
    assert f(a + 4, 4, 1.0, a, a, a, None) == ERR_ALIGN and f(a, 4, 1.0, a + 4, a, a, None) == ERR_ALIGN


# ----------------------------------------------------------------------------- handler arguments
def _edsr(tmp_path, **kw):
    return handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), num_blocks=1, **kw)


@pytest.mark.parametrize("bad", [dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=1.5), dict(ema_decay=float("nan")),
                                 dict(weight_decay=-1e-4), dict(weight_decay=float("inf")), dict(weight_decay=float("nan")),
                                 dict(fused_clip=True), dict(fused_clip=True, grad_clip=0)])
@pytest.mark.parametrize("eval_mode", [False, True])
def test_bad_option_values_raise_value_error_at_construction(tmp_path, bad, eval_mode):
    with pytest.raises(ValueError, match="|".join(bad)):
        _edsr(tmp_path, eval_mode=eval_mode, **bad)


def test_bad_option_values_raise_on_the_kwargs_networks_and_vdsr_too(tmp_path):
    with pytest.raises(ValueError, match="ema_decay"):
        handlers.QRCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ema_decay=1.0, n_resgroups=1,
                              n_resblocks=1)
    with pytest.raises(ValueError, match="fused_clip"):  # VDSR clips by default; grad_clip = 0 turns that off
        sisr_amd.basic.VDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, grad_clip=0, fused_clip=True)


@pytest.mark.parametrize("opts, named", [(dict(ema_decay=0.999), "ema_decay"), (dict(weight_decay=0.01), "weight_decay"),
                                         (dict(fused_clip=True, grad_clip=0.1), "fused_clip")])
def test_options_without_a_flat_adam_raise_runtime_error(tmp_path, opts, named):
    """a CPU handler's optimiser is a plain torch Adam: the options cannot be carried out, and are not dropped silently"""
    with pytest.raises(RuntimeError, match=named + ".*FlatAdam"):
        _edsr(tmp_path, eval_mode=False, **opts)
    with pytest.raises(RuntimeError, match="FlatAdam"):
        sisr_amd.basic.VDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, **opts)


def test_valid_off_values_change_nothing(tmp_path):
    """None, a zero weight decay and fused_clip=False are 'not set': a CPU handler builds its torch Adam as ever (also
    through the handlers that hand **kwargs on to the network); an eval-mode handler has no optimiser to refuse"""
    h = _edsr(tmp_path, eval_mode=False, weight_decay=0.0, ema_decay=None, fused_clip=False)
    assert type(h.optimizer) is torch.optim.Adam and not h.has_ema() and h.fused_clip is False
    h = handlers.QRCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, weight_decay=0, fused_clip=False,
                              n_resgroups=1, n_resblocks=1)
    assert type(h.optimizer) is torch.optim.Adam
    h = _edsr(tmp_path, eval_mode=True, ema_decay=0.999, weight_decay=0.01)
    assert h.optimizer is None and not h.has_ema()
    with pytest.raises(RuntimeError, match="no average"):
        with h.averaged_weights():
            pass


# ----------------------------------------------------------------------------- checkpoint schema
def test_checkpoint_of_a_handler_without_the_options_has_todays_keys(tmp_path):
    h = _edsr(tmp_path, eval_mode=False)
    state = h.save_model("m", 0, extract_state_only=True)
    assert set(state) == {"network", "optimizer", "model_name", "model_epoch"}
    assert set(state["optimizer"]["param_groups"][0]) == set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])
                                                             .state_dict()["param_groups"][0])
    h.save_model("m", 0)
    with pytest.raises(RuntimeError, match="network_ema.*m_0|m_0.*network_ema"):
        _edsr(tmp_path, eval_mode=True).load_model("m", 0, ema=True)
    _edsr(tmp_path, eval_mode=True).load_model("m", 0)
