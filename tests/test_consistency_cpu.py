"""Degradation-consistency loss, host side (no GPU): the interior taps against Pillow's table, the composed kernel and the flip
identity against the three-step float64 twin, the margins, argument checks and handler plumbing."""
import itertools

import numpy as np
import pytest
import torch

import sisr_amd
from sisr_amd import consistency, degrade, frequency, handlers, ops

import _consistency as S

CPU = torch.device("cpu")
SCALES = (2, 3, 4)
EDGES = (1, 7, 21)


# ----------------------------------------------------------------------------- the taps
@pytest.mark.parametrize("s", SCALES)
def test_interior_taps_are_rows_2_to_out_minus_3_of_pillows_table(s):
    """bicubic_interior_taps(s) against coef / 2^22 of pil_bicubic_table(64 s, 64), rows 2 .. 61, relative to s i: within the
    fixed-point rounding 2^-23 per tap, and nothing but zero-weight taps outside them"""
    first, w = degrade.bicubic_interior_taps(s)
    bounds, coef, _ = degrade.pil_bicubic_table(64 * s, 64)
    assert (first, len(w)) == {4: (-6, 16), 3: (-4, 11), 2: (-3, 8)}[s]
    for i in range(2, 62):
        row = np.zeros(40)
        lo, cnt = bounds[i]
        row[lo - s * i + 10:lo - s * i + 10 + cnt] = coef[i, :cnt] / 2.0 ** degrade.PRECISION_BITS
        want = np.zeros(40)
        want[first + 10:first + 10 + len(w)] = w
        assert np.abs(row - want).max() <= 2.0 ** -23, (s, i)


@pytest.mark.parametrize("s", SCALES)
def test_taps_are_symmetric_and_sum_to_one(s):
    first, w = degrade.bicubic_interior_taps(s)
    assert w.dtype == np.float64 and w[0] != 0 and w[-1] != 0  # (s = 3 has two taps of weight 0 inside: the filter's zeros at +-1)
    assert np.array_equal(w, w[::-1])
    assert abs(w.sum() - 1.0) <= 4e-16
    assert first + (first + len(w) - 1) == s - 1  # centred on the s-pixel cell: what makes flips commute with D


def test_other_scales_raise():
    for bad in (1, 5, 8, 2.5, True, None):
        with pytest.raises(ValueError, match="scale"):
            degrade.bicubic_interior_taps(bad)


# ----------------------------------------------------------------------------- margins
def test_margins():
    assert [degrade.consistency_margin(s, 21) for s in (4, 3, 2)] == [4, 5, 7]
    assert degrade.consistency_margin(4, 1) == 2
    for s, l in itertools.product(SCALES, EDGES):  # ... and by the definition, from the footprints
        assert degrade.consistency_margin(s, l) == S.margin(s, l), (s, l)
        first, w = degrade.bicubic_interior_taps(s)
        assert degrade.consistency_geometry(s, len(w) + l - 1) == (l, S.margin(s, l), s * S.margin(s, l) + first - l // 2)
    for bad in (0, 2, 23):
        with pytest.raises(ValueError, match="blur kernel edge"):
            degrade.consistency_margin(4, bad)


# ----------------------------------------------------------------------------- the composed kernel
@pytest.mark.parametrize("s,l", list(itertools.product(SCALES, EDGES)))
def test_composed_kernel_is_the_three_step_degradation(s, l):
    """compose_degradation applied as a strided correlation against blur -> horizontal pass -> vertical pass, float64 against
    float64 on random data with two different anisotropic kernels, at every kept output: 1e-13 relative"""
    m = degrade.consistency_margin(s, l)
    k = S.kernels(2, l, seed=10 * s + l)
    if l > 1:
        assert not torch.equal(k[0], k[1]) and not torch.allclose(k[0], k[0].T) and not torch.allclose(k[0], k[0].flip(1))
    x = S.image(2, 3, s * (2 * m + 5), s * (2 * m + 8), seed=s + l)
    K, first = degrade.compose_degradation(k.numpy(), s)
    first_w, w = degrade.bicubic_interior_taps(s)
    assert K.dtype == np.float64 and K.shape == (2, len(w) + l - 1, len(w) + l - 1) and first == first_w - l // 2
    got = S.strided_correlation(x, torch.from_numpy(K), s, first, m)
    want = S.twin(x, k, s)
    assert got.shape == want.shape == (2, 3, 5, 8)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"s {s} l {l}: n {K.shape[1]} m {m} max rel err {err:.2e}")
    assert err <= 1e-13
    assert S.rel_l2(S.stock(x, k, s), want) <= 1e-13  # the yardstick's composition is the same operator


def test_one_output_tile():
    """h = 2m + 1: the one kept output, every scale, against the twin"""
    for s in SCALES:
        m = degrade.consistency_margin(s, 21)
        k = S.kernels(2, 21, seed=s)
        x = S.image(2, 1, s * (2 * m + 1), s * (2 * m + 1), seed=40 + s)
        K, first = degrade.compose_degradation(k.numpy(), s)
        got, want = S.strided_correlation(x, torch.from_numpy(K), s, first, m), S.twin(x, k, s)
        assert got.shape == want.shape == (2, 1, 1, 1)
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-13


@pytest.mark.parametrize("s", SCALES)
def test_flips_commute_once_the_kernel_is_transformed(s):
    """all eight (hflip, vflip, transpose): T(D_k(x)) on the kept region == D of T x with compose_degradation(k, s, flips),
    to 1e-13; and without transforming the kernel the identity fails for an anisotropic one"""
    l = 7
    m = degrade.consistency_margin(s, l)
    k = S.kernels(1, l, seed=3)
    x = S.image(1, 2, s * (2 * m + 4), s * (2 * m + 4), seed=9)  # square: the transpose keeps the shape
    base = S.twin(x, k, s)
    K0, first = degrade.compose_degradation(k.numpy(), s)
    failed = 0
    for flips in itertools.product((0, 1), repeat=3):
        want = S.augment(base, flips)
        K, _ = degrade.compose_degradation(k.numpy(), s, np.array([flips]))
        got = S.strided_correlation(S.augment(x, flips).contiguous(), torch.from_numpy(K), s, first, m)
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-13, flips
        plain = S.strided_correlation(S.augment(x, flips).contiguous(), torch.from_numpy(K0), s, first, m)
        failed += float((plain - want).abs().max()) > 1e-6
    assert failed == 7  # every transform but the identity needs the kernel's


def test_compose_checks_its_arguments():
    with pytest.raises(ValueError, match="odd"):
        degrade.compose_degradation(np.ones((1, 4, 4)), 4)
    with pytest.raises(ValueError, match="21"):
        degrade.compose_degradation(np.ones((1, 23, 23)), 4)
    with pytest.raises(ValueError, match="flips"):
        degrade.compose_degradation(np.ones((2, 3, 3)), 4, np.zeros((1, 3)))
    with pytest.raises(ValueError, match="scale"):
        degrade.compose_degradation(np.ones((1, 3, 3)), 5)


# ----------------------------------------------------------------------------- the operator's host-side checks
def test_a_tile_without_a_kept_output_raises_with_the_sizes():
    """h = 2m (and w = 2m) raise before anything touches a device; the message names the sizes"""
    K = torch.from_numpy(degrade.compose_degradation(S.kernels(1, 21, seed=1).numpy(), 4)[0])
    for h, w in ((8, 9), (9, 8), (8, 8), (3, 20)):
        with pytest.raises(ValueError, match=f"{h} x {w} LR tile.*{4 * h} x {4 * w} HR tile.*2 m = 8"):
            ops.degrade_valid(torch.zeros(1, 3, 4 * h, 4 * w), K, 4)
    with pytest.raises(RuntimeError, match="HIP device|CPU"):  # h = 2m + 1 passes the checks; there is no CPU path behind them
        ops.degrade_valid(torch.zeros(1, 3, 36, 36), K, 4)
    with pytest.raises(ValueError, match="multiple of the scale"):
        ops.degrade_valid(torch.zeros(1, 3, 37, 36), K, 4)
    with pytest.raises(RuntimeError, match="B, n, n"):
        ops.degrade_valid(torch.zeros(2, 3, 36, 36), K, 4)
    with pytest.raises(ValueError, match="no odd blur edge"):
        ops.degrade_valid(torch.zeros(1, 3, 36, 36), K[:, :35, :35], 4)


def test_entry_points_refuse_bad_geometry_before_any_device_call():
    """a footprint that would leave the image, a negative offset, an unknown scale, a kernel beyond the LDS tile: error codes, no
    launch"""
    import ctypes as C
    L = sisr_amd.hip.lib()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    for fn in (L.sisr_degrade_valid_fwd, L.sisr_degrade_valid_bwd):
        assert fn(a, a, a, 1, 1, 36, 36, 36, 4, 1, 1, 1, None) == -1   # 0 + 1 + 36 > 36
        assert fn(a, a, a, 1, 1, 36, 40, 36, 4, 0, 1, 3, None) == -1   # along W: 8 + 36 > 40
        assert fn(a, a, a, 1, 1, 36, 36, 36, 4, -1, 1, 1, None) == -1
        assert fn(None, a, a, 1, 1, 36, 36, 36, 4, 0, 1, 1, None) == -1
        assert fn(a, a, a, 1, 1, 64, 64, 36, 5, 0, 1, 1, None) == -4
        assert fn(a, a, a, 1, 1, 64, 64, 37, 4, 0, 1, 1, None) == -4
        assert fn(a, a + 4, a, 1, 1, 36, 36, 36, 4, 0, 1, 1, None) == -2   # K must be 8-byte aligned
    assert L.sisr_degrade_valid_tile(0) == ops.degrade_valid_tile() > 0
    assert L.sisr_degrade_valid_tile(1) == ops.degrade_valid_tile(backward=True) > 0


# ----------------------------------------------------------------------------- the mechanism and the handlers
def test_bad_weight_raises(tmp_path):
    for bad in (-0.1, float("nan"), float("inf"), "0.1", True):
        with pytest.raises(ValueError, match="consistency_loss"):
            handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, consistency_loss=bad)
        with pytest.raises(ValueError, match="consistency_loss"):
            consistency.ConsistencyMechanism(handlers.L1Loss(), bad, 4)
    with pytest.raises(ValueError, match="scales"):
        consistency.ConsistencyMechanism(handlers.L1Loss(), 0.1, 8)


def test_unset_and_zero_leave_the_criterion_as_it_is(tmp_path):
    for v in (None, 0, 0.0):
        h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, consistency_loss=v)
        assert type(h.criterion) is handlers.L1Loss and h._consistency is None, v
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1)
    assert type(h.criterion) is handlers.L1Loss and h.consistency_loss is None
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, num_blocks=1, consistency_loss=0.1)
    assert type(h.criterion) is handlers.L1Loss  # evaluation handlers do not wrap


def test_lr_rgb_handlers_take_the_key_outermost(tmp_path):
    """EDSR, RCAN, HAN, SAN, their Q forms, SRMD and SFTMD: the mechanism wraps whatever criterion there is, the frequency term
    included; nothing of it reaches the checkpoint or the optimiser"""
    d = dict(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, consistency_loss=0.25)
    small = dict(n_resgroups=1, n_resblocks=1)
    made = [handlers.EDSRHandler(num_blocks=1, freq_loss=0.1, **d), handlers.QEDSRHandler(num_blocks=1, **d),
            handlers.QRCANHandler(**small, **d), handlers.HANHandler(**small, **d), handlers.QHANHandler(**small, **d),
            sisr_amd.san.SANHandler(**small, **d), sisr_amd.san.QSANHandler(**small, **d),
            sisr_amd.srmd.SRMDHandler(metadata=["blur_sigma"], nb=1, nc=64, **d),
            sisr_amd.sftmd.SFTMDHandler(metadata=["blur_sigma"], nb=1, **d)]
    for h in made:
        name = type(h).__name__
        assert isinstance(h.criterion, consistency.ConsistencyMechanism) and h.criterion is h._consistency, name
        assert h.criterion.gamma == 0.25 and h.criterion._bound is None, name
        assert not list(h.criterion.parameters()) and not list(h.criterion.state_dict()), name
    assert isinstance(made[0].criterion.base, frequency.FrequencyMechanism)
    assert type(made[0].criterion.base.base) is handlers.L1Loss and type(made[1].criterion.base) is handlers.L1Loss


def test_interpolated_input_y_channel_and_code_models_refuse_the_key(tmp_path):
    """SPARNet (interpolated RGB input), VDSR / SRCNN (interpolated Y input), the predictor and the corrector (their output is a
    code): NotImplementedError with a sentence saying why, in training and in evaluation mode"""
    d = dict(device=CPU, model_save_dir=str(tmp_path), consistency_loss=0.1)
    small = dict(min_ch=32, max_ch=32, in_size=16, out_size=16, min_feat_size=8, res_depth=1)
    for mode in (False, True):
        with pytest.raises(NotImplementedError, match="consistency_loss.*interpolated"):
            sisr_amd.sparnet.SPARNetHandler(eval_mode=mode, **small, **d)
        with pytest.raises(NotImplementedError, match="consistency_loss.*interpolated"):
            sisr_amd.basic.VDSRHandler(eval_mode=mode, **d)
    with pytest.raises(NotImplementedError, match="consistency_loss.*interpolated"):
        sisr_amd.sparnet.QSPARNetHandler(eval_mode=False, metadata=["blur_sigma"], **small, **d)
    with pytest.raises(NotImplementedError, match="consistency_loss.*interpolated"):
        sisr_amd.basic.SRCNNHandler(eval_mode=False, **d)
    with pytest.raises(NotImplementedError, match="consistency_loss.*code"):
        sisr_amd.predictor.PredictorHandler(eval_mode=False, **d)
    # without the key they build as before
    assert type(sisr_amd.basic.VDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False).criterion) is sisr_amd.basic.MSELoss


def test_mechanism_without_a_binding_is_its_base():
    """nothing bound (run_eval(request_loss=True)): base(sr, y) alone, whatever gamma is; bind / clear toggle it"""
    calls = []

    class Base(torch.nn.Module):
        def forward(self, sr, y):
            calls.append(1)
            return (sr - y).abs().mean()

    crit = consistency.ConsistencyMechanism(Base(), 3.0, 4)
    sr, y = torch.rand(1, 3, 36, 36), torch.rand(1, 3, 36, 36)
    assert torch.equal(crit(sr, y), (sr - y).abs().mean()) and calls == [1]
    K = torch.from_numpy(degrade.compose_degradation(S.kernels(1, 21, seed=1).numpy(), 4)[0])
    crit.bind(torch.rand(1, 3, 9, 9), K)
    with pytest.raises(RuntimeError, match="HIP device|CPU"):  # bound: the operator is reached (and has no CPU path)
        crit(sr, y)
    crit.bind(torch.rand(1, 3, 8, 9), K)
    with pytest.raises(RuntimeError, match="is not x 4"):
        crit(sr, y)
    crit.clear()
    assert torch.equal(crit(sr, y), (sr - y).abs().mean())


def test_train_step_needs_the_batchs_kernels(tmp_path):
    """a batch without kernels -- the zeros of an offline set -- raises a clear error when the term is on, before any launch"""
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, consistency_loss=0.1)
    x, y = torch.rand(2, 3, 12, 12), torch.rand(2, 3, 48, 48)
    for kw in ({}, {"blur_kernels": torch.zeros(2, dtype=torch.int64)}, {"blur_kernels": torch.rand(3, 21, 21)}):
        with pytest.raises(RuntimeError, match="consistency_loss: the batch carries no blur kernels"):
            h.train_step(x, y, **kw)
        assert h.criterion._bound is None
    lr, K = h._consistency_operands(torch.rand(2, 13, 12, 12), y, {"blur_kernels": S.kernels(2, 21, seed=2), "flips": torch.tensor([[1, 0, 1], [0, 0, 0]])})
    assert lr.shape == (2, 3, 12, 12) and K.dtype == torch.float64 and K.shape == (2, 36, 36)  # SRMD: metadata planes behind the image
    want, _ = degrade.compose_degradation(S.kernels(2, 21, seed=2).numpy(), 4, np.array([[1, 0, 1], [0, 0, 0]]))
    assert np.array_equal(K.numpy(), want)
    plain = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1)
    assert plain._consistency_operands(x, y, {}) is None


# ----------------------------------------------------------------------------- the loaders' flags
def test_random_flip_rotate_reports_its_draws():
    import random
    from sisr_amd import data
    lr, hr = torch.rand(3, 5, 7), torch.rand(3, 20, 28)
    for seed in range(8):
        random.seed(seed)
        a = data.random_flip_rotate(lr, hr)
        random.seed(seed)
        b_lr, b_hr, flips = data.random_flip_rotate(lr, hr, want_flags=True)
        assert torch.equal(a[0], b_lr) and torch.equal(a[1], b_hr)
        assert torch.equal(S.augment(lr, flips), b_lr) and torch.equal(S.augment(hr, flips), b_hr)
    assert torch.equal(data._flip_table([(3, 4, True, False, True), (0, 0, False, False, False)]), torch.tensor([[1, 0, 1], [0, 0, 0]]))
