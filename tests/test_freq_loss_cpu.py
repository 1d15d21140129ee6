"""Frequency-domain (FFT L1) loss: the table-form oracle against torch.fft and the analytic gradient in float64, the test
inputs' kink rule, handler plumbing and host-side argument checks (no GPU)."""
import ctypes as C

import pytest
import torch

import sisr_amd
from sisr_amd import frequency, handlers, perceptual, structural

import _freq_loss as S
import _perceptual as P

CPU = torch.device("cpu")
CASE_IDS = ["%dx%dx%dx%d-%g" % (s + (n,)) for s, n in S.CASES]


# ----------------------------------------------------------------------------- oracle and formula
@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_table_oracle_is_torch_fft_in_float64(case):
    """the matrix form over the tables against the definition through torch.fft.rfft2, both in float64: value and autograd
    gradient within 1e-12 relative"""
    shape, noise = case
    sr, y, _ = S.make_pair(shape, noise)
    sr, y = sr.double(), y.double()
    v, g = S.autograd_grad(sr, y)
    v_fft, g_fft = S.autograd_grad(sr, y, fn=S.fft_l1)
    print(f"oracle {shape} noise {noise}: value {float(v):.6e} vs fft {abs(float(v) - float(v_fft)) / float(v_fft):.2e}, "
          f"gradient {S.rel_l2(g, g_fft):.2e}")
    assert abs(float(v) - float(v_fft)) <= 1e-12 * float(v_fft)
    assert S.rel_l2(g, g_fft) <= 1e-12


@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_analytic_gradient_is_float64_autograd(case):
    shape, noise = case
    sr, y, _ = S.make_pair(shape, noise)
    sr, y = sr.double(), y.double()
    _, want = S.autograd_grad(sr, y)
    got = S.analytic_grad(sr, y)
    assert got.shape == sr.shape
    e = S.rel_l2(got, want)
    print(f"analytic gradient {shape} noise {noise}: rel L2 {e:.3e}")
    assert e <= 1e-12, e


@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_inputs_keep_away_from_the_kinks(case):
    """every non-structural |Re F|, |Im F| of a test input is at least 2e-5 x its noise in float64"""
    shape, noise = case
    sr, y, margin = S.make_pair(shape, noise)
    print(f"kink margin {shape} noise {noise}: {margin:.3e} (rule {S.KINK * noise:.1e})")
    assert sr.dtype == torch.float32 and margin >= S.KINK * noise
    assert S.kink_margin(sr, y) == margin


@pytest.mark.parametrize("shape", S.SHAPES)
def test_structural_imaginary_parts_are_exact_zeros(shape):
    sr, y, _ = S.make_pair(shape, 0.05)
    m = S.structural_mask(*shape[2:])
    assert int(m.sum()) == (2 if shape[2] % 2 == 0 else 1) * (2 if shape[3] % 2 == 0 else 1)
    for dt in (torch.float64, torch.float32):
        _, fi = S.spectrum(sr.to(dt), y.to(dt))
        assert bool((fi[..., m] == 0).all()), dt
    # the definition itself has them zero in exact arithmetic only: that is why the tables are the oracle's form
    ref = torch.fft.rfft2(sr.double() - y.double(), norm="ortho").imag
    assert float(ref[..., m].abs().max()) <= 1e-15


def test_tables_are_exact_at_quarter_turns():
    for n in (2, 8, 75, 128):
        c, s = S.tables(n, n, torch.float32)
        assert c.dtype == torch.float32 and c.shape == (n, n)
        k = torch.arange(n)[:, None] * torch.arange(n)[None, :]
        for q, (cv, sv) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
            hit = (4 * (k % n)) == q * n
            assert bool((c[hit] == cv).all()) and bool((s[hit] == sv).all()), (n, q)
        assert torch.equal(c, c.t()) and torch.equal(s, s.t())  # Ch, Sh are symmetric


# ----------------------------------------------------------------------------- criterion module
def test_mechanism_keeps_the_base_as_a_submodule_and_has_no_parameters():
    base = handlers.L1Loss()
    m = frequency.FrequencyMechanism(base, 0.1)
    assert m.base is base and m.beta == 0.1
    assert list(m.parameters()) == [] and list(m.state_dict()) == []
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="freq_loss"):
            frequency.FrequencyMechanism(base, bad)


# ----------------------------------------------------------------------------- handler wiring
def test_freq_loss_wraps_the_l1_criterion(tmp_path):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, freq_loss=0.1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism)
    assert type(h.criterion.base) is handlers.L1Loss and h.criterion.beta == 0.1 and h.freq_loss == 0.1
    assert list(h.criterion.parameters()) == []
    state = h.save_model("m", 0, extract_state_only=True)
    assert set(state["network"]) == set(h.net.state_dict())
    h2 = handlers.RCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.3)
    assert isinstance(h2.criterion, frequency.FrequencyMechanism) and h2.criterion.beta == 0.3


def test_freq_loss_wraps_the_mse_criterion_of_the_y_channel_handlers(tmp_path):
    for cls in (sisr_amd.basic.SRCNNHandler, sisr_amd.basic.VDSRHandler):
        h = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.1)
        assert isinstance(h.criterion, frequency.FrequencyMechanism), cls.__name__
        assert type(h.criterion.base) is sisr_amd.basic.MSELoss, cls.__name__
        h0 = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False)
        assert type(h0.criterion) is sisr_amd.basic.MSELoss, cls.__name__


def test_wrap_order_is_base_then_structural_then_frequency(tmp_path, monkeypatch):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ssim_loss=0.2,
                             freq_loss=0.1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism)
    assert isinstance(h.criterion.base, structural.StructuralMechanism) and h.criterion.base.alpha == 0.2
    assert type(h.criterion.base.base) is handlers.L1Loss
    monkeypatch.delenv("SISR_VGG19_WEIGHTS", raising=False)
    path = str(tmp_path / "vgg.pth")
    torch.save(P.seeded_state(3, "vgg19_54"), path)
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.05,
                             perceptual_weights=path, ssim_loss=0.2, freq_loss=0.1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism)
    assert isinstance(h.criterion.base, structural.StructuralMechanism)
    assert isinstance(h.criterion.base.base, perceptual.PerceptualMechanism) and h.criterion.base.base.lambda_per == 0.05
    assert list(h.criterion.state_dict()) == ["base.base.vgg_extractor." + k for k in P.state_keys()]
    vgg = {id(p) for p in h.criterion.parameters()}
    assert len(vgg) == 32 and not vgg & {id(p) for grp in h.optimizer.param_groups for p in grp["params"]}
    # perceptual alone under the frequency term
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.05,
                             perceptual_weights=path, freq_loss=0.1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism)
    assert isinstance(h.criterion.base, perceptual.PerceptualMechanism)


def test_meta_attention_and_kwargs_networks_take_the_key(tmp_path):
    """QRCANHandler, QEDSRHandler and the SPARNet / SRMD / SFTMD handlers hand their **kwargs on to the network as well:
    `freq_loss` must pass through both, as `ssim_loss` does"""
    h = handlers.QRCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.1, n_resgroups=1,
                              n_resblocks=1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism) and type(h.criterion.base) is handlers.L1Loss
    h = handlers.QEDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.1, num_blocks=1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism) and type(h.criterion.base) is handlers.L1Loss
    small = dict(min_ch=32, max_ch=32, in_size=16, out_size=16, min_feat_size=8, res_depth=1)
    for cls, extra in ((sisr_amd.sparnet.SPARNetHandler, {}), (sisr_amd.sparnet.QSPARNetHandler, {"metadata": ["blur_sigma"]})):
        h = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.1, **small, **extra)
        assert isinstance(h.criterion, frequency.FrequencyMechanism), cls.__name__
        assert type(h.criterion.base) is handlers.L1Loss, cls.__name__
    h = sisr_amd.srmd.SRMDHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.1,
                                  metadata=["blur_sigma"], nb=1, nc=64)
    assert isinstance(h.criterion, frequency.FrequencyMechanism)
    h = sisr_amd.sftmd.SFTMDHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.1,
                                    metadata=["blur_sigma"], nb=1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism)
    for cls in (handlers.HANHandler, sisr_amd.san.SANHandler):
        h = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=0.1, n_resgroups=1, n_resblocks=1)
        assert isinstance(h.criterion, frequency.FrequencyMechanism), cls.__name__


def test_unset_and_zero_leave_the_criterion_as_it_is(tmp_path):
    for v in (None, 0, 0.0):
        h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, freq_loss=v)
        assert type(h.criterion) is handlers.L1Loss, v
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1)
    assert type(h.criterion) is handlers.L1Loss and h.freq_loss is None
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ssim_loss=0.2)
    assert type(h.criterion) is structural.StructuralMechanism


def test_bad_weight_raises(tmp_path):
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="freq_loss"):
            handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, freq_loss=bad)
    with pytest.raises(ValueError, match="freq_loss"):
        sisr_amd.basic.VDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, freq_loss=-1)


def test_eval_mode_does_not_wrap(tmp_path):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, num_blocks=1, freq_loss=0.1)
    assert type(h.criterion) is handlers.L1Loss
    h = sisr_amd.basic.SRCNNHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, freq_loss=0.1)
    assert type(h.criterion) is sisr_amd.basic.MSELoss


# ----------------------------------------------------------------------------- entry points and operator
def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """sisr_freq_loss and sisr_freq_loss_tables validate on the host and return an error code: no launch is made, so this
    runs without a GPU (the pointers are host stand-ins that must never be dereferenced)"""
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -4
    tb, wsb = L.sisr_freq_loss_table_bytes, L.sisr_freq_loss_workspace_bytes
    assert tb(43, 75) == (2 * 43 * 43 + 2 * 38 * 75) * 4 and tb(2, 2) == (2 * 4 + 2 * 4) * 4
    assert tb(1, 8) == 0 and tb(8, 1) == 0 and tb(4097, 8) == 0 and tb(8, 4097) == 0 and tb(4096, 4096) > 0
    # 2 planes of 43 x 75: 43 x 38 bins = one tile per plane -> 16 bytes of partials; two fp32 maps; the sign bytes padded to 16
    assert wsb(2, 43, 75, 0) == 16 + 2 * 2 * 43 * 38 * 4
    assert wsb(2, 43, 75, 1) == 16 + 2 * 2 * 43 * 38 * 4 + 3280
    assert wsb(1, 128, 128, 0) == 4 * 8 + 2 * 128 * 65 * 4  # 2 x 2 tiles: Wh = 65 is one past the tile
    assert wsb(0, 43, 75, 1) == 0 and wsb(-1, 43, 75, 0) == 0 and wsb(1, 1, 75, 1) == 0 and wsb(1, 43, 4097, 0) == 0
    big = 1 << 30
    t = L.sisr_freq_loss_tables
    assert t(8, 8, None, None) == ERR_ARG
    assert t(1, 8, a, None) == ERR_ARG and t(8, 1, a, None) == ERR_ARG
    assert t(4097, 8, a, None) == ERR_ARG and t(8, 4097, a, None) == ERR_ARG
    assert t(8, 8, a + 2, None) == ERR_ALIGN
    f = L.sisr_freq_loss
    # null operands
    assert f(None, a, 1, 16, 16, a, a, a, a, big, None) == ERR_ARG
    assert f(a, None, 1, 16, 16, a, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, None, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, a, None, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, a, a, a, None, big, None) == ERR_ARG
    # planes < 1, a side below 2 or above the cap
    assert f(a, a, 0, 16, 16, a, a, a, a, big, None) == ERR_ARG
    assert f(a, a, -3, 16, 16, a, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 1, 16, a, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 1, a, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 4097, 16, a, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 4097, a, a, a, a, big, None) == ERR_ARG
    # workspace too small: for the value alone, and for the sign map
    assert f(a, a, 1, 16, 16, a, a, None, a, wsb(1, 16, 16, 0) - 1, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, a, a, a, a, wsb(1, 16, 16, 1) - 1, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, a, a, a, a, wsb(1, 16, 16, 0), None) == ERR_ARG
    # misaligned pointers
    assert f(a, a, 1, 16, 16, a, a, a, a + 8, big, None) == ERR_ALIGN
    assert f(a + 2, a, 1, 16, 16, a, a, a, a, big, None) == ERR_ALIGN
    assert f(a, a + 1, 1, 16, 16, a, a, a, a, big, None) == ERR_ALIGN
    assert f(a, a, 1, 16, 16, a + 2, a, a, a, big, None) == ERR_ALIGN
    assert f(a, a, 1, 16, 16, a, a + 2, a, a, big, None) == ERR_ALIGN
    assert f(a, a, 1, 16, 16, a, a, a + 2, a, big, None) == ERR_ALIGN
    # more planes than the grid's third extent takes
    assert f(a, a, 65536, 2, 2, a, a, a, a, big, None) == ERR_UNSUPPORTED


def test_operator_has_no_cpu_path_and_names_the_extent():
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        sisr_amd.ops.spectral_l1(x, x.clone())
    for shape in ((1, 1, 1, 16), (1, 1, 16, 1), (1, 1, 4097, 2), (1, 1, 2, 4097)):
        t = torch.empty(shape)
        with pytest.raises(ValueError, match=r"extent \(%d, %d\)" % shape[2:]):
            sisr_amd.ops.spectral_l1(t, t.clone())
    for shape in ((0, 3, 16, 16), (2, 0, 16, 16)):
        t = torch.empty(shape)
        with pytest.raises(ValueError, match="empty batch"):
            sisr_amd.ops.spectral_l1(t, t.clone())
    with pytest.raises(RuntimeError, match="one shape"):
        sisr_amd.ops.spectral_l1(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))
    with pytest.raises(RuntimeError, match="one shape"):
        sisr_amd.ops.spectral_l1(torch.rand(3, 16, 16), torch.rand(3, 16, 16))
