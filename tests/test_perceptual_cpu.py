"""Perceptual (VGG19 feature) loss: module, weight loading, handler plumbing and host-side argument checks (no GPU)."""
import ctypes as C

import pytest
import torch

import sisr_amd
from sisr_amd import handlers, perceptual

import _perceptual as P

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def weight_files(tmp_path_factory):
    """seeded VGG19 weights on disk, under the reference's keys and under torchvision's (plus classifier entries)"""
    d = tmp_path_factory.mktemp("vgg")
    ref = P.seeded_state(3, "vgg19_54")
    tv = {k.replace("vgg19_54.", "features."): v for k, v in ref.items()}
    tv["classifier.0.weight"] = torch.zeros(4, 4)
    tv["classifier.0.bias"] = torch.zeros(4)
    torch.save(ref, d / "ref.pth")
    torch.save(tv, d / "tv.pth")
    return ref, str(d / "ref.pth"), str(d / "tv.pth"), d


def test_state_dict_keys_and_shapes_are_the_references():
    m = perceptual.VGGFeatureExtractor()
    sd = m.state_dict()
    assert list(sd.keys()) == P.state_keys()
    for i, (co, ci) in P.shapes().items():
        assert tuple(sd[f"vgg19_54.{i}.weight"].shape) == (co, ci, 3, 3)
        assert tuple(sd[f"vgg19_54.{i}.bias"].shape) == (co,)
    assert len(m.vgg19_54) == 35


def test_all_parameters_are_frozen():
    m = perceptual.PerceptualMechanism(lambda_per=0.01)
    ps = list(m.parameters())
    assert len(ps) == 32 and not any(p.requires_grad for p in ps)
    assert m.lambda_pixel == 1 and m.lambda_per == 0.01


def test_both_key_spellings_load(weight_files):
    ref, ref_path, tv_path, _ = weight_files
    for path in (ref_path, tv_path):
        m = perceptual.VGGFeatureExtractor()
        assert perceptual.load_vgg19_weights(m, path) is m
        sd = m.state_dict()
        assert all(torch.equal(sd[k], ref[k]) for k in P.state_keys())
        assert not any(p.requires_grad for p in m.parameters())


def test_stock_modules_compute_the_restated_features(weight_files):
    """the nn.Sequential that carries the parameters IS torchvision's features[:35]: run as stock torch on the host it
    gives the helper's restatement bit for bit (conv5_4 before its ReLU, four pools)"""
    ref, ref_path, _, _ = weight_files
    m = perceptual.load_vgg19_weights(perceptual.VGGFeatureExtractor(), ref_path)
    x = torch.rand(1, 3, 16, 32, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        got = m.vgg19_54((x - m.mean) / m.std)
    assert got.shape == (1, 512, 1, 2)
    assert torch.equal(got, P.phi(x, ref))


def test_missing_layer_and_wrong_shape_raise_naming_the_key(weight_files):
    ref, _, _, d = weight_files
    missing = {k: v for k, v in ref.items() if k != "vgg19_54.21.bias"}
    torch.save(missing, d / "missing.pth")
    with pytest.raises(KeyError, match=r"features\.21\.bias.*vgg19_54\.21\.bias"):
        perceptual.load_vgg19_weights(perceptual.VGGFeatureExtractor(), str(d / "missing.pth"))
    wrong = dict(ref)
    wrong["vgg19_54.5.weight"] = torch.zeros(128, 64, 1, 1)
    torch.save(wrong, d / "wrong.pth")
    with pytest.raises(ValueError, match=r"vgg19_54\.5\.weight.*\(128, 64, 1, 1\)"):
        perceptual.load_vgg19_weights(perceptual.VGGFeatureExtractor(), str(d / "wrong.pth"))


def test_handler_without_weights_names_both_sources(tmp_path, monkeypatch):
    monkeypatch.delenv("SISR_VGG19_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError) as e:
        handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.01)
    assert "perceptual_weights" in str(e.value) and "SISR_VGG19_WEIGHTS" in str(e.value)
    assert "outside the HIP hot path" not in str(e.value)
    with pytest.raises(RuntimeError, match="perceptual_weights.*SISR_VGG19_WEIGHTS"):
        handlers.RCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, perceptual=0.01)


def test_handler_builds_the_criterion_beside_the_network(tmp_path, monkeypatch, weight_files):
    ref, ref_path, tv_path, _ = weight_files
    monkeypatch.delenv("SISR_VGG19_WEIGHTS", raising=False)
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.05,
                             perceptual_weights=ref_path)
    assert isinstance(h.criterion, perceptual.PerceptualMechanism)
    assert h.criterion.lambda_per == 0.05 and h.criterion.lambda_pixel == 1
    assert torch.equal(h.criterion.vgg_extractor.state_dict()["vgg19_54.34.weight"], ref["vgg19_54.34.weight"])
    vgg = {id(p) for p in h.criterion.parameters()}
    assert len(vgg) == 32
    assert not vgg & {id(p) for grp in h.optimizer.param_groups for p in grp["params"]}
    assert not vgg & {id(p) for p in h.net.parameters()}
    state = h.save_model("m", 0, extract_state_only=True)
    assert not any("vgg" in k for k in state["network"])
    assert set(state["network"]) == set(h.net.state_dict())
    # the environment variable is the second source
    monkeypatch.setenv("SISR_VGG19_WEIGHTS", tv_path)
    h2 = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.01)
    assert torch.equal(h2.criterion.vgg_extractor.state_dict()["vgg19_54.0.weight"], ref["vgg19_54.0.weight"])
    # evaluation handlers never build it (ref: models/__init__.py:341)
    h3 = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, num_blocks=1, perceptual=0.01)
    assert type(h3.criterion) is handlers.L1Loss


def test_meta_attention_handler_takes_it_too(tmp_path, monkeypatch, weight_files):
    """QRCANHandler hands its **kwargs on to the network as well: `perceptual_weights` must pass through both, and its
    'augmented_rgb' colorspace is an RGB one"""
    _, ref_path, _, _ = weight_files
    monkeypatch.delenv("SISR_VGG19_WEIGHTS", raising=False)
    h = handlers.QRCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, perceptual=0.01,
                              perceptual_weights=ref_path, n_resgroups=1, n_resblocks=1)
    assert isinstance(h.criterion, perceptual.PerceptualMechanism)
    assert not {id(p) for p in h.criterion.parameters()} & {id(p) for grp in h.optimizer.param_groups for p in grp["params"]}


def test_sparnet_handlers_keep_the_perceptual_criterion(tmp_path, monkeypatch, weight_files):
    """The reference's SPARNet handlers set criterion = nn.L1Loss() again after training_setup, which drops the perceptual
    criterion without a word (ref: SPARNet/handlers.py:17, :33).  Here the option holds on them as on every other RGB handler;
    without it they train on L1 as before."""
    _, ref_path, _, _ = weight_files
    monkeypatch.delenv("SISR_VGG19_WEIGHTS", raising=False)
    small = dict(min_ch=32, max_ch=32, in_size=16, out_size=16, min_feat_size=8, res_depth=1)
    for cls, extra in ((sisr_amd.sparnet.SPARNetHandler, {}), (sisr_amd.sparnet.QSPARNetHandler, {"metadata": ["blur_sigma"]})):
        h = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, perceptual=0.01, perceptual_weights=ref_path,
                **small, **extra)
        assert isinstance(h.criterion, perceptual.PerceptualMechanism) and h.criterion.lambda_per == 0.01, cls.__name__
        vgg = {id(p) for p in h.criterion.parameters()}
        assert len(vgg) == 32 and not vgg & {id(p) for grp in h.optimizer.param_groups for p in grp["params"]}
        assert not any("vgg" in k for k in h.save_model("m", 0, extract_state_only=True)["network"])
        h0 = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, perceptual=None, **small, **extra)
        assert type(h0.criterion) is handlers.L1Loss, cls.__name__
        with pytest.raises(RuntimeError, match="perceptual_weights.*SISR_VGG19_WEIGHTS"):
            cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, perceptual=0.01, **small, **extra)


def test_y_channel_handlers_refuse_by_name(tmp_path, weight_files):
    _, ref_path, _, _ = weight_files
    for cls in (sisr_amd.basic.SRCNNHandler, sisr_amd.basic.VDSRHandler):
        with pytest.raises(NotImplementedError, match=cls.__name__ + ".*ycbcr"):
            cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, perceptual=0.01, perceptual_weights=ref_path)


def test_reduced_precision_modes_refuse(tmp_path, weight_files, monkeypatch):
    _, ref_path, _, _ = weight_files
    monkeypatch.setattr(sisr_amd.ops, "PRECISION", "bf16")
    with pytest.raises(NotImplementedError, match="perceptual loss.*fp32"):
        handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.01,
                             perceptual_weights=ref_path)


def test_no_perceptual_keeps_the_l1_criterion(tmp_path):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=None)
    assert type(h.criterion) is handlers.L1Loss
    assert h.perceptual_weights is None


def test_extractor_has_no_cpu_path():
    m = perceptual.VGGFeatureExtractor()
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 3, 16, 16))


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """sisr_vgg_prep_fwd / _bwd and sisr_maxpool2_fwd / _relu_bwd validate on the host and return an error code: no launch is
    made, so this runs without a GPU (the pointers are host stand-ins that must never be dereferenced)."""
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    # null map
    assert L.sisr_vgg_prep_fwd(None, a, a, a, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_vgg_prep_fwd(a, a, a, None, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_vgg_prep_fwd(a, None, a, a, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_vgg_prep_bwd(None, a, a, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_vgg_prep_bwd(a, a, None, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_fwd(None, a, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_fwd(a, None, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_relu_bwd(None, a, a, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_relu_bwd(a, None, a, 1, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_relu_bwd(a, a, None, 1, 8, 8, 64, None) == ERR_ARG
    # C = 60: not a multiple of 64
    assert L.sisr_vgg_prep_fwd(a, a, a, a, 1, 8, 8, 60, None) == ERR_UNSUPPORTED
    assert L.sisr_vgg_prep_bwd(a, a, a, 1, 8, 8, 60, None) == ERR_UNSUPPORTED
    assert L.sisr_maxpool2_fwd(a, a, 1, 8, 8, 60, None) == ERR_UNSUPPORTED
    assert L.sisr_maxpool2_relu_bwd(a, a, a, 1, 8, 8, 60, None) == ERR_UNSUPPORTED
    # H = 1 (or W = 1): no 2 x 2 window
    assert L.sisr_maxpool2_fwd(a, a, 1, 1, 8, 64, None) == ERR_UNSUPPORTED
    assert L.sisr_maxpool2_fwd(a, a, 1, 8, 1, 64, None) == ERR_UNSUPPORTED
    assert L.sisr_maxpool2_relu_bwd(a, a, a, 1, 1, 8, 64, None) == ERR_UNSUPPORTED
    assert L.sisr_maxpool2_relu_bwd(a, a, a, 1, 8, 1, 64, None) == ERR_UNSUPPORTED
    # B = 0, and non-positive sizes
    assert L.sisr_vgg_prep_fwd(a, a, a, a, 0, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_vgg_prep_bwd(a, a, a, 0, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_fwd(a, a, 0, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_relu_bwd(a, a, a, 0, 8, 8, 64, None) == ERR_ARG
    assert L.sisr_vgg_prep_fwd(a, a, a, a, 1, 0, 8, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_fwd(a, a, 1, 8, -2, 64, None) == ERR_ARG
    assert L.sisr_maxpool2_fwd(a, a, 1, 8, 8, 0, None) == ERR_ARG


def test_rounded_once_l1_entry_point_refuses_bad_arguments_before_any_device_call():
    """sisr_l1_loss_mean: null operands, n <= 0 and a misaligned workspace are refused on the host; its workspace is one double
    per block where sisr_l1_loss's is one float"""
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    ERR_ARG, ERR_ALIGN = -1, -2
    assert L.sisr_l1_loss_mean_workspace_bytes() == 2 * L.sisr_l1_loss_workspace_bytes()
    assert L.sisr_l1_loss_mean(None, a, 16, a, a, a, None) == ERR_ARG
    assert L.sisr_l1_loss_mean(a, None, 16, a, a, a, None) == ERR_ARG
    assert L.sisr_l1_loss_mean(a, a, 16, None, a, a, None) == ERR_ARG
    assert L.sisr_l1_loss_mean(a, a, 16, a, a, None, None) == ERR_ARG
    assert L.sisr_l1_loss_mean(a, a, 0, a, a, a, None) == ERR_ARG
    assert L.sisr_l1_loss_mean(a, a, 16, a, a, a + 8, None) == ERR_ALIGN
