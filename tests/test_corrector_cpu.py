"""IKC's Corrector, the parts that need no GPU: the refusals of the pointwise entry points, the algebra of the folded first
head layer, and the constructor."""
import ctypes as C
import os

import pytest
import torch

import _corrector as T
import _predictor as P
import sisr_amd

ARG, ALIGN, UNSUPPORTED = -1, -2, -4


def test_pointwise_entry_points_refuse_bad_arguments_before_any_device_call():
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    assert a % 16 == 0
    nan = float("nan")

    def fwd(x=a, mask=None, packed=a, cin_p=128, cout_p=128, nbias=128, slope=0.2, B=1):
        return L.sisr_conv1_mfma_leaky(x, mask, packed, a, a, nbias, a, B, 8, 8, cin_p, cout_p, 1, slope, None)

    assert fwd(x=None) == ARG and fwd(packed=None) == ARG and fwd(B=0) == ARG and fwd(slope=nan) == ARG and fwd(nbias=-1) == ARG
    assert fwd(cin_p=48) == UNSUPPORTED and fwd(cout_p=96) == UNSUPPORTED and fwd(cout_p=256) == UNSUPPORTED
    assert fwd(cout_p=64, nbias=65) == UNSUPPORTED
    assert fwd(x=a + 4) == ALIGN and fwd(mask=a + 4) == ALIGN and fwd(packed=a + 4) == ALIGN
    assert L.sisr_pack_conv1(None, a, a, 128, 128, 128, 128, None) == ARG
    assert L.sisr_pack_conv1(a, a, a, 129, 128, 128, 128, None) == UNSUPPORTED
    assert L.sisr_pack_conv1(a, a, a, 96, 96, 96, 128, None) == UNSUPPORTED

    def wgrad(x=a, cop=128, cip=128, cout=128, slope=0.2, nbytes=1 << 30):
        return L.sisr_wgrad1_mfma_leaky(x, a, a, a, a, a, 2, 8, 8, cout, 128, cop, cip, a, nbytes, slope, None)

    assert wgrad(x=None) == ARG and wgrad(slope=nan) == ARG and wgrad(cout=0) == ARG and wgrad(nbytes=16) == ARG
    assert wgrad(cop=48) == UNSUPPORTED and wgrad(cip=256) == UNSUPPORTED and wgrad(cop=64, cout=65) == UNSUPPORTED
    assert L.sisr_wgrad1_mfma_workspace_bytes(2, 8, 8, 128, 96) == 0
    # 2 x 8 rows -> 4 slices of 128 x 128 partial weights; per image 32 column-sum parts (64 pixels, 2 at a time) + the sum
    assert L.sisr_wgrad1_mfma_workspace_bytes(2, 8, 8, 128, 128) == 4 * (4 * 128 * 128 + (32 + 1) * 2 * 128)
    # the K x K entry points keep their two widths
    assert L.sisr_convk_mfma_leaky(a, None, a, a, 64, a, 1, 8, 8, 5, 64, 128, 1, 0.2, None) == UNSUPPORTED
    assert L.sisr_pack_convk(a, a, a, 1, 128, 64, 128, 64, None) == UNSUPPORTED


@pytest.mark.parametrize("num_features, M", [(64, 12), (48, 1)])
def test_the_folded_first_head_layer_is_exact_algebra(num_features, M):
    """float64: the twin with a real torch.cat equals the per-image-bias form to 1e-12, output and every gradient"""
    cfg = dict(num_codes=M, num_features=num_features)
    sd = T.kaiming_state(T.Twin(**cfg), 201)
    g = torch.Generator().manual_seed(202)
    x, codes = torch.rand((2, 3, 20, 28), generator=g).double(), torch.rand((2, M), generator=g).double()
    cot = torch.randn((2, M), generator=g).double()
    got = []
    for fold in (False, True):
        net, c = T.twin(sd, **cfg), codes.clone().requires_grad_(True)
        out = net(x, c, fold=fold)
        out.backward(cot)
        got.append([out.detach(), c.grad] + [p.grad for p in net.parameters()])
    assert float(got[0][0].abs().mean()) > 1e-3
    for a, b in zip(*got):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))


def test_corrector_has_the_parameters_of_the_concatenated_net():
    net = sisr_amd.corrector.DegradationCorrector(num_codes=12)
    want = {k: tuple(v.shape) for k, v in T.Twin(num_codes=12).state_dict().items()}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want
    assert want["head_dict.conv_0.weight"] == (128, 128, 1, 1) and want["code_dict.linear_0.weight"] == (64, 12)
    assert net.strides == [1, 1, 2, 1, 2] and [m.stride for m in net.layer_dict.children()] == [(s, s) for s in net.strides]
    assert sisr_amd.corrector.DegradationCorrector(num_layers=3).strides == [1, 1, 1]
    assert sisr_amd.corrector.DegradationCorrector(num_layers=2, strides=[2, 1]).strides == [2, 1]


@pytest.mark.parametrize("kwargs, limit", [
    (dict(num_codes=65), "num_codes"), (dict(num_codes=0), "num_codes"), (dict(num_features=65), "num_features"),
    (dict(kernel_size=4), "kernel_size"), (dict(kernel_size=11), "kernel_size"), (dict(in_channels=33), "in_channels"),
    (dict(strides=[1, 1, 2]), "strides"), (dict(strides=[1, 1, 3, 1, 2]), "strides"), (dict(num_layers=0), "num_layers")])
def test_corrector_refuses_what_it_cannot_run(kwargs, limit):
    with pytest.raises(NotImplementedError, match=limit):
        sisr_amd.corrector.DegradationCorrector(**kwargs)


def test_corrector_refuses_cpu_tensors_and_wrong_shapes():
    net = sisr_amd.corrector.DegradationCorrector(num_codes=4, num_features=32)
    with pytest.raises(RuntimeError, match="only runs on a HIP device"):
        net(torch.zeros(2, 3, 8, 8), torch.zeros(2, 4))


# ----------------------------------------------------------------------------- the handler (construction needs no GPU)
def _qrcan(metadata):
    return {"name": "qrcan", "internal_params": {"scale": 4, "style": "standard", "include_q_layer": True, "n_resgroups": 1,
                                                 "n_resblocks": 1, "metadata": list(metadata)}}


def _corrector(tmp_path, **extra):
    kw = dict(metadata=list(P.KEYS), num_features=32, sr_model=["q", 0], iterations=2)
    kw.update(extra)
    return sisr_amd.available_models["corrector"](device="cpu", model_save_dir=os.path.join(str(tmp_path), "c", "saved_models"),
                                                  eval_mode=True, **kw)


def test_registry_key_and_handler_attributes(tmp_path):
    P.save_experiment(sisr_amd, tmp_path, "q", _qrcan(P.KEYS), gpu=False)
    h = _corrector(tmp_path)
    assert h.predicts_metadata is True and h.num_metadata == 12 and h.metadata == P.KEYS and h.iterations == 2
    assert h.im_input == "unmodified" and h.colorspace == "rgb" and h.model_name == "corrector"
    assert isinstance(h.criterion, sisr_amd.basic.MSELoss) and isinstance(h.net, sisr_amd.corrector.DegradationCorrector)
    assert h.frozen["predictor"] is None and h.frozen["sr_model"].name == "qrcan"
    assert not any(p.requires_grad for p in h.frozen["sr_model"].model.parameters())
    assert set(h.state_dict()) == {"net." + k for k in h.net.state_dict()}
    assert torch.equal(h.initial_codes(torch.zeros(3, 3, 4, 4)), torch.full((3, 12), 0.5))  # the mean code
    assert _corrector(tmp_path, model_loc=str(tmp_path), iterations=7).iterations == 7


def test_handler_refuses_what_the_loop_cannot_use(tmp_path):
    P.save_experiment(sisr_amd, tmp_path, "q", _qrcan(P.KEYS), gpu=False)
    P.save_experiment(sisr_amd, tmp_path, "other", _qrcan(["blur_kernel", "jpeg_quality", "noise"]), gpu=False)
    P.save_experiment(sisr_amd, tmp_path, "plain", {"name": "edsr", "internal_params": {"scale": 4, "num_blocks": 1}}, gpu=False)
    with pytest.raises(ValueError) as err:
        _corrector(tmp_path, sr_model=["other", 0])
    assert "sr_model 'other' reads the metadata ['blur_kernel', 'jpeg_quality', 'noise']" in str(err.value)
    assert str(P.KEYS) in str(err.value) and "in the same order" in str(err.value)
    with pytest.raises(ValueError, match="reads no degradation code"):
        _corrector(tmp_path, sr_model=["plain", 0])
    with pytest.raises(ValueError, match="predicts no degradation code"):
        _corrector(tmp_path, predictor=["q", 0])
    with pytest.raises(ValueError, match="sr_model = .experiment, epoch. names the SR network"):
        _corrector(tmp_path, sr_model=None)
    with pytest.raises(ValueError, match="iterations must be at least 1"):
        _corrector(tmp_path, iterations=0)
    with pytest.raises(NotImplementedError, match="perceptual"):
        _corrector(tmp_path, perceptual=0.1)


def test_eval_sisr_refuses_ikc_without_metadata_predictor():
    with pytest.raises(ValueError, match="ikc: the loop corrects the code of metadata_predictor"):
        sisr_amd.cli._load_corrector({"ikc": {"corrector": ["c", 0]}}, None)
    assert sisr_amd.cli._load_corrector({}, None) == (None, 0)
