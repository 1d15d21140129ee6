#!/usr/bin/env python3
"""SRCNN / VDSR golden vectors, produced by RUNNING THE REFERENCE on CPU (build container only).

    python tools/make_fixtures_basic.py

b1  default SRCNN and a reduced VDSR ([3]*4, [1,64,64,64,1]) on a (2,1,13,22) input: output, cotangent, every parameter
    gradient, state dict; the meta holds the fixture's own distance from a float64 evaluation of the same net
    (max |output error|, relative norm error per gradient)
b2  full-depth seed-8 key list / parameter count / SHA-256 of both models; the five Set5 images: LR from tests/golden/set5,
    PIL-bicubic-upsampled x4 (ref: SISR/evaluation/standard_eval.py:146-158), converted with the reference's converter,
    through the reference handlers' run_eval on Y: per-image Y-PSNR, MSE loss, 32x32 centre crops
b3  five run_train steps per handler (Adam 1e-4; VDSR with its gradient clip) on seeded torch.rand (2,1,24,24) batches:
    per-step loss, post-clip gradient norm, output mean, learning rate; the final parameter sum
b4  one epoch of the reference's own train loop (TrainingHandler, as train_sisr drives it) with srcnn on the Set5 images,
    the LR images written bicubic-upsampled x4 to a temporary folder (input = 'interp'); stored like g5_train_sisr.json
    (python tools/make_fixtures_basic.py b4 regenerates this alone)
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as MF  # noqa: E402  (installs the import shim, imports the reference)

from PIL import Image  # noqa: E402
from SISR.models import ModelInterface  # noqa: E402
from SISR.models.basic import architectures as A  # noqa: E402
from sr_tools.image_manipulation import ycbcr_convert  # noqa: E402
from sr_tools.metrics import psnr as ref_psnr  # noqa: E402

OUT, _np = MF.OUT, MF._np
SET5 = os.path.join(OUT, "set5")
REDUCED_VDSR = {"kernel_pattern": [3] * 4, "channel_pattern": [1, 64, 64, 64, 1]}
NETS = {"b1_srcnn": (A.SRCNN, {}), "b1_vdsr_reduced": (A.VDSR, REDUCED_VDSR)}


def make_b1():
    for name, (cls, cfg) in NETS.items():
        torch.manual_seed(8)
        net = cls(**cfg)
        x = torch.rand(2, 1, 13, 22, generator=torch.Generator().manual_seed(81))
        out = net(x)
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(82))
        out.backward(cot)
        net64 = copy.deepcopy(net).double()
        net64.zero_grad()
        out64 = net64(x.double())
        out64.backward(cot.double())
        g64 = dict(net64.named_parameters())
        meta = dict(cfg, out_err_max=float((out.detach().double() - out64.detach()).abs().max()),
                    grad_rel_err={k: float((p.grad.double() - g64[k].grad).norm() / g64[k].grad.norm())
                                  for k, p in net.named_parameters()})
        blob = {"in0": _np(x), "out": _np(out), "cot": _np(cot), "meta": np.array(json.dumps(meta))}
        for k, v in net.state_dict().items():
            blob["sd/" + k] = _np(v)
        for k, p in net.named_parameters():
            blob["pg/" + k] = _np(p.grad)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **blob)
        print(f"{name:18s} {os.path.getsize(path) / 1e3:7.1f} KB out err {meta['out_err_max']:.2e} "
              f"grad err {max(meta['grad_rel_err'].values()):.2e}")


def interp_ycbcr(name, scale=4):
    """(LR bicubic-upsampled x scale, HR), both converted to 3-channel YCbCr ('jpg' form) -> float32 (1,3,H,W) tensors"""
    lr = Image.open(os.path.join(SET5, "lr_random_blur", name)).convert("RGB")
    hr = Image.open(os.path.join(SET5, "hr", name)).convert("RGB")
    up = lr.resize((lr.width * scale, lr.height * scale), resample=Image.BICUBIC)
    conv = []
    for im in (up, hr):
        t = torch.from_numpy(np.asarray(im).transpose(2, 0, 1).copy()).float().div(255)
        conv.append(ycbcr_convert(t, im_type="jpg", input="rgb", y_only=False)[None])
    return conv


def make_b2(model_name):
    torch.manual_seed(8)
    model = ModelInterface.define_model(model_name, device=torch.device("cpu"), model_save_dir="/tmp", eval_mode=True)
    sd = model.net.state_dict()
    entry = {"sha256": MF.sd_digest(sd), "n_tensors": len(sd), "n_params": int(sum(p.numel() for p in model.net.parameters())),
             "keys": list(sd), "colorspace": model.colorspace, "im_input": model.im_input, "images": {}}
    crops = {}
    for im_name in sorted(f for f in os.listdir(os.path.join(SET5, "hr")) if f.endswith(".png")):
        x, y = interp_ycbcr(im_name)
        out, loss, _ = model.run_eval(x[:, :1], y[:, :1], request_loss=True)
        o = out.numpy()[0]
        p = float(ref_psnr(np.clip(o[0], 0, 1), y.numpy()[0, 0], max_value=1))
        entry["images"][im_name] = {"mean": float(o.mean()), "std": float(o.std()), "mse": float(loss), "y_psnr": p}
        hh, ww = o.shape[1:]
        crops[im_name] = o[:, hh // 2 - 16:hh // 2 + 16, ww // 2 - 16:ww // 2 + 16].copy()
        print(f"b2 {model_name} {im_name:14s} psnr={p:.4f} mse={float(loss):.6f}")
    np.savez_compressed(os.path.join(OUT, f"b2_{model_name}_crops.npz"), **crops)
    return entry


def make_b3(model_name):
    torch.manual_seed(8)
    model = ModelInterface.define_model(model_name, device=torch.device("cpu"), model_save_dir="/tmp", eval_mode=False, lr=1e-4)
    g = torch.Generator().manual_seed(83)
    steps = []
    for it in range(5):
        x = torch.rand(2, 1, 24, 24, generator=g)
        y = torch.rand(2, 1, 24, 24, generator=g)
        loss, o = model.run_train(x, y)
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.net.parameters())))
        steps.append({"loss": float(loss), "grad_norm": gn, "out_mean": float(o.mean()), "lr": model.get_learning_rate()})
        print(f"b3 {model_name} step {it} loss={float(loss):.6f} gn={gn:.5f}")
    return {"steps": steps, "grad_clip": model.grad_clip,
            "final_param_sum": float(sum(v.double().sum() for v in model.net.state_dict().values()))}


def write_interp(folder, scale=4):
    """the stored Set5 LR images, PIL-bicubic-upsampled x scale, as PNGs under `folder` (what input = 'interp' reads)"""
    os.makedirs(folder, exist_ok=True)
    for f in sorted(os.listdir(os.path.join(SET5, "lr_random_blur"))):
        if f.endswith(".png"):
            lr = Image.open(os.path.join(SET5, "lr_random_blur", f)).convert("RGB")
            lr.resize((lr.width * scale, lr.height * scale), resample=Image.BICUBIC).save(os.path.join(folder, f))


def make_b4():
    import tempfile
    import pandas as pd
    from SISR.training.training_handler import TrainingHandler
    from sr_tools.helper_functions import convert_default_none_dict
    tmp = tempfile.mkdtemp()
    write_interp(os.path.join(tmp, "interp"))
    # cutoff keeps the splits 'train' / 'eval' (an unnamed set without it counts as 'all', hence Y only, in both)
    ds = {"name": None, "lr": os.path.join(tmp, "interp"), "hr": os.path.join(SET5, "hr"), "cutoff": 5}
    params = {
        "experiment": "b4_srcnn", "experiment_save_loc": tmp,
        "data": {"batch_size": 2, "dataloader_threads": 0,
                 "training_sets": {"data_1": dict(ds, crop=32, random_augment=True)},
                 "eval_sets": {"data_1": dict(ds)}},
        "model": {"name": "srcnn", "internal_params": {"scale": 1, "lr": 1e-4}},  # interp images: LR and HR of one size
        "training": {"gpu": "off", "seed": 8, "num_epochs": 1, "metrics": ["PSNR"], "logging": "text", "save_samples": False},
    }
    cfg = json.loads(json.dumps(params))
    p = convert_default_none_dict(params)
    exp = TrainingHandler(experiment_name=p["experiment"], save_loc=p["experiment_save_loc"], model_params=p["model"],
                          **p["training"], data_params={**p["data"]})
    exp.run_experiment()
    summ = pd.read_csv(os.path.join(exp.model.logs, "summary.csv"))
    out = {"srcnn": {"config": cfg, "summary": {k: [float(v) for v in summ[k]] for k in summ.columns}}}
    for part in ("training_sets", "eval_sets"):  # paths in the stored config are rewritten by the tests
        for d in out["srcnn"]["config"]["data"][part].values():
            d["lr"], d["hr"] = "INTERP", "SET5/hr"
    out["srcnn"]["config"]["experiment_save_loc"] = "TMP"
    print("b4", out["srcnn"]["summary"])
    with open(os.path.join(OUT, "b4_train_sisr.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1:] == ["b4"]:
        make_b4()
        sys.exit(0)
    make_b1()
    doc = {"full_depth": {m: make_b2(m) for m in ("srcnn", "vdsr")}, "train_steps": {m: make_b3(m) for m in ("srcnn", "vdsr")}}
    with open(os.path.join(OUT, "b_basic.json"), "w") as f:
        json.dump(doc, f, indent=1)
    make_b4()
