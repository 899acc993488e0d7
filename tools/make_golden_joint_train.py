#!/usr/bin/env python
"""tests/golden/joint_train_vs_reference.npz: one forward of the REFERENCE's own AnimatingSoftmaxSplating with --train_motion
(models/animating_softmax_splating.py:189-193, :514-536, :748-766) in train() mode, float32 on the CPU, at 256 x 256, batch 1, index
triple [3, 10, 40]: the flags of tests/joint_train_fixture.py (the baseline's of tools/make_golden_train_step.py plus --train_motion
--motion_model_type SPADE_unet_mask_motion, --div_flow 2.0, --losses 1.0_l1, --motion_losses 10.0_EndPointError), get_resnet_arch
patched to the narrow widths of tools/make_golden_train_step.py, the motion predictor replaced by the reference's
SPADEUnet4MaskMotion(num_filters=8) as tools/make_golden_motion_train.py builds it.  State and batch come from
tests/joint_train_fixture.py; the softsplat kernel text is compiled for the host by tools/make_golden.py's cupy stand-in.

Recorded (data only): every loss entry; the flow the model hands to its Euler integration, whole; the noise every noise layer drew;
PredImg, PredMotion and the moved weight_u / weight_v of the motion network at digest positions with each tensor's max|.|; the sorted
keys with shapes of ``BaseModel(model, opt).state_dict()``; the names of ``model.parameters()`` in order with requires_grad, before
and after the freeze of train_animating_fixmotion.py:448-450.  Needs the reference checkout next to the repository (build container only)."""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import joint_train_fixture as JF  # noqa: E402
import make_golden as MG  # noqa: E402
from make_golden_train_step import ARCH  # noqa: E402


def main():
    MG.load_reference()
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg19 = None
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.utils = types.ModuleType("torchvision.utils")
    for name, m in (("torchvision", tv), ("torchvision.models", tv.models), ("torchvision.transforms", tv.transforms),
                    ("torchvision.utils", tv.utils), ("cv2", types.ModuleType("cv2")), ("av", types.ModuleType("av")),
                    ("lz4framed", types.ModuleType("lz4framed")), ("ipdb", types.ModuleType("ipdb"))):
        sys.modules.setdefault(name, m)
    torch.cuda.is_available = lambda: True               # (the loss modules are built only then; forward() calls .cuda() then)
    torch.Tensor.cuda = lambda self, *a, **k: self.as_subclass(MG.CudaLike)
    nn.Module.cuda = lambda self, device=None: self
    torch.set_num_threads(16)
    from models.base_model import BaseModel
    from models.networks import architectures, configs
    from models.networks.architectures import SPADEUnet4MaskMotion
    from options.train_options import ArgumentParser
    import models.animating_softmax_splating as A

    opt, _ = ArgumentParser().parse(JF.FLAGS)
    opt.isTrain = True
    opt.beta1, opt.beta2 = float(opt.beta1), float(opt.beta2)
    torch.manual_seed(7)
    patches = [mock.patch.object(mod, "get_resnet_arch", lambda *a, **k: dict(ARCH)) for mod in (architectures, configs)
               if hasattr(mod, "get_resnet_arch")]
    for p in patches:
        p.start()
    model = A.AnimatingSoftmaxSplating(opt)
    for p in patches:
        p.stop()
    model.motion_regressor.motion_predictor = SPADEUnet4MaskMotion(num_filters=JF.NF, channels_in=6, channels_out=2, opt=opt)
    model = model.train()
    base = BaseModel(model, opt)
    own = model.state_dict()
    sd = dict(JF.generator_state())
    sd.update({"motion_regressor.motion_predictor." + k: v for k, v in JF.motion_state().items()})
    missing, extra = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    assert not missing and not extra, (missing[:5], extra[:5])
    model.load_state_dict({k: sd[k].reshape(own[k].shape) for k in own})

    g = {}
    seen, flows = {}, []
    for k, m in model.named_modules():
        if hasattr(m, "gain") and hasattr(m, "bias") and isinstance(getattr(m, "gain"), nn.Linear):
            m.gain.register_forward_hook(lambda mod, a, o, k=k: seen.setdefault(k, []).append(a[0].detach().as_subclass(torch.Tensor).clone()))
    model.euler_integration.register_forward_pre_hook(lambda mod, a: flows.append(a[0].detach().as_subclass(torch.Tensor).clone()))
    b = JF.batch()
    batch = {"images": list(b["images"]), "motions": b["motions"].as_subclass(MG.CudaLike), "hints": b["hints"], "index": b["index"]}
    with torch.no_grad():                                # (values only, as tools/make_golden_train_step.py)
        loss, pred = model(batch)
    plain = lambda t: t.detach().as_subclass(torch.Tensor)            # noqa: E731

    def digest(name, t):
        flat = plain(t).double().reshape(-1)
        g[name + "#samples"] = flat[JF.positions(name, flat.numel())].numpy()
        g[name + "#max_abs"] = np.float64(flat.abs().max())
    g["flow"] = flows[0].numpy().astype(np.float32)
    assert len(flows) == 2 and torch.equal(flows[1], -flows[0])
    for k, calls in seen.items():
        for j, t in enumerate(calls):
            g[f"noise/{k}/{j}"] = t.numpy()
    g["loss_keys"] = np.array(list(loss.keys()))
    for k, v in loss.items():
        g["loss/" + k] = plain(v).double().numpy()
        print("loss", k, float(g["loss/" + k]))
    g["pred_keys"] = np.array(sorted(pred.keys()))
    digest("PredImg", pred["PredImg"])
    digest("PredMotion", pred["PredMotion"])
    g["GTMotion_is_the_batch"] = np.bool_(torch.equal(plain(pred["GTMotion"]), b["motions"]))
    after = model.motion_regressor.motion_predictor.state_dict()
    for k in after:
        if k.endswith("weight_u") or k.endswith("weight_v"):
            g["after/" + k] = after[k].detach().numpy().astype(np.float64)
    sdb = base.state_dict()
    keys = sorted(sdb.keys())
    g["state_keys"] = np.array(keys)
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sdb[k].dim()] = list(sdb[k].shape)
    g["state_shapes"] = shapes
    g["parameter_order"] = np.array([k for k, _ in model.named_parameters()])
    g["parameter_learns"] = np.array([p.requires_grad for _, p in model.named_parameters()])
    for name, param in base.named_parameters():          # train_animating_fixmotion.py:448-450
        if "motion_predictor" in name:
            param.requires_grad = False
    g["parameter_learns_frozen"] = np.array([p.requires_grad for _, p in model.named_parameters()])
    from oracle import oracle as O
    O.build()
    n_f, n_p = JF.INDEX[0][1] - JF.INDEX[0][0], JF.INDEX[0][2] + 1 - JF.INDEX[0][1]
    valid = (float(O.euler_integration(g["flow"], n_f)[1].mean()), float(O.euler_integration(-g["flow"], n_p)[1].mean()))
    g["valid_fraction"] = np.array(valid)
    print("flow max", float(np.abs(g["flow"]).max()), "valid", valid, "PredImg max", float(g["PredImg#max_abs"]))
    print(len(keys), "state keys,", len(g["parameter_order"]), "parameters,", int(g["parameter_learns_frozen"].sum()), "learn when frozen,",
          len(seen), "noise layers")
    np.savez_compressed(JF.GOLDEN, **g)
    print("wrote", JF.GOLDEN, os.path.getsize(JF.GOLDEN) // 1024, "kB")


if __name__ == "__main__":
    import shutil
    sys.path.insert(0, ROOT)
    try:
        main()
    finally:
        shutil.rmtree(MG.TMP, ignore_errors=True)
