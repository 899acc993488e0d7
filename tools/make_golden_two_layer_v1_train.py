#!/usr/bin/env python
"""tests/golden/two_layer_v1_train_vs_reference.npz: one forward of the REFERENCE's own AnimatingSoftmaxSplatingJoint
(models/animating_softmax_splating_2layers_alpha_seperate.py:256-809) in train() mode, float32 on the CPU, under the options of
train_animating_scripts/train_alpha_finetuneBG_finetuneFluid_v1.sh (--use_alpha0_as_blending_weight, ATVloss 0.3, ADCloss 1,
FluidRegionloss 3, RockRegionloss 30, RockRegionlosstarget 0.25, MVloss 1, no AlphaMSEloss), with MRADCloss 1 so that every term is
recorded.  Everything else is tools/make_golden_two_layer_train.py's: batch 2, 32 x 32, ngf 16, the same narrow widths, seed, inputs and
stand-ins -- so the model's initial state dict, its inputs and the noise its layers draw are those of
tests/golden/two_layer_train_vs_reference.npz (asserted here), and this file records only what differs: every entry of the loss dictionary
and of pred_dict and the buffers the forward changed.  Data only, under 1 MB.  tests/two_layer_v1_f64.py::load reads the two files
together.  Needs the reference checkout next to the repository (build container only)."""
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
import losses_fixture as LF  # noqa: E402
import make_golden as MG  # noqa: E402
import two_layer_f64 as D  # noqa: E402
from make_golden_train_step import inputs  # noqa: E402
from make_golden_two_layer_train import FEAT, W, arch, extra_inputs, pack  # noqa: E402

OPTIONS = ("--model_type softmax_splating_2layers_alpha_seperate --refine_model_type resnet_256W8UpDown64_de_resnet_pconv2_nonorm "
           "--alpha_refine_model_type resnet_256W8UpDown64Layers_de_resnet_pconv2_nonorm --bg_refine_model_type resnet_256W8UpDown64BG_nonorm "
           "--pconv pconv_pbn_woresbias --norm_G sync:spectral_batch --normalize_image --train_Z --use_inverse_depth --accumulation wsum "
           f"--losses 1.0_l1 10.0_content --ngf {FEAT} --out_channel {FEAT + 1} --W {W} --ATVloss 0.3 --AKLloss 0.0 --ADCloss 1.0 "
           "--FluidRegionloss 3 --balanced_weight 10 --RockRegionloss 30 --RockRegionlossDecay 20 --MRADCloss 1.0 --train_bg --train_alpha "
           "--MVloss 1.0 --RockRegionlosstarget 0.25 --use_alpha0_as_blending_weight")


def main():
    ss, eim = MG.load_reference()
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg19 = lambda pretrained=False, **kw: types.SimpleNamespace(features=LF.vgg19_features())
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.utils = types.ModuleType("torchvision.utils")
    for name, m in (("torchvision", tv), ("torchvision.models", tv.models), ("torchvision.transforms", tv.transforms),
                    ("torchvision.utils", tv.utils), ("cv2", types.ModuleType("cv2")), ("av", types.ModuleType("av")),
                    ("lz4framed", types.ModuleType("lz4framed"))):
        sys.modules.setdefault(name, m)
    torch.cuda.is_available = lambda: True
    torch.Tensor.cuda = lambda self, *a, **k: self.as_subclass(MG.CudaLike)
    nn.Module.cuda = lambda self, device=None: self
    torch.set_num_threads(16)
    from models.base_model import BaseModel
    from models.networks import architectures, configs
    from options.train_options import ArgumentParser
    import models.animating_softmax_splating_2layers_alpha_seperate as A

    opt, _ = ArgumentParser().parse(OPTIONS)
    opt.isTrain = True
    opt.beta1, opt.beta2 = float(opt.beta1), float(opt.beta2)
    opt.discriminator_losses = "0" if not getattr(opt, "discriminator_losses", None) else opt.discriminator_losses
    torch.manual_seed(9)
    patches = [mock.patch.object(mod, "get_resnet_arch", arch) for mod in (architectures, configs) if hasattr(mod, "get_resnet_arch")]
    for p in patches:
        p.start()
    model = A.AnimatingSoftmaxSplatingJoint(opt).train()
    BaseModel(model, opt)                                                      # (as the v2 maker: it draws from the generator)
    for p in patches:
        p.stop()
    with torch.no_grad():
        for k, p in model.named_parameters():
            if not k.startswith("loss_function"):
                p.copy_(p + 0.02 * torch.randn(p.shape))
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if not k.startswith("loss_function")}
    seen = {}
    for k, m in model.named_modules():
        if hasattr(m, "gain") and hasattr(m, "bias") and isinstance(getattr(m, "gain"), nn.Linear):
            m.gain.register_forward_hook(lambda mod, a, o, k=k: seen.setdefault(k, []).append(a[0].detach().as_subclass(torch.Tensor).clone()))
    images, motion, index = inputs()
    mean_video, rock = extra_inputs()
    batch = {"images": [images[0], images[1], images[2]], "mean_video": [mean_video], "motions": motion.as_subclass(MG.CudaLike),
             "mask_rock": rock, "index": index}
    with torch.no_grad():
        loss, pred = model(batch)
    plain = lambda t: t.detach().as_subclass(torch.Tensor).numpy()            # noqa: E731
    # the state, the inputs and the noise are the v2 fixture's: same seed, same construction, same order of draws
    v2 = D.load()
    for k, v in before.items():
        assert np.array_equal(v2["sd/" + k], v.numpy()), k
    for k, calls in seen.items():
        for j, t in enumerate(calls):
            assert np.array_equal(v2[f"noise/{k}/{j}"], t.numpy()), (k, j)
    assert len([k for k in v2 if k.startswith("sd/")]) == len(before)
    assert len([k for k in v2 if k.startswith("noise/")]) == sum(len(c) for c in seen.values())
    for k, t in (("images", images), ("motions", motion), ("index", index), ("mean_video", mean_video), ("mask_rock", rock)):
        assert np.array_equal(v2[k], t.numpy()), k
    g = {"loss_keys": np.array("\n".join(loss.keys())), "pred_keys": np.array("\n".join(pred.keys())), "options": np.array(OPTIONS)}
    for k, v in loss.items():
        g["loss/" + k] = plain(v).astype(np.float32)
        print("loss", k, g["loss/" + k])
    for k, v in pred.items():
        g["pred/" + k] = plain(v).astype(np.float32)
    after = {k: plain(v) for k, v in model.state_dict().items() if k in before and not torch.equal(before[k], v.detach().as_subclass(torch.Tensor))}
    pack(g, "after", after)
    print(len(after), "buffers changed")
    path = os.path.join(ROOT, "tests", "golden", "two_layer_v1_train_vs_reference.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    import shutil
    try:
        main()
    finally:
        shutil.rmtree(MG.TMP, ignore_errors=True)
