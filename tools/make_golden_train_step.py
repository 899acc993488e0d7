#!/usr/bin/env python
"""tests/golden/train_step_vs_reference.npz: one forward of the REFERENCE's own AnimatingSoftmaxSplating
(models/animating_softmax_splating.py:445-775) in train() mode, float32 on the CPU, under the options of
train_animating_scripts/train_baseline2_pconv.sh (softmax_splating, resnet_256W8UpDown64_de_resnet_pconv2_nonorm, pconv_pbn_woresbias,
--norm_G sync:spectral_batch, --train_Z, --normalize_image, --discriminator_losses pix2pixHD), at the shape of
tests/test_gpu_train_step.py: batch 2, 32 x 32, get_resnet_arch patched to the narrow widths of tests/test_gpu_spectral.py, ndf 8, the
seeded VGG19 of tests/losses_fixture.py in torchvision's place (nothing is downloaded).  Its softsplat kernel text is compiled for the
host by tools/make_golden.py's cupy stand-in; ``.cuda()`` returns the CPU tensor marked as a device one, as tools/make_golden_e2e.py does.

Recorded (data only): the inputs, the model's initial state dict, the noise every noise layer drew at each of its calls, every entry
of the loss dictionary, PredImg, Z_f, the sorted keys with shapes of ``BaseModel(model, opt).state_dict()``, and the names of
``model.parameters()`` in order (the indices of the reference's optimizerG state).
Needs the reference checkout next to the repository (build container only)."""
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

ENC_WIDTHS, DEC_WIDTHS = [8, 8, 8, 16, 16, 16, 16], [16, 24, 24, 16, 16, 16, 8]
UPDOWN = [False, "Down", "Down", False, "Up", "Up", False, False]
FEAT, W, BS, NDF = 16, 32, 2, 8
INDEX = [[0, 30, 59], [3, 10, 40]]                        # two different time pairs
ARCH = dict(layers_enc=[3] + ENC_WIDTHS + [FEAT], downsample=[False] * 8, layers_dec=[FEAT] + DEC_WIDTHS + [3], upsample=UPDOWN)
OPTIONS = ("--model_type softmax_splating --refine_model_type resnet_256W8UpDown64_de_resnet_pconv2_nonorm --pconv pconv_pbn_woresbias "
           "--norm_G sync:spectral_batch --normalize_image --train_Z --use_softmax_splatter --use_inverse_depth "
           f"--losses 1.0_l1 10.0_content --discriminator_losses pix2pixHD --ndf {NDF} --ngf {FEAT} --out_channel {FEAT} --W {W}")


def inputs():
    """Three images in [-1, 1] that share their low frequencies, a smooth motion field of a few pixels, the indices."""
    gen = torch.Generator().manual_seed(20240)
    y, x = torch.meshgrid(torch.arange(W, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([torch.sin(x / 5 + c + b) * torch.cos(y / 7 - c) for b in range(BS) for c in range(3)]).reshape(BS, 3, W, W)
    images = torch.stack([(0.7 * base + 0.25 * torch.randn(BS, 3, W, W, generator=gen)).clamp(-1, 1) for _ in range(3)])
    motion = torch.stack([0.08 * torch.sin(y / 6 + x / 11), 0.06 * torch.cos(x / 5 - y / 9)])[None].repeat(BS, 1, 1, 1)
    motion = motion * torch.tensor([1.0, -0.7]).view(BS, 1, 1, 1)
    return images, motion.contiguous(), torch.tensor(INDEX, dtype=torch.int64)


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
    torch.cuda.is_available = lambda: True               # (get_loss_from_name returns a loss only then; forward() calls .cuda() then)
    torch.Tensor.cuda = lambda self, *a, **k: self.as_subclass(MG.CudaLike)
    nn.Module.cuda = lambda self, device=None: self
    torch.set_num_threads(16)
    from models.base_model import BaseModel
    from models.networks import architectures, configs
    from options.train_options import ArgumentParser
    import models.animating_softmax_splating as A

    opt, _ = ArgumentParser().parse(OPTIONS)
    opt.isTrain = True
    opt.beta1, opt.beta2 = float(opt.beta1), float(opt.beta2)      # (argparse leaves the default 0 an int, which today's torch.optim.Adam refuses)
    torch.manual_seed(7)
    patches = [mock.patch.object(mod, "get_resnet_arch", lambda *a, **k: dict(ARCH)) for mod in (architectures, configs)
               if hasattr(mod, "get_resnet_arch")]
    for p in patches:
        p.start()
    model = A.AnimatingSoftmaxSplating(opt).train()
    base = BaseModel(model, opt)
    for p in patches:
        p.stop()
    g = {}
    with torch.no_grad():                                # float32 values a little away from the initialisation's symmetry
        for k, p in model.named_parameters():
            if not k.startswith("loss_function"):
                p.copy_(p + 0.02 * torch.randn(p.shape))
    for k, v in model.state_dict().items():
        if not k.startswith("loss_function"):            # (the VGG19 is tests/losses_fixture.py's: regenerated, not stored)
            g["sd/" + k] = v.detach().clone().numpy()
    seen = {}
    for k, m in model.named_modules():
        if hasattr(m, "gain") and hasattr(m, "bias") and isinstance(getattr(m, "gain"), nn.Linear):
            m.gain.register_forward_hook(lambda mod, a, o, k=k: seen.setdefault(k, []).append(a[0].detach().as_subclass(torch.Tensor).clone()))
    images, motion, index = inputs()
    batch = {"images": [images[0], images[1], images[2]], "motions": motion.as_subclass(MG.CudaLike), "index": index}
    with torch.no_grad():                                # (values only; today's autograd also refuses the forward's in-place adds on views of a custom Function's output)
        loss, pred = model(batch)
    plain = lambda t: t.detach().as_subclass(torch.Tensor).numpy()            # noqa: E731
    g["images"], g["motions"], g["index"] = images.numpy(), motion.numpy(), index.numpy()
    for k, calls in seen.items():
        for j, t in enumerate(calls):
            g[f"noise/{k}/{j}"] = t.numpy()
    g["loss_keys"] = np.array(sorted(loss.keys()))
    for k, v in loss.items():
        g["loss/" + k] = plain(v).astype(np.float32)
        print("loss", k, g["loss/" + k])
    g["PredImg"], g["Z_f"] = plain(pred["PredImg"]), plain(pred["Z_f"])
    g["pred_keys"] = np.array(sorted(pred.keys()))
    sd = base.state_dict()
    keys = sorted(sd.keys())
    g["state_keys"] = np.array(keys)
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    g["state_shapes"] = shapes
    g["parameter_order"] = np.array([k for k, _ in model.named_parameters()])
    g["parameter_learns"] = np.array([p.requires_grad for _, p in model.named_parameters()])
    g["netD_parameter_order"] = np.array([k for k, _ in base.netD.named_parameters()])
    print("PredImg", g["PredImg"].shape, "range", g["PredImg"].min(), g["PredImg"].max(), "Z_f range", g["Z_f"].min(), g["Z_f"].max())
    print(len(keys), "state keys,", len(g["parameter_order"]), "parameters,", len(seen), "noise layers")
    path = os.path.join(ROOT, "tests", "golden", "train_step_vs_reference.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    import shutil
    try:
        main()
    finally:
        shutil.rmtree(MG.TMP, ignore_errors=True)
