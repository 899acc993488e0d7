#!/usr/bin/env python
"""tests/golden/two_layer_train_vs_reference.npz: one forward of the REFERENCE's own AnimatingSoftmaxSplatingJoint
(models/animating_softmax_splating_2layers_alpha_seperate.py:256-809) in train() mode, float32 on the CPU, under the options of
train_animating_scripts/train_alpha_finetuneBG_finetuneFluid_v2.sh (softmax_splating_2layers_alpha_seperate, the resnet_256W8UpDown64
encoder / pconv2 decoder, the ...64Layers alpha networks, the ...64BG background network, pconv_pbn_woresbias, --norm_G
sync:spectral_batch, --train_Z, --train_bg, --train_alpha, --use_reweight_mask_loss, ATVloss 1, ADCloss 1, AlphaMSEloss 1000, MVloss 1),
with MRADCloss 1 so that every alpha loss is recorded: batch 2, 32 x 32, ngf 16 (the splat runs at C = 17), get_resnet_arch patched to the
narrow widths below, the seeded VGG19 of tests/losses_fixture.py in torchvision's place (nothing is
downloaded).  Built the way tools/make_golden_train_step.py is: the softsplat kernel text compiled for the host by tools/make_golden.py's
cupy stand-in, ``.cuda()`` returning the CPU tensor marked as a device one.

Recorded (data only): the inputs, the model's initial state dict, the noise every noise layer drew at each of its calls, every entry of
the loss dictionary and of pred_dict, the buffers the forward changed (after it), the sorted state keys with shapes, and the names of
``model.parameters()`` in order.  Needs the reference checkout next to the repository (build container only)."""
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
from make_golden_train_step import UPDOWN, inputs  # noqa: E402

FEAT, W, BS = 16, 32, 2
ENC_WIDTHS, DEC_WIDTHS = [8, 8, 8, 8, 8, 8, 8], [8, 16, 16, 8, 8, 8, 8]      # five networks in one file of < 1 MB: narrower than the single-layer fixture's
OPTIONS = ("--model_type softmax_splating_2layers_alpha_seperate --refine_model_type resnet_256W8UpDown64_de_resnet_pconv2_nonorm "
           "--alpha_refine_model_type resnet_256W8UpDown64Layers_de_resnet_pconv2_nonorm --bg_refine_model_type resnet_256W8UpDown64BG_nonorm "
           "--pconv pconv_pbn_woresbias --norm_G sync:spectral_batch --normalize_image --train_Z --use_inverse_depth --accumulation wsum "
           f"--losses 1.0_l1 10.0_content --ngf {FEAT} --out_channel {FEAT + 1} --W {W} --ATVloss 1.0 --AKLloss 0.0 --ADCloss 1.0 "
           "--MRADCloss 1.0 --AlphaMSEloss 1000.0 --use_reweight_mask_loss --train_bg --train_alpha --MVloss 1.0 --RockRegionlosstarget 0.25")


def arch(model_type, opt, in_channels=3):
    """get_resnet_arch (models/networks/configs.py) with the narrow widths: the ...64Layers alpha networks end in opt.out_channel (2) and
    read ngf + addtional_decoder_input, the ...64BG network reads and writes an image, the main pair is tools/make_golden_train_step.py's."""
    if "Layers" in model_type:
        enc, dec = [in_channels] + ENC_WIDTHS + [opt.out_channel], [FEAT + opt.addtional_decoder_input] + DEC_WIDTHS + [3 + opt.addtional_decoder_output]
    elif "BG" in model_type:
        enc, dec = None, [3] + DEC_WIDTHS + [3]
    else:
        enc, dec = [in_channels] + ENC_WIDTHS + [FEAT], [FEAT] + DEC_WIDTHS + [3]
    out = dict(downsample=[False] * 8, layers_dec=dec, upsample=list(UPDOWN))
    if enc is not None:
        out["layers_enc"] = enc
    return out


def extra_inputs():
    """The mean video frame, and a rock mask: a disc and a band, so that both moving classes exist."""
    gen = torch.Generator().manual_seed(20241)
    images, motion, _ = inputs()
    mean_video = (images.mean(0) * 0.8 + 0.1 * torch.randn(BS, 3, W, W, generator=gen)).clamp(-1, 1)
    y, x = torch.meshgrid(torch.arange(W, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    rock = torch.stack([((x - 10) ** 2 + (y - 20) ** 2 < 49).float(), (y < 9).float()])[:, None]
    return mean_video.contiguous(), rock.contiguous()


def pack(g, group, tensors):
    """A dict of arrays as three entries: the names ('\\n'-joined), the shapes [n,4] (-1 padded) and every value as float32 in one flat
    array (counters are small integers) -- thousands of zip members cost more than their data.  tests/two_layer_f64.py::unpack reads it."""
    names = list(tensors)
    shapes = np.full((len(names), 4), -1, np.int64)
    for i, k in enumerate(names):
        shapes[i, :tensors[k].ndim] = list(tensors[k].shape)
    g[group + "_names"] = np.array("\n".join(names))
    g[group + "_shapes"] = shapes
    g[group + "_data"] = np.concatenate([np.asarray(tensors[k], dtype=np.float32).reshape(-1) for k in names]) if names else np.zeros(0, np.float32)


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
    base = BaseModel(model, opt)
    for p in patches:
        p.stop()
    g = {}
    with torch.no_grad():
        for k, p in model.named_parameters():
            if not k.startswith("loss_function"):
                p.copy_(p + 0.02 * torch.randn(p.shape))
    before = {}
    for k, v in model.state_dict().items():
        if not k.startswith("loss_function"):
            before[k] = v.detach().clone()
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
    g["images"], g["motions"], g["index"], g["mean_video"], g["mask_rock"] = (images.numpy(), motion.numpy(), index.numpy(),
                                                                              mean_video.numpy(), rock.numpy())
    pack(g, "sd", {k: v.numpy() for k, v in before.items()})
    pack(g, "noise", {f"{k}/{j}": t.numpy() for k, calls in seen.items() for j, t in enumerate(calls)})
    g["loss_keys"] = np.array("\n".join(loss.keys()))
    for k, v in loss.items():
        g["loss/" + k] = plain(v).astype(np.float32)
        print("loss", k, g["loss/" + k])
    g["pred_keys"] = np.array("\n".join(pred.keys()))
    for k, v in pred.items():
        g["pred/" + k] = plain(v).astype(np.float32)
    after = {k: plain(v) for k, v in model.state_dict().items() if k in before and not torch.equal(before[k], v.detach().as_subclass(torch.Tensor))}
    pack(g, "after", after)
    n_after = len(after)
    sd = base.state_dict()
    keys = sorted(sd.keys())
    g["state_keys"] = np.array("\n".join(keys))
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    g["state_shapes"] = shapes
    g["parameter_order"] = np.array("\n".join(k for k, _ in model.named_parameters()))
    g["parameter_learns"] = np.array([p.requires_grad for _, p in model.named_parameters()])
    print(len(keys), "state keys,", len(str(g["parameter_order"]).split("\n")), "parameters,", len(seen), "noise layers,", n_after, "buffers changed,",
          {k: len(v) for k, v in list(seen.items())[:2]}, "calls of the first noise layers")
    path = os.path.join(ROOT, "tests", "golden", "two_layer_train_vs_reference.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    import shutil
    try:
        main()
    finally:
        shutil.rmtree(MG.TMP, ignore_errors=True)
