#!/usr/bin/env python
"""tests/golden/metrics_vs_reference.npz: outputs of the REFERENCE's own metric functions on the seeded inputs of tests/metrics_fixture.py
-- models/losses/ssim.py:ssim (windows 11 and 7, both size_average values, with and without a mask), evaluation/animation/metrics.py
(psnr with and without a mask, perceptual_sim) and models/networks/pretrained_networks.py:PNet("vgg") per layer, its torchvision stubbed
so that models.vgg16() returns the seeded layer list of metrics_fixture.vgg16_features(); plus one fluid-mode case (eval_CLAW_fluid.py:
88-109 restated on the reference's read_flo).  CPU, fp32.  No weights, nothing of the reference's text.  Needs the reference checkout
(path: argv[1], default /root/reference)."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_fixture as MF  # noqa: E402


def _stubs():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = lambda pretrained=False, **kw: types.SimpleNamespace(features=MF.vgg16_features())
    tv.transforms = types.ModuleType("torchvision.transforms")             # (imported, unused, by utils/utils.py)
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tv.models)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    for name in ("cv2", "av", "lz4framed"):
        sys.modules.setdefault(name, types.ModuleType(name))


def main():
    sys.path.insert(0, REF)
    _stubs()
    torch.set_num_threads(16)
    from models.losses.ssim import ssim
    from evaluation.animation.metrics import psnr, perceptual_sim
    from models.networks.pretrained_networks import PNet
    from utils.utils import read_flo
    g = {}
    for H, W in MF.SIZES:
        a_u8, b_u8 = MF.image_pair(H, W)
        a, b = MF.to_tensor(a_u8), MF.to_tensor(b_u8)
        mask = torch.from_numpy(MF.mask_for(H, W))
        t = f"{H}x{W}"
        for ws in MF.WINDOWS:
            g[f"{t}_w{ws}_ssim_mean"] = ssim(a, b, ws, None, True).numpy()
            g[f"{t}_w{ws}_ssim"] = ssim(a, b, ws, None, False).numpy()
            g[f"{t}_w{ws}_ssim_mask"] = ssim(a, b, ws, mask, True).numpy()
            g[f"{t}_w{ws}_ssim_mask_noavg"] = ssim(a, b, ws, mask, False).numpy()
        g[f"{t}_psnr"] = psnr(a, b).numpy()
        g[f"{t}_psnr_mask"] = psnr(a, b, mask).numpy()
        print(t, "ssim", g[f"{t}_w11_ssim"], "psnr", g[f"{t}_psnr"])
    pnet = PNet("vgg", use_gpu=False).eval()
    for H, W in MF.VGG_SIZES:
        a_u8, b_u8 = MF.image_pair(H, W, tag="vgg")
        a, b = MF.to_tensor(a_u8), MF.to_tensor(b_u8)
        with torch.no_grad():
            total, per = pnet(a * 2 - 1, b * 2 - 1, retPerLayer=True)
            again = perceptual_sim(a, b, pnet)
        assert torch.equal(total, again)
        g[f"{H}x{W}_perceptual"] = total.numpy()
        g[f"{H}x{W}_perceptual_layers"] = torch.stack(per).numpy()
        print(H, W, "perceptual", total.numpy(), "layers", torch.stack(per)[:, 0].numpy())
    # fluid mode, eval_CLAW_fluid.py:88-109 with the reference's own read_flo
    flow_hw2, image, pred = MF.fluid_inputs()
    import tempfile
    from PIL import Image
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "scene.flo")
        with open(p, "wb") as f:
            np.array([202021.25], np.float32).tofile(f)
            np.array([flow_hw2.shape[1], flow_hw2.shape[0]], np.int32).tofile(f)
            flow_hw2.tofile(f)
        ph, pw = MF.FLUID["pred_hw"]
        flow = torch.FloatTensor(read_flo(p)).unsqueeze(0)
        flow = F.interpolate(flow, (ph, pw), mode='bilinear').squeeze()
        motion_speed = (flow[0:1, :, :] ** 2 + flow[1:2, :, :] ** 2).sqrt()
        mask = (motion_speed > motion_speed.mean() * 0.1).float()
        img = Image.fromarray(image).resize((pw, ph), Image.BILINEAR)
        img = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)
        pred_t = torch.from_numpy(pred[0]).permute(2, 0, 1).float() / 255.0
        g["fluid_mask"] = mask.numpy()
        g["fluid_composite"] = (pred_t * mask + img * (1.0 - mask)).numpy()
    out = os.path.join(ROOT, "tests", "golden", "metrics_vs_reference.npz")
    np.savez_compressed(out, **g)
    print("wrote", out, os.path.getsize(out) // 1024, "kB")


if __name__ == "__main__":
    main()
