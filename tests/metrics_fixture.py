"""Inputs and VGG16 weights of tests/golden/metrics_vs_reference.npz, and a float64 torch restatement of the three metrics.

Like tests/nets_fixture.py: the VGG16 weights are DEFINED here from their key names (torchvision's features.{i}.weight / .bias) and a
seed, so only the reference's outputs are committed.  tools/make_golden_metrics.py (needs the reference checkout) runs the reference's
models/losses/ssim.py, evaluation/animation/metrics.py and PNet("vgg") (its torchvision.models.vgg16 stubbed to return
vgg16_features()) on the seeded inputs below.  The float64 restatement (ssim_f64, psnr_f64, perceptual_f64) is the yardstick of the GPU
tests at sizes the file does not hold.  Test infrastructure only."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from nets_fixture import _rng

VGG16_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")   # torchvision cfg "D"
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))                  # pretrained_networks.py:209-218
SHIFT = (-0.030, -0.088, -0.188)                                        # pretrained_networks.py:45-46
SCALE = (0.458, 0.448, 0.450)
SIZES = ((5, 7), (37, 61), (64, 96))                                    # SSIM / PSNR cases (5 x 7: smaller than the window)
VGG_SIZES = ((64, 96), (72, 100))                                       # Perceptual cases (72 x 100: odd pooled sizes)
WINDOWS = (11, 7)
N = 3
FLUID = {"flow_hw": (9, 13), "image_hw": (20, 30), "pred_hw": (24, 40)}


def vgg16_state_dict():
    """torchvision-format VGG16 feature weights, every value a function of its key (He-scaled normal weights, small biases)."""
    sd, cin, idx = {}, 3, 0
    for v in VGG16_CFG:
        if v == "M":
            idx += 1
            continue
        w = _rng("vgg16", f"features.{idx}.weight").standard_normal((v, cin, 3, 3)) * math.sqrt(2.0 / (cin * 9))
        b = _rng("vgg16", f"features.{idx}.bias").standard_normal(v) * 0.05
        sd[f"features.{idx}.weight"] = torch.from_numpy(w.astype(np.float32))
        sd[f"features.{idx}.bias"] = torch.from_numpy(b.astype(np.float32))
        cin, idx = v, idx + 2
    assert tuple(int(k.split(".")[1]) for k in sd if k.endswith("weight")) == VGG16_CONVS
    return sd


def vgg16_features(sd=None, dtype=torch.float32):
    """torchvision's vgg16().features layer list (Conv2d, ReLU(inplace=True), MaxPool2d(2, 2)) with the weights of ``sd``."""
    sd = vgg16_state_dict() if sd is None else sd
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(cin, v, kernel_size=3, padding=1)
        i = len(layers)
        with torch.no_grad():
            conv.weight.copy_(sd[f"features.{i}.weight"])
            conv.bias.copy_(sd[f"features.{i}.bias"])
        layers += [conv, nn.ReLU(inplace=True)]
        cin = v
    return nn.Sequential(*layers).to(dtype).eval()


def image_pair(H, W, n=N, tag="pair"):
    """Seeded uint8 [n,H,W,3] frames: a smooth image plus noise, and a perturbed, shifted copy (SSIM well inside (0, 1))."""
    r = _rng("metrics", tag, H, W, n)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = r.uniform(0, 2 * np.pi, (n, 1, 1, 3))
    base = 128 + 70 * np.sin(x[None, :, :, None] / 6.0 + ph) * np.cos(y[None, :, :, None] / 9.0 - ph)
    a = np.clip(np.rint(base + r.normal(0, 14, base.shape)), 0, 255).astype(np.uint8)
    b = np.clip(np.rint(base + r.normal(0, 14, base.shape) + 5), 0, 255).astype(np.uint8)
    return a, b


def mask_for(H, W, n=N, tag="mask"):
    """Seeded binary [n,1,H,W] masks (about 60 % ones)."""
    return (_rng("metrics", tag, H, W, n).uniform(size=(n, 1, H, W)) > 0.4).astype(np.float32)


def to_tensor(u8, dtype=torch.float32):
    """uint8 [n,h,w,3] -> [n,3,h,w] in [0, 1] (ToTensor: v / 255)."""
    return (torch.from_numpy(np.ascontiguousarray(u8)).permute(0, 3, 1, 2).to(dtype) / 255.0).contiguous()


def fluid_inputs():
    """Seeded inputs of the fluid-mode case: a .flo field [h,w,2], the scene's input image uint8 [h,w,3] and one predicted frame."""
    r = _rng("metrics", "fluid")
    fh, fw = FLUID["flow_hw"]
    y, x = np.meshgrid(np.arange(fh, dtype=np.float32), np.arange(fw, dtype=np.float32), indexing="ij")
    flow = np.stack([np.sin(x / 3) * (x > 5) * 2, np.cos(y / 2) * (x > 5)], -1).astype(np.float32) + \
        r.normal(0, 0.05, (fh, fw, 2)).astype(np.float32)
    ih, iw = FLUID["image_hw"]
    image = r.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
    ph, pw = FLUID["pred_hw"]
    pred = r.integers(0, 256, (1, ph, pw, 3), dtype=np.uint8)
    return flow, image, pred


# ---------------------------------------------------------------- float64 restatement of the reference's arithmetic

def _window(window_size, C, dtype=torch.float64):
    g = torch.tensor([math.exp(-((x - window_size // 2) ** 2) / float(2 * 1.5 ** 2)) for x in range(window_size)], dtype=dtype)
    g = g / g.sum()
    return (g[:, None] @ g[None, :]).expand(C, 1, window_size, window_size).contiguous()


def ssim_f64(a, b, window_size=11, mask=None, size_average=True):
    """models/losses/ssim.py:_ssim in float64; a, b float [N,C,H,W] in [0, 1]."""
    a, b = a.double(), b.double()
    C = a.shape[1]
    w = _window(window_size, C).to(a.device)
    conv = lambda t: F.conv2d(t, w, padding=window_size // 2, groups=C)  # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    if mask is not None:
        mask = mask.double()
        n = mask.shape[0]
        return (m.mean(1, keepdim=True) * mask).view(n, -1).sum(1) / mask.view(n, -1).sum(1).clamp(min=1)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def psnr_f64(a, b, mask=None):
    """evaluation/animation/metrics.py:psnr in float64."""
    a, b = a.double(), b.double()
    n = a.shape[0]
    if mask is not None:
        mask = mask.double()
        mse = ((a - b) ** 2 * mask).view(n, -1).sum(1) / (3 * mask.view(n, -1).sum(1).clamp(min=1))
    else:
        mse = ((a - b) ** 2).view(n, -1).mean(1)
    return 10 * (1 / mse).log10()


def perceptual_f64(a, b, sd=None, per_layer=False, features=None):
    """perceptual_sim(a, b, PNet("vgg")) in float64: a, b float [N,3,H,W] in [0, 1]."""
    feats = features if features is not None else vgg16_features(sd, torch.float64)
    shift = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)

    def run(x):
        h, outs = ((x.double() * 2 - 1) - shift) / scale, []
        for lo, hi in SLICES:
            for i in range(lo, hi):
                h = feats[i](h)
            outs.append(h)
        return outs

    def norm(f):
        return f / (torch.sqrt((f ** 2).sum(1, keepdim=True)) + 1e-10)

    with torch.no_grad():
        per = [1.0 - (norm(f0) * norm(f1)).sum(1).mean((1, 2)) for f0, f1 in zip(run(a), run(b))]
    total = sum(per[1:], per[0])
    return (total, per) if per_layer else total
