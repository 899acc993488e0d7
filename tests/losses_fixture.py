"""Inputs and VGG19 weights of tests/golden/losses_vs_reference.npz.

Like tests/metrics_fixture.py: the VGG19 weights are DEFINED here from their key names (torchvision's features.{i}.weight / .bias) and a
seed, so only the reference's outputs are committed.  tools/make_golden_losses.py (needs the reference checkout) runs the reference's own
SynthesisLoss (models/losses/synthesis.py; its torchvision.models.vgg19 stubbed to return vgg19_features()) in float64 on the seeded
images below.  tests/loss_f64.py restates the same arithmetic for the sizes the file does not hold.  Test infrastructure only."""
import math

import numpy as np
import torch
import torch.nn as nn

from nets_fixture import _rng

VGG19_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512)      # torchvision cfg "E" up to features.28
VGG19_CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
GOLDEN_SHAPE = (2, 3, 32, 48)
LOSSES = ("1.0_l1", "10.0_content")                                       # options/train_options.py:390


def vgg19_state_dict():
    """torchvision-format VGG19 feature weights up to features.28, every value a function of its key (He-scaled normal weights, small
    biases), float32."""
    sd, cin, idx = {}, 3, 0
    for v in VGG19_CFG:
        if v == "M":
            idx += 1
            continue
        w = _rng("vgg19", f"features.{idx}.weight").standard_normal((v, cin, 3, 3)) * math.sqrt(2.0 / (cin * 9))
        b = _rng("vgg19", f"features.{idx}.bias").standard_normal(v) * 0.05
        sd[f"features.{idx}.weight"] = torch.from_numpy(w.astype(np.float32))
        sd[f"features.{idx}.bias"] = torch.from_numpy(b.astype(np.float32))
        cin, idx = v, idx + 2
    assert tuple(int(k.split(".")[1]) for k in sd if k.endswith("weight")) == VGG19_CONVS
    return sd


def vgg19_features(sd=None, dtype=torch.float32):
    """torchvision's vgg19().features[:30] layer list (Conv2d, ReLU(inplace=True), MaxPool2d(2, 2)) with the weights of ``sd``."""
    sd = vgg19_state_dict() if sd is None else sd
    layers, cin = [], 3
    for v in VGG19_CFG:
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
    assert len(layers) == 30
    return nn.Sequential(*layers).to(dtype).eval()


def image_pair(N, H, W, tag="pair"):
    """Seeded float32 [N,3,H,W] images in [-1, 1] (what the reference's generators emit and its loaders give): a smooth image plus noise
    as the ground truth, and a perturbed copy as the prediction.  -> (pred, gt)."""
    r = _rng("losses", tag, N, H, W)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = r.uniform(0, 2 * np.pi, (N, 3, 1, 1))
    base = 0.6 * np.sin(x[None, None] / 5.0 + ph) * np.cos(y[None, None] / 7.0 - ph)
    gt = np.clip(base + r.normal(0, 0.1, base.shape), -1, 1).astype(np.float32)
    pred = np.clip(base + r.normal(0, 0.1, base.shape) + 0.03, -1, 1).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(gt)
