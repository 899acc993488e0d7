"""Seeded weights and image pairs of the LPIPS tests (tests/test_lpips_host.py, tests/test_gpu_lpips.py) and of
tests/golden/lpips_trunk_vs_reference.npz.

Like tests/metrics_fixture.py: the AlexNet trunk and the LPIPS heads are DEFINED here from their key names and a seed -- convolutions
randn * sqrt(2 / fan_in), biases 0.1 * randn, heads 0.05 * |randn| --, so only the reference's outputs are committed.
tools/make_golden_lpips.py (needs the reference checkout) runs the reference's PNet("alex", pnet_rand=True, use_gpu=False) in float64
with its torchvision.models.alexnet stubbed to alexnet_features(); that pins the slices, the pools and the scaling constants to the
reference.  The linear heads have no counterpart in the reference checkout (they belong to the lpips package, which is not available):
they are checked against the written-out definition of tests/lpips_f64.py only.  Test infrastructure only."""
import math

import numpy as np
import torch
import torch.nn as nn

from nets_fixture import _rng

ALEX_CONVS = (0, 3, 6, 8, 10)                                             # torchvision alexnet().features indices of the convolutions
ALEX_CFG = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))   # cin, cout, k, stride, pad
CHANNELS = tuple(c[1] for c in ALEX_CFG)
GOLDEN_SHAPE = (2, 3, 35, 50)
SHAPES = ((1, 3, 31, 31), (2, 3, 35, 50), (3, 3, 64, 97), (1, 3, 90, 160))      # the whole-metric cases (+ (1, 3, 180, 320) once)


def alexnet_state_dict():
    """torchvision-format AlexNet feature weights, every value a function of its key."""
    sd = {}
    for idx, (cin, cout, k, _, _) in zip(ALEX_CONVS, ALEX_CFG):
        w = _rng("alexnet", f"features.{idx}.weight").standard_normal((cout, cin, k, k)) * math.sqrt(2.0 / (cin * k * k))
        b = _rng("alexnet", f"features.{idx}.bias").standard_normal(cout) * 0.1
        sd[f"features.{idx}.weight"] = torch.from_numpy(w.astype(np.float32))
        sd[f"features.{idx}.bias"] = torch.from_numpy(b.astype(np.float32))
    return sd


def linear_state_dict():
    """The keys and shapes of the lpips package's weights/v0.1/alex.pth: lin{k}.model.1.weight [1,C,1,1], non-negative as the
    package's trained heads are."""
    return {f"lin{k}.model.1.weight": torch.from_numpy((0.05 * np.abs(_rng("lpips", f"lin{k}").standard_normal((1, c, 1, 1)))).astype(np.float32))
            for k, c in enumerate(CHANNELS)}


def alexnet_features(sd=None, dtype=torch.float32):
    """torchvision's alexnet().features layer list (13 modules) with the weights of ``sd``."""
    sd = alexnet_state_dict() if sd is None else sd
    convs = {}
    for idx, (cin, cout, k, s, p) in zip(ALEX_CONVS, ALEX_CFG):
        conv = nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p)
        with torch.no_grad():
            conv.weight.copy_(sd[f"features.{idx}.weight"])
            conv.bias.copy_(sd[f"features.{idx}.bias"])
        convs[idx] = conv
    pool = lambda: nn.MaxPool2d(kernel_size=3, stride=2)                 # noqa: E731
    relu = lambda: nn.ReLU(inplace=True)                                  # noqa: E731
    return nn.Sequential(convs[0], relu(), pool(), convs[3], relu(), pool(), convs[6], relu(), convs[8], relu(), convs[10], relu(),
                         pool()).to(dtype).eval()


def image_pair(N, C, H, W, tag="pair"):
    """Seeded float32 [N,3,H,W] pairs in [0, 1]: x0 uniform, x1 = clamp(x0 + 0.3 randn)."""
    assert C == 3
    r = _rng("lpips", tag, N, H, W)
    x0 = r.uniform(0.0, 1.0, (N, 3, H, W))
    x1 = np.clip(x0 + 0.3 * r.standard_normal((N, 3, H, W)), 0.0, 1.0)
    return torch.from_numpy(x0.astype(np.float32)), torch.from_numpy(x1.astype(np.float32))
