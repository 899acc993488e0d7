"""LPIPS v0.1, net "alex", eval() mode, spatial averaging -- the definition the kernels of csrc/lpips.hip are tested against, written out
from torch operators and evaluated on the CPU in float64 (the yardstick) or float32 (what fp32 costs the definition itself: E_plain32):

    x'    = (x - shift) / scale,  shift = (-.030, -.088, -.188), scale = (.458, .448, .450): float32 VALUES (widened in float64)
    relu1 = ReLU(conv(x', 3 -> 64, 11x11, stride 4, padding 2) + b)                       features.0
    relu2 = ReLU(conv(maxpool3x3s2(relu1), 64 -> 192, 5x5, padding 2) + b)                features.3
    relu3 = ReLU(conv(maxpool3x3s2(relu2), 192 -> 384, 3x3, padding 1) + b)               features.6
    relu4 = ReLU(conv(relu3, 384 -> 256, 3x3, padding 1) + b)                             features.8
    relu5 = ReLU(conv(relu4, 256 -> 256, 3x3, padding 1) + b)                             features.10
    n(f)  = f / (sqrt(sum_c f_c^2) + 1e-10)                                               the eps is OUTSIDE the root
    d_k   = mean_hw sum_c w_k[c] (n(relu_k(in0))_c - n(relu_k(in1))_c)^2                  w_k = lin{k}.model.1.weight, no bias
    LPIPS = d_0 + d_1 + d_2 + d_3 + d_4                                                   added in that order, [N,1,1,1]

The max-pools are floor mode without padding; the zero padding of the first convolution applies to x'.  ``pnet_alex`` is the
reference's own use of the same trunk, PNet("alex") (models/networks/pretrained_networks.py:72-93): sum_k (1 - mean_hw cos), which
tests/golden/lpips_trunk_vs_reference.npz holds from the reference's code.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_fixture as LF

SHIFT32 = np.array([-0.030, -0.088, -0.188], np.float32)
SCALE32 = np.array([0.458, 0.448, 0.450], np.float32)
EPS = 1e-10


def _const(v, dtype):
    return torch.from_numpy(v).to(dtype).view(1, 3, 1, 1)                   # (float32 values, widened)


def prep(x, dtype=torch.float64, normalize=False):
    """x' of float [N,3,H,W] (uint8 [N,H,W,3]: v / 255 first)."""
    if x.dtype == torch.uint8:
        x = x.permute(0, 3, 1, 2).to(dtype) / 255.0
    x = x.cpu().to(dtype)
    if normalize:
        x = 2 * x - 1
    return (x - _const(SHIFT32, dtype)) / _const(SCALE32, dtype)


def trunk(xp, sd, dtype=torch.float64, raw=False):
    """relu1 ... relu5 of the prepared input (raw: the five convolution outputs before their ReLU)."""
    outs, h = [], xp
    for k, (idx, (_, _, _, s, p)) in enumerate(zip(LF.ALEX_CONVS, LF.ALEX_CFG)):
        if k in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        y = F.conv2d(h, sd[f"features.{idx}.weight"].to(dtype), sd[f"features.{idx}.bias"].to(dtype), stride=s, padding=p)
        h = torch.relu(y)
        outs.append(y if raw else h)
    return outs


def normalize_tensor(f):
    return f / (torch.sqrt((f ** 2).sum(1, keepdim=True)) + EPS)


def layer_distance(f0, f1, w, dtype=torch.float64):
    """d of one layer from RAW features [N,C,H,W] and head weights w [C] -> [N]."""
    f0, f1 = torch.relu(f0.cpu().to(dtype)), torch.relu(f1.cpu().to(dtype))
    d = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
    return (d * w.cpu().to(dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips(in0, in1, sd, lin, dtype=torch.float64, normalize=False):
    """(LPIPS [N], [d_0 .. d_4] each [N]) in ``dtype`` on the CPU."""
    with torch.no_grad():
        o0, o1 = trunk(prep(in0, dtype, normalize), sd, dtype), trunk(prep(in1, dtype, normalize), sd, dtype)
        per = [layer_distance(a, b, lin[f"lin{k}.model.1.weight"].reshape(-1), dtype) for k, (a, b) in enumerate(zip(o0, o1))]
    val = per[0]
    for p in per[1:]:
        val = val + p
    return val, per


def pnet_alex(in0, in1, sd, dtype=torch.float64):
    """PNet("alex").forward(in0, in1, retPerLayer=True) on this file's trunk: (val [N], the five 1 - mean_hw(cos) [N], the five
    sums over everything of relu_k(in0) -- what the golden file holds)."""
    with torch.no_grad():
        o0, o1 = trunk(prep(in0, dtype), sd, dtype), trunk(prep(in1, dtype), sd, dtype)
        per = [1.0 - (normalize_tensor(a) * normalize_tensor(b)).sum(1).mean((1, 2)) for a, b in zip(o0, o1)]
    val = 1.0 * per[0]
    for p in per[1:]:
        val = val + p
    return val, per, [a.sum() for a in o0]


def rel_err(got, want):
    """The largest error relative to max|want| (float64)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))
