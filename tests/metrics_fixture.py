"""Inputs and VGG16 weights of tests/golden/metrics_vs_reference.npz, and a float64 torch restatement of the three metrics.

Like tests/nets_fixture.py: the VGG16 weights are DEFINED here from their key names (torchvision's features.{i}.weight / .bias) and a
seed, so only the reference's outputs are committed.  tools/make_golden_metrics.py (needs the reference checkout) runs the reference's
models/losses/ssim.py, evaluation/animation/metrics.py and PNet("vgg") (its torchvision.models.vgg16 stubbed to return
vgg16_features()) on the seeded inputs below.  The float64 restatement (ssim_f64, psnr_f64, perceptual_f64) is the yardstick of the GPU
tests at sizes the file does not hold; tests/test_gpu_metric_kernels.py adds the input families the file's smooth-plus-noise pairs
leave out (hard_pairs: flat, saturated, posterised frames; feature_pairs: features with dead pixels) and the float64 / float32
definitions of the single kernels' operations, all seeded or constructed.  Test infrastructure only."""
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


def image_pair(H, W, n=N, tag="pair", C=None):
    """Seeded uint8 [n,H,W,3] frames: a smooth image plus noise, and a perturbed, shifted copy (SSIM well inside (0, 1)).
    With C: [n,H,W,C] frames of a family of their own (the seed names C; without it the inputs of the golden file)."""
    r = _rng("metrics", tag, H, W, n) if C is None else _rng("metrics", tag, H, W, C, n)
    C = 3 if C is None else C
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = r.uniform(0, 2 * np.pi, (n, 1, 1, C))
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


HARD_LEVELS = (255, 254, 253, 230, 199, 128, 64, 18, 3, 1)              # flat frames: saturated, near it, mid-range, near black


def hard_pairs(H, W):
    """Named uint8 pairs {name: (a, b)}, each [H,W,3], of the frames clips really contain and image_pair does not: flat frames a
    grey level or three apart (every pixel has the same inputs, hence the same fp32 rounding error -- nothing averages out), black, a
    saturated half next to a noisy half, posterised blocks, a frame against itself and against its one-pixel shift."""
    r = _rng("metrics", "hard", H, W)
    flat = lambda v: np.full((H, W, 3), v, np.uint8)                     # noqa: E731
    out = {}
    for v in HARD_LEVELS:
        for d in (1, 3):
            if v - d >= 0:
                out[f"flat{v}-{d}"] = (flat(v), flat(v - d))
    out["black+1"] = (flat(0), flat(1))
    pa, pb = image_pair(H, W, n=1, tag="hard")
    n0, n1 = pa[0], pb[0]
    a, b = n0.copy(), n1.copy()
    a[:, :W // 2], b[:, :W // 2] = 255, 253
    out["half_saturated"] = (a, b)
    post = n0 // 32 * 32
    out["posterised+1"] = (post, post + 1)
    out["self"] = (n0, n0.copy())
    out["shift1"] = (n0, np.roll(n0, 1, axis=1))
    grad = np.clip(r.integers(0, 4, (H, W, 3)) + 250, 0, 255).astype(np.uint8)      # a clipped sky: 250 .. 253 with the odd step
    out["near_saturated_texture"] = (grad, np.minimum(grad.astype(np.int32) + 2, 255).astype(np.uint8))
    return out


def hard_pairs_float(H, W):
    """The float forms {name: (a, b)}, each float32 [3,H,W] in [0, 1], of hard_pairs with values off the uint8 lattice: + U(-0.2, 0.2) / 255,
    clipped.  Flat pairs get one offset per frame and channel (they stay flat); the textured pairs one per pixel; "self" stays a frame
    against itself and "shift1" a frame against its own shift."""
    r = _rng("metrics", "hard_float", H, W)
    out = {}
    for name, (a, b) in hard_pairs(H, W).items():
        shape = (3, 1, 1) if name.startswith(("flat", "black")) else (3, H, W)
        jit = lambda: r.uniform(-0.2, 0.2, shape) / 255.0               # noqa: E731
        fa = np.clip(a.transpose(2, 0, 1) / 255.0 + jit(), 0.0, 1.0).astype(np.float32)
        if name == "self":
            fb = fa.copy()
        elif name == "shift1":
            fb = np.roll(fa, 1, axis=2)
        else:
            fb = np.clip(b.transpose(2, 0, 1) / 255.0 + jit(), 0.0, 1.0).astype(np.float32)
        out[name] = (np.broadcast_to(fa, (3, H, W)).copy(), np.broadcast_to(fb, (3, H, W)).copy())
    return out


def feature_pairs(N, C, H, W):
    """Named float32 feature pairs {name: (f0, f1)}, each [N,C,H,W] (NCHW), for the feature-distance kernel: signs, scales and the
    pixels whose ReLU'd feature vector is all zero (the + 1e-10 of normalize_tensor), which dense random weights never produce."""
    r = _rng("metrics", "features", N, C, H, W)
    g = lambda: torch.from_numpy(r.standard_normal((N, C, H, W)).astype(np.float32))   # noqa: E731
    band = torch.zeros(H * W, dtype=torch.bool)
    band[: max(1, (H * W) // 3)] = True                                   # a third of the pixels (the only one at 1 x 1)
    band = band.view(1, 1, H, W)
    f0, f1 = g(), g()
    out = {"randn": (f0, f1)}
    neg = -f0.abs() - 0.5
    out["dead_in_f0"] = (torch.where(band, neg, f0), f1)
    out["dead_in_f1"] = (f0, torch.where(band, neg, f1))
    out["dead_in_both"] = (torch.where(band, neg, f0), torch.where(band, neg, f1))
    out["same"] = (f0, f0.clone())
    out["times3"] = (f0, 3 * f0)
    out["small"] = (1e-3 * f0, 1e-3 * f1)
    out["large"] = (1e3 * f0, 1e3 * f1)
    out["small_vs_large"] = (1e-3 * f0, 1e3 * f1)
    out["channels_permuted"] = (f0, f0[:, torch.from_numpy(r.permutation(C))].contiguous())
    return out, band


def feature_distance_def(f0, f1, dtype=torch.float64):
    """1 - mean_hw(cos) of the ReLU'd features, perceptual_f64's norm / 1 - mean, every operation in ``dtype`` on the CPU -> [N] float64."""
    def norm(f):
        f = torch.relu(f.cpu().to(dtype))
        return f / (torch.sqrt((f ** 2).sum(1, keepdim=True)) + 1e-10)
    return (1.0 - (norm(f0) * norm(f1)).sum(1).mean((1, 2))).double()


def to_blocked(x):
    """[N,C,H,W] -> the channel-blocked layout of the fp32-rung convolutions (blocks of 8 channels innermost), same shape."""
    N, C, H, W = x.shape
    return x.reshape(N, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().view(N, C, H, W)


def from_blocked(x):
    N, C, H, W = x.shape
    return x.view(N, C // 8, H, W, 8).permute(0, 1, 4, 2, 3).reshape(N, C, H, W)


def vgg_prep_f64(x, from01):
    """PNet's input scaling in float64: x float64 [N,3,H,W]; ((x * 2 - 1) - shift) / scale with from01, (x - shift) / scale without."""
    x = x.double()
    if from01:
        x = x * 2 - 1
    return (x - torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)


# ---------------------------------------------------------------- float64 restatement of the reference's arithmetic

def _window1d(window_size, dtype=torch.float64):
    g = torch.tensor([math.exp(-((x - window_size // 2) ** 2) / float(2 * 1.5 ** 2)) for x in range(window_size)], dtype=dtype)
    return g / g.sum()


def _window(window_size, C, dtype=torch.float64):
    g = _window1d(window_size, dtype)
    return (g[:, None] @ g[None, :]).expand(C, 1, window_size, window_size).contiguous()


def ssim_map(a, b, window_size=11, dtype=torch.float64, separable=False):
    """models/losses/ssim.py:_ssim up to its ssim_map [N,C,H,W], every operation in ``dtype``; a, b float [N,C,H,W] in [0, 1].
    separable: the same window g g^T applied as a row pass and a column pass (same zero padding; 2 ws instead of ws^2 terms) -- for
    float64 at 720p, where the difference from the 2-D sum is ~1e-16 and the time 5x less."""
    a, b = a.to(dtype), b.to(dtype)
    C, R = a.shape[1], window_size // 2
    w = _window(window_size, C, dtype).to(a.device)
    if separable:
        g = _window1d(window_size, dtype).to(a.device)
        wr, wc = g.view(1, 1, 1, -1).expand(C, 1, 1, -1).contiguous(), g.view(1, 1, -1, 1).expand(C, 1, -1, 1).contiguous()
        conv = lambda t: F.conv2d(F.conv2d(t, wr, padding=(0, R), groups=C), wc, padding=(R, 0), groups=C)  # noqa: E731
    else:
        conv = lambda t: F.conv2d(t, w, padding=R, groups=C)             # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def ssim_reduce(m, mask=None, size_average=True):
    """ssim.py:61-69 on an ssim_map, in float64: the masked per-image form, the mean, or the per-image means."""
    m = m.double()
    if mask is not None:
        mask = mask.double()
        n = m.shape[0]
        return (m.mean(1, keepdim=True) * mask).view(n, -1).sum(1) / mask.expand(n, -1, -1, -1).reshape(n, -1).sum(1).clamp(min=1)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def ssim_f64(a, b, window_size=11, mask=None, size_average=True):
    """models/losses/ssim.py:_ssim in float64; a, b float [N,C,H,W] in [0, 1]."""
    return ssim_reduce(ssim_map(a, b, window_size, torch.float64), mask, size_average)


def ssim_f32_reference(a, b, window_size=11, mask=None, size_average=False):
    """ssim_f64's code with the window, the inputs and every product in float32 on the CPU -- the reference's formulation (one 2-D
    window of ws x ws terms) at the reference's precision; only the final per-image mean is taken in float64.  It is NOT an oracle:
    the tests compare the kernels with float64 and use this to size the bound (what fp32 costs the reference itself on these inputs).
    (= ssim_reduce(ssim_map(float32)); the tests call the two steps themselves to share one map between the masked and unmasked forms.)"""
    return ssim_reduce(ssim_map(a.cpu(), b.cpu(), window_size, torch.float32), mask, size_average)


def psnr_f64(a, b, mask=None):
    """evaluation/animation/metrics.py:psnr in float64."""
    a, b = a.double(), b.double()
    n = a.shape[0]
    if mask is not None:
        mask = mask.double()
        mse = ((a - b) ** 2 * mask).view(n, -1).sum(1) / (3 * mask.expand(n, -1, -1, -1).reshape(n, -1).sum(1).clamp(min=1))
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
