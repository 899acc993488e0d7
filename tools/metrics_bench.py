#!/usr/bin/env python
"""Times of the clip-evaluation metrics (slr_sfs_amd.metrics) at 720 x 1280: HIP events around each call, median of --iters (>= 50) after
warm-up, next to the reference's arithmetic run through torch on the same GPU (grouped F.conv2d on MIOpen for SSIM, F.conv2d + torch
ReLU / max pool / cos_sim for VGG16).  Prints one JSON line per case:
  ssim_psnr  : SSIM + PSNR of one 60-frame clip pair from uint8 frames -- us, fraction of 8 TB/s on the input bytes, vs torch;
  perceptual : the Perceptual metric per frame pair (batches of metrics.perceptual_batch pairs) -- ms, fraction of the 157.3 TFLOP/s
               fp32 matrix peak of its 13 convolutions (time of the convolutions alone), share of the pooling + distance kernels, vs MIOpen;
  clip       : a whole 60-frame clip scored with all three metrics (evaluate_clip), seconds.
Random VGG16 weights (the timing does not depend on them)."""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slr_sfs_amd import metrics  # noqa: E402

PEAK_F32 = 157.3e12
HBM = 8.0e12


def time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def torch_ssim_psnr(a_u8, b_u8, ws=11):
    """ssim.py:_ssim + metrics.py:psnr as torch ops (grouped F.conv2d -> MIOpen) from uint8 frames, one clip at a time."""
    a = a_u8.permute(0, 3, 1, 2).float() / 255.0
    b = b_u8.permute(0, 3, 1, 2).float() / 255.0
    g = torch.tensor([math.exp(-((x - ws // 2) ** 2) / float(2 * 1.5 ** 2)) for x in range(ws)], device=a.device)
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).expand(3, 1, ws, ws).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=ws // 2, groups=3)  # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    m1s, m2s, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(a * a) - m1s, conv(b * b) - m2s, conv(a * b) - m12
    m = ((2 * m12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((m1s + m2s + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m.mean((1, 2, 3)), 10 * (1 / (a - b).pow(2).mean((1, 2, 3))).log10()


def torch_vgg(net, x0, x1):
    """PNet("vgg") as torch ops (F.conv2d on MIOpen, fp32) with the same weights."""
    shift = torch.tensor([-0.030, -0.088, -0.188], device=x0.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=x0.device).view(1, 3, 1, 1)
    x = (torch.cat([x0, x1]) * 2 - 1 - shift) / scale
    n, k, val = x0.shape[0], 0, 0
    for s, cnt in enumerate(metrics.VGG16_SLICES):
        if s:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(cnt):
            c = net.convs[k]
            x = F.relu(F.conv2d(x, c.weight, c.bias, padding=1))
            k += 1
        f = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        val = val + 1.0 - (f[:n] * f[n:]).sum(1).mean((1, 2))
    return val


def vgg_flops(H, W):
    f, h, w, k = 0, H, W, 0
    for s, cnt in enumerate(metrics.VGG16_SLICES):
        if s:
            h, w = h // 2, w // 2
        for _ in range(cnt):
            f += 2 * 9 * metrics.VGG16_CHANNELS[k] * metrics.VGG16_CHANNELS[k + 1] * h * w
            k += 1
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=60)
    a = ap.parse_args()
    H, W, n = 720, 1280, a.frames
    torch.manual_seed(0)
    dev = torch.device("cuda")
    x = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev)
    y = (x.int() + torch.randint(-12, 13, x.shape, device=dev)).clamp(0, 255).to(torch.uint8)
    with torch.no_grad():
        us = time_ms(lambda: metrics.ssim_mse(x, y), a.iters, a.warmup) * 1e3
        us_t = time_ms(lambda: torch_ssim_psnr(x, y), max(10, a.iters // 5), 2) * 1e3
        s_ours, s_t = metrics.ssim_mse(x, y)[:, 0], torch_ssim_psnr(x, y)[0]
    print(json.dumps({"case": "ssim_psnr", "frames": n, "size": [H, W], "us": round(us, 1), "us_torch_miopen": round(us_t, 1),
                      "speedup_vs_torch": round(us_t / us, 2), "frac_hbm_8tbs_input_bytes": round(2 * x.numel() / (us * 1e-6) / HBM, 3),
                      "max_abs_diff_ssim_vs_torch": float((s_ours - s_t).abs().max())}), flush=True)

    net = metrics.PerceptualVGG16().to(dev)
    B = metrics.perceptual_batch(H, W)
    xb, yb = x[:B].contiguous(), y[:B].contiguous()
    with torch.no_grad():
        ms = time_ms(lambda: metrics.perceptual_sim(xb, yb, net), a.iters, a.warmup) / B
        prep = torch.empty(2 * B, 3, H, W, device=dev)
        for t, part in ((xb, prep[:B]), (yb, prep[B:])):
            metrics._lib.call("slr_vgg_prep", dev, t, 1, 1, part, B, H, W)
        ms_feat = time_ms(lambda: net.features(prep), a.iters, a.warmup) / B
        feats = net.features(prep)
        pools = [metrics.relu_maxpool2x2(f) for f in feats[:4]]
        ms_pool = time_ms(lambda: [metrics.relu_maxpool2x2(f) for f in feats[:4]], a.iters, a.warmup) / B
        ms_dist = time_ms(lambda: [metrics.feature_distance(f[:B], f[B:]) for f in feats], a.iters, a.warmup) / B
        del pools
        xf, yf = (xb.permute(0, 3, 1, 2).float() / 255).contiguous(), (yb.permute(0, 3, 1, 2).float() / 255).contiguous()
        ms_t = time_ms(lambda: torch_vgg(net, xf, yf), max(10, a.iters // 5), 2) / B
        diff = float((metrics.perceptual_sim(xb, yb, net) - torch_vgg(net, xf, yf)).abs().max())
    fl = 2 * vgg_flops(H, W)                                                # both images of a pair
    ms_conv = ms_feat - ms_pool
    print(json.dumps({"case": "perceptual", "size": [H, W], "pairs_per_batch": B, "ms_per_pair": round(ms, 3),
                      "ms_per_pair_torch_miopen": round(ms_t, 3), "speedup_vs_miopen": round(ms_t / ms, 2),
                      "gflop_per_pair": round(fl / 1e9, 1), "ms_convs_per_pair": round(ms_conv, 3),
                      "frac_fp32_peak_convs": round(fl / (ms_conv * 1e-3) / PEAK_F32, 3),
                      "frac_pool_and_distance": round((ms_pool + ms_dist) / ms, 3), "max_abs_diff_vs_torch": diff}), flush=True)

    with torch.no_grad():
        def clip():
            r = metrics.evaluate_clip(x, y, perceptual=net)
            return r["Perceptual"]
        ms_clip = time_ms(clip, 3, 1)
    print(json.dumps({"case": "clip", "frames": n, "size": [H, W], "metrics": ["PSNR", "SSIM", "Perceptual"],
                      "seconds": round(ms_clip / 1e3, 3)}), flush=True)


if __name__ == "__main__":
    main()
