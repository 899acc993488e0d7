#!/usr/bin/env python
"""Milliseconds per motion prediction of the two motion U-Nets (nets.Unet4Motion, nets.SPADEUnet4MaskMotion) at 256^2 and 768^2, batch 1:
HIP events around each forward, median of --iters (>= 50) after warm-up; FLOPs counted from the layer shapes and the fraction of the
fp32 matrix peak (157 TFLOP/s); the same modules under nets.torch_convolutions() (MIOpen fp32 convolutions + torch elementwise ops) for
comparison.  Per-kernel times: run it once under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/motion_bench.py --quick`.
Prints one JSON line per (net, size)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slr_sfs_amd import nets  # noqa: E402

PEAK_F32 = 157.3e12


def flops(spade, H, W, cin, nf=32):
    """Multiply-adds x 2 of every convolution (4x4 encoder, 3x3 decoder, SPADE's 3x3 mlp_shared and gamma/beta convolutions)."""
    enc = [cin, nf, nf * 2, nf * 4, nf * 8, nf * 8, nf * 8, nf * 8, nf * 8]
    dec = [(nf * 8, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 4), (nf * 8, nf * 2), (nf * 4, nf),
           (nf * 2, 2)]
    area = lambda lv: (H >> lv) * (W >> lv)  # noqa: E731
    f = {"enc4x4": 0, "dec3x3": 0, "spade": 0}
    for i in range(1, 9):
        f["enc4x4"] += 2 * enc[i] * enc[i - 1] * 16 * area(i)
        if spade and 2 <= i <= 7:
            f["spade"] += 2 * 9 * area(i) * (128 * 6 + 2 * enc[i] * 128)
    for k, (ci, co) in enumerate(dec, 1):
        f["dec3x3"] += 2 * co * ci * 9 * area(8 - k)
        if spade and k < 8:
            f["spade"] += 2 * 9 * area(8 - k) * (128 * 6 + 2 * co * 128)
    return f


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a few forwards of each, no MIOpen leg (for a profiler run)")
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, cls, cin in (("SPADEUnet4MaskMotion", nets.SPADEUnet4MaskMotion, 6), ("Unet4Motion", nets.Unet4Motion, 3)):
        net = cls(cin).cuda().eval()
        for S in (256, 768):
            x = torch.rand(1, cin, S, S, device="cuda") * 2 - 1
            if a.quick:
                time_ms(lambda: net(x), 3, 1)
                continue
            ms = time_ms(lambda: net(x), a.iters, a.warmup)
            with nets.torch_convolutions():
                ms_torch = time_ms(lambda: net(x), a.iters, a.warmup)
            f = flops(cin == 6, S, S, cin)
            tot = sum(f.values())
            print(json.dumps({"net": name, "size": S, "ms": round(ms, 3), "ms_miopen_route": round(ms_torch, 3),
                              "gflop": round(tot / 1e9, 2), "gflop_parts": {k: round(v / 1e9, 2) for k, v in f.items()},
                              "tflops": round(tot / ms / 1e9, 1), "frac_fp32_peak": round(tot / (ms * 1e-3) / PEAK_F32, 3)}), flush=True)
    # the 4x4 / stride 2 kernel alone at the conv2..conv4 shapes of 768^2
    if not a.quick:
        for cin, cout, S in ((32, 64, 384), (64, 128, 192), (128, 256, 96)):
            conv = nets.Conv4x4s2(cin, cout).cuda()
            x = torch.randn(1, cin, S, S, device="cuda")
            with torch.no_grad():
                ms = time_ms(lambda: conv(x, leaky=0.2), a.iters, a.warmup)
            fl = 2 * cout * cin * 16 * (S // 2) ** 2
            print(json.dumps({"kernel": "conv4x4s2", "cin": cin, "cout": cout, "in": S, "ms": round(ms, 4),
                              "frac_fp32_peak": round(fl / (ms * 1e-3) / PEAK_F32, 3)}), flush=True)


if __name__ == "__main__":
    main()
