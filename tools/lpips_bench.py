#!/usr/bin/env python
"""What LPIPS costs on an MI355X (metrics.LPIPSAlex, csrc/lpips.hip) -> profiles/lpips_eval.json.  Measured, no threshold: whatever
comes out is recorded.

  A  the same metric from torch operators in fp32 on the device: F.conv2d (MIOpen), F.max_pool2d, elementwise operators, the same
     seeded weights (tests/lpips_f64.py's definition run in float32 on the GPU)
  B  metrics.LPIPSAlex

at [4,3,720,1280] and [4,3,360,640] pairs: the two alternated in one process, median of --rounds (7) rounds with min - max, device
events around a block of --steps calls.  Unless --no-trace, one child process per side and shape under `rocprofv3 --kernel-trace`
(kernel trace only, a run of its own): launches and the sum of kernel time per call, and each new kernel's time against its FLOPs at the
fp32 matrix peak (157.3 TFLOP/s) or its bytes at 8 TB/s.  Then one 60-frame 720 x 1280 clip through evaluate_clip with and without
lpips=: what the new key costs a scene."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_f64 as D  # noqa: E402
import lpips_fixture as LF  # noqa: E402

PEAK_F32 = 157.3e12
PEAK_BW = 8.0e12
MARKER = "slr::normalize_kernel("        # a kernel of the library that neither side launches: brackets the traced calls
SHAPES = {"4x3x720x1280": (4, 720, 1280), "4x3x360x640": (4, 360, 640)}


def sizes(H, W):
    """[(C, h, w)] of relu1 .. relu5, and the pooled sizes in front of the second and third convolution."""
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    p1 = ((h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1)
    p2 = ((p1[0] - 3) // 2 + 1, (p1[1] - 3) // 2 + 1)
    return [(64, h1, w1), (192, *p1), (384, *p2), (256, *p2), (256, *p2)], p1, p2


def work(N, H, W):
    """Per new kernel, for one call on N pairs (2N images through the trunk): FLOPs of the convolutions, bytes of the others."""
    f, p1, p2 = sizes(H, W)
    B = 2 * N
    px = lambda k: f[k][1] * f[k][2]                                         # noqa: E731
    out = {"convkxk_kernel<11": {"flop": 2.0 * B * 64 * 3 * 121 * px(0)}, "convkxk_kernel<5": {"flop": 2.0 * B * 192 * 64 * 25 * px(1)},
           "lpips_prep_kernel": {"bytes": 4.0 * B * 3 * H * W * 2},
           "relu_maxpool3s2_b8_kernel": {"bytes": 4.0 * B * (64 * (px(0) + p1[0] * p1[1]) + 192 * (px(1) + p2[0] * p2[1]))},
           "lpips_distance_kernel": {"bytes": 4.0 * B * sum(c * h * w for c, h, w in f)}}
    conv3 = 2.0 * B * 9 * px(2) * (192 * 384 + 384 * 256 + 256 * 256)
    return out, out["convkxk_kernel<11"]["flop"] + out["convkxk_kernel<5"]["flop"] + conv3


def make_side(S, side, N, H, W):
    sd, lin = LF.alexnet_state_dict(), LF.linear_state_dict()
    g = torch.Generator().manual_seed(3)
    a = torch.rand(N, 3, H, W, generator=g)
    b = (a + 0.3 * torch.randn(N, 3, H, W, generator=g)).clamp(0, 1)
    a, b = a.cuda(), b.cuda()
    if side == "B":
        net = S.metrics.load_lpips_state_dicts(S.metrics.LPIPSAlex(), sd, lin).cuda()
        return lambda: S.metrics.lpips_sim(a, b, net)
    sdd = {k: v.cuda() for k, v in sd.items()}
    ws = [lin[f"lin{k}.model.1.weight"].cuda() for k in range(5)]
    shift, scale = (torch.from_numpy(v).cuda().view(1, 3, 1, 1) for v in (D.SHIFT32, D.SCALE32))

    def run():
        with torch.no_grad():
            x = (torch.cat([a, b]) - shift) / scale
            val = 0
            for f, w in zip(D.trunk(x, sdd, torch.float32), ws):
                n = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                val = val + ((n[:N] - n[N:]) ** 2 * w).sum(1).mean((1, 2))
        return val
    return run


def run_only(S, args):
    side, shape = args.only.split("_")
    run = make_side(S, side, *SHAPES[shape])
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.trace_warmup):
        run()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.trace_steps):
        run()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_call(args, name, per_kernel):
    """Launches and kernel time of one call of one side, from a child process under rocprofv3 (kernel trace only)."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", name, "--trace-steps", str(args.trace_steps), "--trace-warmup",
               str(args.trace_warmup)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if MARKER in r[2]]
    assert len(marks) == 2, f"{len(marks)} markers"
    per, n = {}, args.trace_steps
    for t0, t1, kname in rows[marks[0] + 1:marks[1]]:
        per.setdefault(kname, []).append(t1 - t0)
    total = sum(sum(v) for v in per.values()) / n / 1e3
    res = dict(kernel_us_per_call=round(total, 1), launches_per_call=round(sum(len(v) for v in per.values()) / n, 1))
    top = sorted(((sum(v) / n / 1e3, k) for k, v in per.items()), reverse=True)[:6]
    res["largest"] = [dict(us_per_call=round(us, 1), share=round(us / total, 3), launches_per_call=round(len(per[k]) / n, 1), kernel=k[:110])
                      for us, k in top]
    if per_kernel:
        new = {}
        for kernel, w in per_kernel.items():
            v = [t for k, ts in per.items() if kernel in k for t in ts]
            if v:
                us = sum(v) / n / 1e3
                e = dict(us_per_call=round(us, 1), launches_per_call=round(len(v) / n, 1), share=round(us / total, 3))
                if "flop" in w:
                    e.update(GFLOP=round(w["flop"] / 1e9, 2), share_of_fp32_matrix_peak=round(w["flop"] / (us * 1e-6) / PEAK_F32, 4))
                else:
                    e.update(MB=round(w["bytes"] / 1e6, 1), share_of_8TBs=round(w["bytes"] / (us * 1e-6) / PEAK_BW, 4))
                new[kernel] = e
        res["new_kernels"] = new
    return res


def alternate(runs, args):
    times = {k: [] for k in runs}
    for run in runs.values():
        for _ in range(args.warmup):
            run()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                run()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.steps)
    out = {}
    for k, t in times.items():
        out[k] = dict(ms=round(float(np.median(t)), 4), min_max=[round(min(t), 4), round(max(t), 4)], rounds=[round(x, 4) for x in t])
    a, b = list(times)
    out[f"{b}_over_{a}"] = round(out[b]["ms"] / out[a]["ms"], 3)
    out[f"{b}_faster_by_more_than_the_spread"] = bool(min(times[a]) > max(times[b]))
    out[f"{a}_faster_by_more_than_the_spread"] = bool(min(times[b]) > max(times[a]))
    return out


def clip_cost(S, args):
    """One 60-frame 720 x 1280 clip through evaluate_clip with and without lpips= (PSNR and SSIM either way)."""
    net = S.metrics.load_lpips_state_dicts(S.metrics.LPIPSAlex(), LF.alexnet_state_dict(), LF.linear_state_dict()).cuda()
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randint(0, 256, (60, 720, 1280, 3), dtype=torch.uint8, device="cuda", generator=g)
    y = (x.int() + torch.randint(-12, 13, x.shape, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
    runs = {"without": lambda: S.metrics.evaluate_clip(x, y), "with_lpips": lambda: S.metrics.evaluate_clip(x, y, lpips=net)}
    saved = args.steps
    args.steps = 1
    r = alternate(runs, args)
    args.steps = saved
    r["lpips_ms_per_clip"] = round(r["with_lpips"]["ms"] - r["without"]["ms"], 3)
    r["lpips_ms_per_frame"] = round(r["lpips_ms_per_clip"] / 60, 4)
    r["pairs_per_batch"] = S.metrics.lpips_batch(720, 1280)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=2)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", help="(child of a trace) run this side's calls and nothing else: A_4x3x720x1280, B_4x3x360x640, ...")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lpips_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/lpips_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_round": args.steps,
           "A": "tests/lpips_f64.py's definition from torch operators in float32 on the device (F.conv2d on MIOpen, F.max_pool2d)",
           "B": "slr_sfs_amd.metrics.LPIPSAlex (csrc/lpips.hip; the 3x3 layers on the direct fp32 kernel of csrc/conv.hip)"}
    for shape, (N, H, W) in SHAPES.items():
        runs = {"A": make_side(S, "A", N, H, W), "B": make_side(S, "B", N, H, W)}
        a, b = runs["A"]().cpu().double(), runs["B"]().cpu().double()
        r = alternate(runs, args)
        r["B_vs_A_score"] = float(((b - a).abs() / a.abs()).max())
        per_kernel, flop = work(N, H, W)
        r["GFLOP_per_pair"] = round(flop / N / 1e9, 2)
        r["B_share_of_fp32_matrix_peak"] = round(flop / (r["B"]["ms"] * 1e-3) / PEAK_F32, 4)
        r["feature_sizes"] = sizes(H, W)[0]
        if not args.no_trace:
            r["A_trace"] = kernel_time_per_call(args, f"A_{shape}", None)
            r["B_trace"] = kernel_time_per_call(args, f"B_{shape}", per_kernel)
        doc[shape] = r
        del runs
        torch.cuda.empty_cache()
    doc["clip_60x720x1280"] = clip_cost(S, args)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
