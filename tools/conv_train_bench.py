#!/usr/bin/env python
"""Forward + backward (gradients to input, weight and bias) of one learning 3x3 convolution of the decoder on the training crop, two ways
in one process with the same seeded weights:

  A  F.conv2d (MIOpen) + torch autograd -- what the reference's nn.Conv2d / PartialConv2d run; the partial form as the torch ops of
     models/layers/partialconv2d.py:61-74 (the mask convolution under no_grad included);
  B  slr_sfs_amd.conv3x3 / partial_conv3x3 (csrc/conv.hip forward and backward-data, csrc/conv_grad.hip weight and bias gradient), on
     channel-blocked activations where the channel counts allow (the package's activation layout); Bn: the same on NCHW tensors.

Per shape: warm-up, then A, B (and Bn) alternated (ROUNDS rounds of STEPS steps, device events around every block), and -- unless
--no-trace -- one child process per variant under `rocprofv3 --kernel-trace` for the sum of kernel time and the launches per step.  The
same run records E = max|dW - dW64| / max|dW64| of both against float64 on the CPU (K = N H W = 131 072 at 256 x 256).  No threshold: the
numbers are recorded.  Prints one JSON document (--out FILE writes it too).  A device is required.

    python tools/conv_train_bench.py --out profiles/conv_train_step.json
"""
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (N, Cin, Cout, H, W, partial)
SHAPES = {"conv_2x64to64x256x256": (2, 64, 64, 256, 256, False), "conv_2x64to128x256x256": (2, 64, 128, 256, 256, False),
          "conv_2x128to256x128x128": (2, 128, 256, 128, 128, False), "conv_2x256to256x64x64": (2, 256, 256, 64, 64, False),
          "conv_2x128to3x256x256": (2, 128, 3, 256, 256, False), "pconv_2x64to64x256x256": (2, 64, 64, 256, 256, True)}


def to_blocked(x):
    N, C, H, W = x.shape
    return x.reshape(N, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().view(N, C, H, W)


def make_case(shape):
    N, cin, cout, H, W, partial = shape
    g = torch.Generator(device="cpu").manual_seed(cin * 1000 + cout)
    c = dict(x=torch.randn(N, cin, H, W, generator=g), w=torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5),
             b=torch.randn(cout, generator=g) * 0.1, g=torch.randn(N, cout, H, W, generator=g))
    if partial:
        m = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
        m[:, :, H // 3:H // 3 + 40, W // 4:W // 4 + 50] = 0.0
        c["mask"], c["x"] = m, c["x"] * m
    return c


def stepper(S, shape, c, variant):
    """step() -> (dx, dW, db) of one forward + backward of ``variant`` on device copies of the case."""
    N, cin, cout, H, W, partial = shape
    ib8, ob8 = variant == "B" and not partial and cin % 8 == 0, variant == "B" and not partial and cout % 8 == 0
    place = lambda t, b8: (to_blocked(t) if b8 else t).cuda()               # noqa: E731
    x, g = place(c["x"], ib8).requires_grad_(True), place(c["g"], ob8)
    w, b = c["w"].cuda().requires_grad_(True), c["b"].cuda().requires_grad_(True)
    if partial:
        mask = c["mask"].cuda()
        mfull, ones = mask.expand(N, cin, H, W).contiguous(), torch.ones(cout, cin, 3, 3, device="cuda")

    def forward():
        if variant == "A" and partial:
            with torch.no_grad():
                um_raw = F.conv2d(mfull, ones, padding=1)
                ratio = (cin * 9) / (um_raw + 1e-8)
                um = torch.clamp(um_raw, 0, 1)
                ratio = ratio * um
            raw = F.conv2d(x * mfull, w, b, padding=1)
            bv = b.view(1, cout, 1, 1)
            return ((raw - bv) * ratio + bv) * um
        if variant == "A":
            return F.conv2d(x, w, b, padding=1)
        if partial:
            return S.partial_conv3x3(x, mask, w, b)[0]
        return S.conv3x3(x, w, b, in_b8=ib8, out_b8=ob8)

    def step():
        x.grad = w.grad = b.grad = None
        forward().backward(g)
        return x.grad, w.grad, b.grad
    return step, dict(in_b8=bool(ib8), out_b8=bool(ob8))


MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: brackets the traced steps


def run_only(S, args):
    shape = SHAPES[args.shape]
    step, _ = stepper(S, shape, make_case(shape), args.only)
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        step()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_step(args, shape_name, variant):
    """Kernel time per step of one variant from a child process under rocprofv3: the kernels between the two markers of run_only."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--shape", shape_name, "--steps", str(args.trace_steps),
               "--warmup", str(args.trace_warmup)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if MARKER in r[2]]
    assert len(marks) == 2, f"{len(marks)} markers"
    per, n = {}, args.trace_steps
    for t0, t1, name in rows[marks[0] + 1:marks[1]]:
        per.setdefault(name, []).append(t1 - t0)
    top = sorted(((sum(v) / n / 1e3, len(v) / n, k) for k, v in per.items()), reverse=True)[:8]
    return dict(kernel_us_per_step=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
                launches_per_step=round(sum(len(v) for v in per.values()) / n, 2),
                top=[dict(us_per_step=round(u, 2), launches_per_step=round(m, 2), kernel=k[:120]) for u, m, k in top])


def dw_float64(c, partial):
    """The weight gradient's definition in float64 on the CPU: dW[co][ci][ky][kx] = sum g[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]."""
    x, g = c["x"].double(), c["g"].double()
    if partial:
        cin = x.shape[1]
        box = F.avg_pool2d(c["mask"].double(), 3, stride=1, padding=1, divisor_override=1) * cin
        um = box.clamp(0, 1)
        g = g * ((9.0 * cin) / (box + 1e-8) * um * um)
    N, cin, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.zeros(g.shape[1], cin, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, xp[:, :, ky:ky + H, kx:kx + W])
    return dw


def measure(S, args, shape_name):
    shape = SHAPES[shape_name]
    N, cin, cout, H, W, partial = shape
    c = make_case(shape)
    variants = ["A", "B"] + ([] if partial else ["Bn"])
    steps, layouts = {}, {}
    for v in variants:
        steps[v], layouts[v] = stepper(S, shape, c, v)
    res = {"shape": dict(N=N, Cin=cin, Cout=cout, H=H, W=W, partial=partial), "rounds": args.rounds, "steps_per_round": args.steps,
           "B_layout": layouts["B"], "weight_gradient_gflop": round(2.0 * 9 * cin * cout * N * H * W / 1e9, 3)}
    if not args.no_accuracy:
        ref = dw_float64(c, partial)
        E = lambda t: float((t.detach().cpu().double() - ref).abs().max() / ref.abs().max())      # noqa: E731
        res["E_dW_vs_float64"] = {v: E(steps[v]()[1]) for v in variants}
        res["K"] = N * H * W
    times = {v: [] for v in variants}
    for v in variants:
        for _ in range(args.warmup):
            steps[v]()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                steps[v]()
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for v in variants:
        t = times[v]
        res[f"{v}_step_us_rounds"] = [round(x, 2) for x in t]
        res[f"{v}_step_us"] = round(float(np.median(t)), 2)
        res[f"{v}_step_us_spread"] = round(float(max(t) - min(t)), 2)
    res["B_over_A"] = round(res["B_step_us"] / res["A_step_us"], 3)
    res["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
    res["A_faster_than_B_by_more_than_the_spread"] = bool(min(times["B"]) > max(times["A"]))
    if not args.no_trace:
        for v in "AB":
            res[f"{v}_trace"] = kernel_time_per_step(args, shape_name, v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--no-accuracy", action="store_true", help="skip the float64 weight gradient on the CPU")
    ap.add_argument("--trace-steps", type=int, default=5)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["A", "B"], help="(child of a trace) run this variant's steps and nothing else")
    ap.add_argument("--shape", choices=list(SHAPES), default="conv_2x64to64x256x256")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/conv_train_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/conv_train_bench.py", "device": torch.cuda.get_device_name(0),
           "A": "F.conv2d (MIOpen) + torch autograd; partial: the torch ops of PartialConv2d",
           "B": "slr_sfs_amd.conv3x3 / partial_conv3x3 (channel-blocked where C % 8 == 0)", "Bn": "the same on NCHW tensors",
           "cases": {}}
    for name in args.shapes:
        doc["cases"][name] = measure(S, args, name)
        if args.out:                                     # (written after every shape: a run cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
