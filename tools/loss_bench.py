#!/usr/bin/env python
"""Forward + backward of the generator loss (SynthesisLoss, --losses 1.0_l1 10.0_content: L1 + VGG19 perceptual + PSNR + SSIM, gradient
to the predicted image), two ways in one process with the same seeded weights:

  A  the reference's formulation written with torch.nn layers (nn.Conv2d / ReLU / MaxPool2d -> MIOpen, nn.L1Loss, the SSIM of
     models/losses/ssim.py as grouped F.conv2d) and torch autograd on the device -- the baseline;
  B  slr_sfs_amd.SynthesisLoss.

Shapes: [2,3,256,256] (a training crop) and [1,3,768,1280] (a frame).  Per shape: warm-up, then A and B alternated (A B A B ...: ROUNDS
rounds of STEPS steps, device events around every block), peak memory of a step of each, and -- unless --no-trace -- one child process
per variant under `rocprofv3 --kernel-trace --stats` for the sum of kernel time per step.  No threshold: the numbers are recorded.
Prints one JSON document (--out FILE writes it too).  A device is required: there is no CPU path for a timing.

    python tools/loss_bench.py --out profiles/loss_step.json
"""
import argparse
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"train_2x3x256x256": (2, 3, 256, 256), "frame_1x3x768x1280": (1, 3, 768, 1280)}
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512)                # vgg19.features[:30]
SLICE_LAST = (1, 6, 11, 20, 29)
WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
LOSSES = ["1.0_l1", "10.0_content"]


def state_dict():
    g = torch.Generator(device="cpu").manual_seed(19)
    sd, cin, idx = {}, 3, 0
    for v in CFG:
        if v == "M":
            idx += 1
            continue
        sd[f"features.{idx}.weight"] = torch.randn(v, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
        sd[f"features.{idx}.bias"] = torch.randn(v, generator=g) * 0.05
        cin, idx = v, idx + 2
    return sd


class TorchLoss(nn.Module):
    """Variant A: models/losses/synthesis.py's arithmetic on torch.nn layers."""

    def __init__(self, sd):
        super().__init__()
        layers, cin = [], 3
        for v in CFG:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
                continue
            conv = nn.Conv2d(cin, v, 3, padding=1)
            with torch.no_grad():
                conv.weight.copy_(sd[f"features.{len(layers)}.weight"])
                conv.bias.copy_(sd[f"features.{len(layers)}.bias"])
            layers += [conv, nn.ReLU(inplace=False)]
            cin = v
        self.features = nn.Sequential(*layers).requires_grad_(False)
        g = torch.tensor([math.exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)) for x in range(11)])
        g = (g / g.sum()).unsqueeze(1)
        self.register_buffer("window", g.mm(g.t()).float().expand(3, 1, 11, 11).contiguous())

    def slices(self, x):
        out = []
        for i, layer in enumerate(self.features):
            x = layer(x)
            if i in SLICE_LAST:
                out.append(x)
        return out

    def ssim(self, a, b):
        conv = lambda t: F.conv2d(t, self.window, padding=5, groups=3)    # noqa: E731
        mu1, mu2 = conv(a), conv(b)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
        return (((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))).mean()

    def forward(self, pred, gt):
        l1 = nn.L1Loss()(pred, gt)
        with torch.no_grad():
            gt_fs = self.slices(gt)
        perc = 0
        for w, p, g in zip(WEIGHTS, self.slices(pred), gt_fs):
            perc = perc + w * nn.L1Loss()(p, g)
        with torch.no_grad():
            mse = (pred - gt).pow(2).sum(dim=1).view(pred.shape[0], -1).mean(dim=1)
            psnr, ssim = (10 * (1 / mse).log10()).mean(), self.ssim(pred, gt)
        return {"L1": l1, "Perceptual": perc, "Total Loss": l1 + perc * 10.0, "psnr": psnr, "ssim": ssim}


def make_case(S, shape):
    sd = state_dict()
    g = torch.Generator(device="cpu").manual_seed(7)
    gt = torch.tanh(torch.randn(*shape, generator=g)).cuda()
    pred = torch.tanh(torch.atanh(gt.cpu().clamp(-0.999, 0.999)) + 0.2 * torch.randn(*shape, generator=g)).cuda()
    vgg = S.load_vgg19_state_dict(S.VGG19Features(), sd).cuda()
    fns = {"A": TorchLoss(sd).cuda(), "B": S.SynthesisLoss(types.SimpleNamespace(losses=LOSSES), vgg).cuda()}
    return pred, gt, fns


def step(fn, pred, gt):
    p = pred.detach().requires_grad_(True)
    out = fn(p, gt)
    out["Total Loss"].backward()
    return out, p.grad


MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: brackets the traced steps


def run_only(S, args):
    pred, gt, fns = make_case(S, SHAPES[args.shape])
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.warmup):
        step(fns[args.only], pred, gt)
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        step(fns[args.only], pred, gt)
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
    top = sorted(((sum(v) / n / 1e3, len(v) / n, k) for k, v in per.items()), reverse=True)[:10]
    return dict(kernel_us_per_step=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
                launches_per_step=round(sum(len(v) for v in per.values()) / n, 2),
                top=[dict(us_per_step=round(u, 2), launches_per_step=round(m, 2), kernel=k[:120]) for u, m, k in top])


def measure(S, args, shape_name):
    shape = SHAPES[shape_name]
    pred, gt, fns = make_case(S, shape)
    steps = args.steps if shape[2] * shape[3] <= 256 * 256 else max(args.steps // 5, 5)
    res = {"shape": list(shape), "rounds": args.rounds, "steps_per_round": steps}
    (oa, ga), (ob, gb) = step(fns["A"], pred, gt), step(fns["B"], pred, gt)
    rel = lambda x, y: float((x.detach() - y.detach()).abs().max() / y.detach().abs().max())      # noqa: E731
    # a sanity check of the workload, not a test: the gradient is discontinuous (tests/loss_f64.py), its difference is recorded as found
    res["max_rel_difference_B_vs_A"] = {**{k: rel(ob[k], oa[k]) for k in oa}, "grad": rel(gb, ga)}
    del oa, ga, ob, gb
    for v in "AB":
        for _ in range(args.warmup):
            step(fns[v], pred, gt)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(fns[v], pred, gt)
        torch.cuda.synchronize()
        res[f"{v}_peak_bytes_of_a_step"] = int(torch.cuda.max_memory_allocated() - base)
        res[f"{v}_resident_bytes_before_the_step"] = int(base)
    times = {"A": [], "B": []}
    for _ in range(args.rounds):
        for v in "AB":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(fns[v], pred, gt)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / steps)
    for v in "AB":
        t = times[v]
        res[f"{v}_step_us_rounds"] = [round(x, 2) for x in t]
        res[f"{v}_step_us"] = round(float(np.median(t)), 2)
        res[f"{v}_step_us_spread"] = round(float(max(t) - min(t)), 2)
    res["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
    res["A_faster_than_B_by_more_than_the_spread"] = bool(min(times["B"]) > max(times["A"]))
    if not args.no_trace:
        for v in "AB":
            res[f"{v}_trace"] = kernel_time_per_step(args, shape_name, v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="steps per round at 256 x 256 (a fifth of it on the frame)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=5)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["A", "B"], help="(child of a trace) run this variant's steps and nothing else")
    ap.add_argument("--shape", choices=list(SHAPES), default="train_2x3x256x256")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/loss_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/loss_bench.py", "device": torch.cuda.get_device_name(0),
           "A": "torch.nn VGG19 (MIOpen) + nn.L1Loss + torch SSIM / PSNR + torch autograd", "B": "slr_sfs_amd.SynthesisLoss",
           "losses": LOSSES, "cases": {name: measure(S, args, name) for name in args.shapes}}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
