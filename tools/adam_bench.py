#!/usr/bin/env python
"""One optimiser step over the project's real parameter lists -- the generator (TrainableDecoderPconv2 + TrainableEncoderWithZ, 139
tensors, 4.0 M elements) and the discriminator (DiscriminatorLoss(ndf=64), 14 tensors, 5.5 M elements) -- with random gradients, three
ways in one process on parameters of the same shapes:

  foreach  torch.optim.Adam(foreach=True)
  fused    torch.optim.Adam(fused=True)
  new      slr_sfs_amd.Adam (csrc/adam.hip)

all with the reference's lr_g / lr_d, betas (0, 0.9), eps 1e-8.  Warm-up, then the three alternated (ROUNDS rounds of STEPS steps, device
events around every block of steps): median, min and max of the rounds per step.  Unless --no-trace, one child process per variant and
list under `rocprofv3 --kernel-trace` (kernel trace only, no counters in that run): launches and summed kernel time per step, and for
`new` the update kernel's time against its bytes (28 per element: p, g, m, v read, p, m, v written) at 8 TB/s.  No target ratio: the two
torch variants are the yardsticks and the numbers are recorded.  Prints one JSON document (--out FILE writes it too).  A device is required.

    python tools/adam_bench.py --out profiles/adam_step.json
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BW = 8.0e12
BYTES_PER_ELEMENT = 28
VARIANTS = ("foreach", "fused", "new")
LISTS = {"generator": 1e-3 / 2, "discriminator": 1e-3 * 2}               # the list and its learning rate (lr_g, lr_d)
BETAS = (0.0, 0.9)
MARKER = "slr::normalize_kernel("        # a kernel of the library that no variant launches: brackets the traced steps


def parameter_list(S, which):
    """Fresh parameters of the real shapes on the device, each with a random gradient of its own."""
    torch.manual_seed(1234)
    mods = [S.TrainableDecoderPconv2(), S.TrainableEncoderWithZ()] if which == "generator" else [S.DiscriminatorLoss(ndf=64)]
    params = [p for m in mods for p in m.cuda().parameters()]
    for p in params:
        p.grad = 1e-2 * torch.randn_like(p)
    return params


def make(S, variant, params, lr):
    if variant == "new":
        return S.Adam(params, lr=lr, betas=BETAS)
    return torch.optim.Adam(params, lr=lr, betas=BETAS, foreach=variant == "foreach", fused=variant == "fused")


def shape_of(params):
    n = [p.numel() for p in params]
    return dict(tensors=len(n), elements=int(sum(n)), smallest=int(min(n)), median=float(np.median(n)),
                MB_per_step=round(BYTES_PER_ELEMENT * sum(n) / 1e6, 1), us_at_8TBs=round(BYTES_PER_ELEMENT * sum(n) / PEAK_BW * 1e6, 2))


def run_only(S, args):
    opt = make(S, args.only, parameter_list(S, args.which), LISTS[args.which])
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.warmup):
        opt.step()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        opt.step()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_step(args, variant, which, elements):
    """Launches and kernel time of one step of one variant on one list, from a child process under rocprofv3."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--which", which, "--steps", str(args.trace_steps),
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
    top = sorted((dict(us_per_step=round(sum(v) / n / 1e3, 2), launches_per_step=round(len(v) / n, 2), kernel=k[:120]) for k, v in per.items()),
                 key=lambda r: -r["us_per_step"])
    res = dict(kernel_us_per_step=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
               launches_per_step=round(sum(len(v) for v in per.values()) / n, 2), top=top[:4])
    if variant == "new":
        for key, pat in (("update_kernel", "adam_update_kernel"), ("prepare_kernel", "adam_prepare_kernel")):
            v = [x for k, xs in per.items() if pat in k for x in xs]
            res[key] = dict(us_per_step=round(sum(v) / n / 1e3, 2), launches_per_step=round(len(v) / n, 2))
        us = res["update_kernel"]["us_per_step"]
        if us > 0:
            by = BYTES_PER_ELEMENT * elements
            res["update_kernel"].update(MB=round(by / 1e6, 1), TBs=round(by / us / 1e6, 3), share_of_8TBs=round(by / us / 1e-6 / PEAK_BW, 4))
    return res


def measure(S, args, which):
    lr = LISTS[which]
    opts = {}
    for v in VARIANTS:                                   # each variant steps parameters of its own: none sees another's updates
        opts[v] = make(S, v, parameter_list(S, which), lr)
    res = {"list": shape_of(opts["new"].param_groups[0]["params"]), "lr": lr}
    times = {v: [] for v in VARIANTS}
    for v in VARIANTS:
        for _ in range(args.warmup):
            opts[v].step()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v in VARIANTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                opts[v].step()
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for v in VARIANTS:
        t = times[v]
        res[v] = dict(step_us=round(float(np.median(t)), 2), step_us_min_max=[round(min(t), 2), round(max(t), 2)],
                      step_us_rounds=[round(x, 2) for x in t])
    for v in ("foreach", "fused"):
        res[f"new_over_{v}"] = round(res["new"]["step_us"] / res[v]["step_us"], 3)
        res[f"new_faster_than_{v}_by_more_than_the_spread"] = bool(min(times[v]) > max(times["new"]))
        res[f"{v}_faster_than_new_by_more_than_the_spread"] = bool(min(times["new"]) > max(times[v]))
    if not args.no_trace:
        for v in VARIANTS:
            res[v]["trace"] = kernel_time_per_step(args, v, which, res["list"]["elements"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=5)
    ap.add_argument("--trace-warmup", type=int, default=3)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=VARIANTS, help="(child of a trace) run this variant's steps and nothing else")
    ap.add_argument("--which", choices=sorted(LISTS), default="generator", help="(child of a trace) the parameter list")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/adam_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/adam_bench.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "foreach": "torch.optim.Adam(foreach=True)", "fused": "torch.optim.Adam(fused=True)", "new": "slr_sfs_amd.Adam (csrc/adam.hip)",
           "betas": list(BETAS), "rounds": args.rounds, "steps_per_round": args.steps,
           "step_us": "device events around a block of steps, per step: what a training loop waits for, host launch cost included"}
    for which in LISTS:
        doc[which] = measure(S, args, which)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
