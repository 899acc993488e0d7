#!/usr/bin/env python
"""Forward + backward of both Euler integrations of the training step (animating_softmax_splating.py:579-580), two ways in one process:

  A  what TrainingSynthesis does by default: a negation, two EulerIntegration calls, their two float-atomic backwards, autograd's add;
  P  slr_sfs_amd.euler_integration_pair: one forward launch, the order-free 64-bit fixed-point backward (scale, walk, finish).

Shape [2,2,256,256]; step counts (30, 30) and (59, 59) in both directions; a smooth field (tools/blend_bench.py's) and a sink field
(converging on one point: every path ends in a few cells, the worst case for atomics on one address).  Per case: warm-up, then A and P
alternated (ROUNDS rounds of STEPS steps, device events around every block): the median with min - max; and -- unless --no-trace -- one
child process per variant under `rocprofv3 --kernel-trace` (nothing else traced) for kernel time and launches per step.  Prints one JSON
document (--out FILE writes it too).  A device is required: a timing has no CPU path.

    python tools/euler_pair_bench.py --out profiles/euler_pair_step.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPE = (2, 2, 256, 256)
CASES = {f"{flow}_n{n}": (flow, n) for flow in ("smooth", "sink") for n in (30, 59)}


def motion(flow):
    from blend_bench import smooth_motion
    B, _, H, W = SHAPE
    if flow == "smooth":
        return np.concatenate([smooth_motion(H, W, 21 + b) for b in range(B)])
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    one = np.stack([0.3 * (0.37 * W + 0.3 - x), 0.3 * (0.58 * H + 0.2 - y)])[None].astype(np.float32)
    return np.concatenate([one, -one])                       # sample 0 converges forwards, sample 1 backwards


def make_case(name):
    flow, n = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(2026)
    return dict(motion=torch.from_numpy(motion(flow)).cuda(), steps=torch.full((SHAPE[0],), n, dtype=torch.int64).cuda(),
                gf=torch.randn(*SHAPE, generator=g).cuda(), gp=torch.randn(*SHAPE, generator=g).cuda())


def step_two_calls(S, c):
    m = c["motion"].detach().requires_grad_(True)
    euler = S.EulerIntegration()
    flow_f, flow_p = euler(m, c["steps"]), euler(-m, c["steps"])
    torch.autograd.backward([flow_f, flow_p], [c["gf"], c["gp"]])
    return flow_f, flow_p, m.grad


def step_pair(S, c):
    m = c["motion"].detach().requires_grad_(True)
    flow_f, flow_p = S.euler_integration_pair(m, c["steps"], c["steps"])
    torch.autograd.backward([flow_f, flow_p], [c["gf"], c["gp"]])
    return flow_f, flow_p, m.grad


STEP = {"A": step_two_calls, "P": step_pair}


def run_only(S, args):
    c = make_case(args.case)
    for _ in range(args.steps):
        STEP[args.only](S, c)
    torch.cuda.synchronize()


def kernel_time_per_step(args, case, variant):
    """Sum of kernel time and number of launches per step from a child process that runs `trace_steps` steps and nothing else (the few
    fill kernels of make_case are part of the total: 4 launches in all, not per step)."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--case", case, "--steps", str(args.trace_steps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        per = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                per.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    n = args.trace_steps
    per = {k: v for k, v in per.items() if len(v) >= n}                          # (what runs every step)
    top = sorted(((sum(v) / n / 1e3, len(v) / n, k) for k, v in per.items()), reverse=True)
    return dict(kernel_us_per_step=round(sum(u for u, _, _ in top), 2), launches_per_step=round(sum(m for _, m, _ in top), 2),
                kernels=[dict(us_per_step=round(u, 2), launches_per_step=round(m, 2), kernel=k[:100]) for u, m, k in top])


def measure(S, args, name):
    c = make_case(name)
    res = {"shape": list(SHAPE), "flow": CASES[name][0], "steps_both_directions": CASES[name][1], "rounds": args.rounds,
           "steps_per_round": args.steps}
    a, p = step_two_calls(S, c), step_pair(S, c)
    res["flows_bit_equal"] = bool(torch.equal(a[0], p[0]) and torch.equal(a[1], p[1]))
    res["max_abs_gradient_difference_P_vs_A"] = float((a[2] - p[2]).abs().max())
    res["max_abs_gradient"] = float(a[2].abs().max())
    res["P_four_calls_bit_equal"] = bool(all(torch.equal(step_pair(S, c)[2], p[2]) for _ in range(4)))
    res["A_four_calls_bit_equal"] = bool(all(torch.equal(step_two_calls(S, c)[2], a[2]) for _ in range(4)))
    for v in "AP":
        for _ in range(args.warmup):
            STEP[v](S, c)
    torch.cuda.synchronize()
    times = {"A": [], "P": []}
    for _ in range(args.rounds):
        for v in "AP":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                STEP[v](S, c)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for v in "AP":
        t = times[v]
        res[f"{v}_step_us"] = round(float(np.median(t)), 2)
        res[f"{v}_step_us_min_max"] = [round(float(min(t)), 2), round(float(max(t)), 2)]
    res["P_over_A_step_time"] = round(res["P_step_us"] / res["A_step_us"], 4)
    res["apart_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["P"]) or min(times["P"]) > max(times["A"]))
    if not args.no_trace:
        for v in "AP":
            res[f"{v}_trace"] = kernel_time_per_step(args, name, v)
        res["P_over_A_kernel_time"] = round(res["P_trace"]["kernel_us_per_step"] / res["A_trace"]["kernel_us_per_step"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=20)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["A", "P"], help="(child of a trace) run this variant's steps and nothing else")
    ap.add_argument("--case", choices=list(CASES), default="smooth_n30")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/euler_pair_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/euler_pair_bench.py", "device": torch.cuda.get_device_name(0),
           "A": "-motion, two EulerIntegration calls, two float-atomic backwards, autograd's add",
           "P": "slr_sfs_amd.euler_integration_pair (one forward launch; scale, walk, finish backward)",
           "cases": {name: measure(S, args, name) for name in args.cases}}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
