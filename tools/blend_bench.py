#!/usr/bin/env python
"""Forward + backward of the splat half of the training step, all six gradients, two ways in one process:

  A  the composed chain (tests/test_gpu_gradients.py::test_training_step_chain_gradients from the displacement fields on, generalised to
     two feature / logit tensors): torch arithmetic around two 65-plane summation splats of the package's drop-in and autograd's mirror
     image of it -- the baseline;
  B  slr_sfs_amd.splat_blend.

Shapes: [2,64,256,256] with Euler steps (30, 59) of 60 and [1,64,768,1280] with step 30.  Per shape: warm-up, then A and B alternated
(A B A B ...: ROUNDS rounds of STEPS steps each, device events around every block), peak memory of a step of each, and -- unless
--no-trace -- one child process per variant under `rocprofv3 --kernel-trace --stats` for the sum of kernel time per step.  B's share of
8 TB/s is taken on the bytes the block needs: (3C + 7) planes forward, (6C + 13) backward.  Prints one JSON document (--out FILE writes it
too).  A device is required: there is no CPU path for a timing.

    python tools/blend_bench.py --out profiles/blend_train_step.json

--deterministic: the same measurement of B against D = ``splat_blend(..., deterministic=True)`` (rounds B D B D ..., one traced child each;
the default operator of the same build is the yardstick): step time and forward kernel time of D over B as they come out.

    python tools/blend_bench.py --deterministic --out profiles/blend_deterministic.json
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

NF = 60
SHAPES = {"train_2x64x256x256": ((2, 64, 256, 256), (30, 59)), "frame_1x64x768x1280": ((1, 64, 768, 1280), (30,))}
PEAK_BYTES_PER_S = 8.0e12


def smooth_motion(H, W, seed, amp=2.0):
    rng = np.random.default_rng(seed)
    p1, p2 = rng.uniform(0, 2 * np.pi, 2)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    u = amp * np.sin(2 * np.pi * (2 * x / W + y / H) + p1)
    v = amp * np.cos(2 * np.pi * (x / W - 1.5 * y / H) + p2)
    m = (x >= 0.35 * W).astype(np.float32)
    return np.stack([u * m, v * m])[None].astype(np.float32)


def make_case(S, shape, steps):
    N, C, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(2025)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    c = dict(start_fs=rn(N, C, H, W), z_start=0.7 * rn(N, 1, H, W), end_fs=rn(N, C, H, W), z_end=0.7 * rn(N, 1, H, W), go=rn(N, C, H, W))
    mo = torch.from_numpy(np.concatenate([smooth_motion(H, W, 21 + b) for b in range(N)])).cuda()
    t = torch.tensor(steps).cuda()
    euler = S.EulerIntegration()
    c["flow_f"], c["flow_p"] = euler(mo, t).contiguous(), euler(-mo, NF - t).contiguous()
    c["alpha"] = (1.0 - t.float() / float(NF)).contiguous()
    return c


NAMES = ("start_fs", "z_start", "flow_f", "end_fs", "z_end", "flow_p")


def step_chain(S, c, splat, mark=None):
    lv = {k: c[k].detach().requires_grad_(True) for k in NAMES}
    B, _, H, W = lv["start_fs"].shape
    a = c["alpha"].view(B, 1, 1, 1)
    ones = lv["start_fs"].new_ones((B, 1, H, W))
    Zf = torch.clamp(lv["z_start"] - lv["z_start"].max(), min=-20.0, max=20.0)
    ten_f = torch.cat([lv["start_fs"] * Zf.exp() * a, Zf.exp() * a], 1)
    gen_f = splat(tenInput=ten_f, tenFlow=lv["flow_f"], tenMetric=ones)
    ten_norm, gen = gen_f[:, -1:, :, :], gen_f[:, :-1, :, :]
    Zp = torch.clamp(lv["z_end"] - lv["z_end"].max(), min=-20.0, max=20.0)
    ten_p = torch.cat([lv["end_fs"] * Zp.exp() * (1 - a), Zp.exp() * (1 - a)], 1)
    gen_p = splat(tenInput=ten_p, tenFlow=lv["flow_p"], tenMetric=ones)
    ten_norm += gen_p[:, -1:, :, :]
    gen += gen_p[:, :-1, :, :]
    gen = gen / torch.clamp(ten_norm, min=1e-8)
    if mark:
        mark()
    gen.backward(c["go"])
    return gen, lv


def step_blend(S, c, splat, mark=None, deterministic=False):
    lv = {k: c[k].detach().requires_grad_(True) for k in NAMES}
    out = S.splat_blend(*[lv[k] for k in NAMES], c["alpha"], deterministic=deterministic)
    if mark:
        mark()
    out.backward(c["go"])
    return out, lv


def step_blend_det(S, c, splat, mark=None):
    return step_blend(S, c, splat, mark, deterministic=True)


STEP = {"A": step_chain, "B": step_blend, "D": step_blend_det}


def need_device():
    if not torch.cuda.is_available():
        raise SystemExit("tools/blend_bench.py: no ROCm device -- a timing has no CPU path")


MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: the trace's phase marker


def run_only(S, args):
    """The workload of a kernel trace: warm-up, then `steps` steps of one variant on one shape with phase markers in the stream -- ONE
    launch of the marker kernel in front of every forward, TWO in front of every backward, one behind the last step."""
    shape, steps = SHAPES[args.shape]
    c, splat = make_case(S, shape, steps), S.ModuleSoftsplat("summation")
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    fwd = lambda: S.softsplat.splat_normalize(tiny)
    bwd = lambda: (S.softsplat.splat_normalize(tiny), S.softsplat.splat_normalize(tiny))
    for _ in range(args.warmup):
        STEP[args.only](S, c, splat)
    torch.cuda.synchronize()
    for _ in range(args.steps):
        fwd()
        STEP[args.only](S, c, splat, bwd)
    fwd()
    torch.cuda.synchronize()


def kernel_time_per_step(args, shape_name, variant):
    """Kernel time per step of one variant, forward and backward apart, from a child process under rocprofv3: the kernels between the
    markers of run_only, in start order -- set-up and warm-up lie in front of the first marker and are not counted."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--shape", shape_name, "--steps", str(args.trace_steps),
               "--warmup", str(args.trace_warmup)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    n = args.trace_steps
    phase, run, total, count, per = None, 0, {"forward": 0, "backward": 0}, {"forward": 0, "backward": 0}, {}
    starts = 0
    for t0, t1, name in rows:
        if MARKER in name:
            run += 1
            continue
        if run:
            assert run in (1, 2), f"{run} markers in a row"
            phase = "forward" if run == 1 else "backward"
            starts += run == 1
            run = 0
        if phase:
            total[phase] += t1 - t0
            count[phase] += 1
            per.setdefault(name, []).append(t1 - t0)
    assert starts == n and run == 1, (starts, n, run)              # every step seen, the closing marker last
    top = sorted(((sum(v) / n / 1e3, len(v) / n, k) for k, v in per.items()), reverse=True)[:8]
    return dict(kernel_us_per_step=(total["forward"] + total["backward"]) / n / 1e3, forward_kernel_us=total["forward"] / n / 1e3,
                backward_kernel_us=total["backward"] / n / 1e3, launches_per_step=(count["forward"] + count["backward"]) / n,
                top=[dict(us_per_step=round(u, 2), launches_per_step=round(m, 2), kernel=k[:120]) for u, m, k in top])


def measure(S, args, shape_name):
    shape, steps = SHAPES[shape_name]
    N, C, H, W = shape
    c, splat = make_case(S, shape, steps), S.ModuleSoftsplat("summation")
    res = {"shape": list(shape), "euler_steps": list(steps), "rounds": args.rounds, "steps_per_round": args.steps}
    # the two compute the same thing (a looser statement than the tests': a sanity check of the workload, not a test)
    (oa, la), (ob, lb) = step_chain(S, c, splat), step_blend(S, c, splat)
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    res["max_rel_difference_B_vs_A"] = {"out": rel(ob.detach(), oa.detach()), **{k: rel(lb[k].grad, la[k].grad) for k in NAMES}}
    del oa, la, ob, lb
    for v in "AB":
        for _ in range(args.warmup):
            STEP[v](S, c, splat)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        STEP[v](S, c, splat)
        torch.cuda.synchronize()
        res[f"{v}_peak_bytes_of_a_step"] = int(torch.cuda.max_memory_allocated() - base)
        res[f"{v}_resident_bytes_before_the_step"] = int(base)
    times = {"A": [], "B": []}
    for _ in range(args.rounds):
        for v in "AB":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                STEP[v](S, c, splat)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for v in "AB":
        t = times[v]
        res[f"{v}_step_us_rounds"] = [round(x, 2) for x in t]
        res[f"{v}_step_us"] = round(float(np.median(t)), 2)
        res[f"{v}_step_us_spread"] = round(float(max(t) - min(t)), 2)
    P = N * H * W * 4
    res["bytes_needed"] = {"forward": (3 * C + 7) * P, "backward": (6 * C + 13) * P}
    res["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
    res["B_peak_below_A"] = bool(res["B_peak_bytes_of_a_step"] < res["A_peak_bytes_of_a_step"])
    if not args.no_trace:
        for v in "AB":
            res[f"{v}_trace"] = kernel_time_per_step(args, shape_name, v)
        kb = res["B_trace"]["kernel_us_per_step"]
        res["B_fraction_of_8TBps_on_needed_bytes"] = {k: round(res["bytes_needed"][k] / PEAK_BYTES_PER_S / (res["B_trace"][f"{k}_kernel_us"] * 1e-6), 4)
                                                      for k in ("forward", "backward")}
        res["B_kernel_time_below_A"] = bool(kb < res["A_trace"]["kernel_us_per_step"])
    return res


def measure_deterministic(S, args, shape_name):
    """B (default) and D (deterministic) alternated in one process; D's cost as a ratio to B, whatever it is."""
    shape, steps = SHAPES[shape_name]
    c, splat = make_case(S, shape, steps), None
    res = {"shape": list(shape), "euler_steps": list(steps), "rounds": args.rounds, "steps_per_round": args.steps}
    (ob, lb), (od, ld) = step_blend(S, c, splat), step_blend_det(S, c, splat)
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    res["max_rel_difference_D_vs_B"] = {"out": rel(od.detach(), ob.detach()), **{k: rel(ld[k].grad, lb[k].grad) for k in NAMES}}
    outs = [step_blend_det(S, c, splat)[0].detach() for _ in range(4)]
    res["D_four_calls_bit_equal"] = bool(all(torch.equal(o, od.detach()) for o in outs))
    res["D_fallback_count"] = int(S.training.splat_blend_fallback_count(c["start_fs"]).item())
    del ob, lb, od, ld, outs
    for v in "BD":
        for _ in range(args.warmup):
            STEP[v](S, c, splat)
    torch.cuda.synchronize()
    times = {"B": [], "D": []}
    for _ in range(args.rounds):
        for v in "BD":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                STEP[v](S, c, splat)
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for v in "BD":
        t = times[v]
        res[f"{v}_step_us_rounds"] = [round(x, 2) for x in t]
        res[f"{v}_step_us"] = round(float(np.median(t)), 2)
        res[f"{v}_step_us_min_max"] = [round(float(min(t)), 2), round(float(max(t)), 2)]
    res["D_over_B_step_time"] = round(res["D_step_us"] / res["B_step_us"], 4)
    if not args.no_trace:
        for v in "BD":
            res[f"{v}_trace"] = kernel_time_per_step(args, shape_name, v)
        res["D_over_B_forward_kernel_time"] = round(res["D_trace"]["forward_kernel_us"] / res["B_trace"]["forward_kernel_us"], 4)
    else:
        res["forward_kernel_time"] = "not measured (--no-trace)"
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=20)
    ap.add_argument("--trace-warmup", type=int, default=3)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--deterministic", action="store_true", help="B against D = splat_blend(..., deterministic=True) instead of A against B")
    ap.add_argument("--only", choices=["A", "B", "D"], help="(child of a trace) run this variant's steps and nothing else")
    ap.add_argument("--shape", choices=list(SHAPES), default="train_2x64x256x256")
    args = ap.parse_args()
    if not args.only:
        assert args.rounds >= 5 and args.steps >= 50, "at least 5 alternated rounds of at least 50 steps"
    need_device()
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    if args.deterministic:
        doc = {"tool": "tools/blend_bench.py --deterministic", "device": torch.cuda.get_device_name(0),
               "B": "slr_sfs_amd.splat_blend", "D": "slr_sfs_amd.splat_blend(..., deterministic=True)",
               "cases": {name: measure_deterministic(S, args, name) for name in args.shapes}}
    else:
        doc = {"tool": "tools/blend_bench.py", "device": torch.cuda.get_device_name(0),
               "A": "composed chain on ModuleSoftsplat('summation') + torch autograd", "B": "slr_sfs_amd.splat_blend",
               "cases": {name: measure(S, args, name) for name in args.shapes}}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
