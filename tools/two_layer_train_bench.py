#!/usr/bin/env python
"""The two-layer model's head and its whole training iteration, measured in one process:

  head       composite + alpha losses, forward + backward, at [2,.,256,256] and [16,.,256,256], two ways from the same inputs:
             A  the definition of tests/two_layer_f64.py from torch operators in float32 on the device, torch autograd;
             B  slr_sfs_amd.layer_composite + alpha_losses (csrc/layers.hip).
  iteration  one iteration through slr_sfs_amd.Trainer(TwoLayerTrainingModel) at [2,3,256,256] with the reference's widths and the
             options of train_alpha_finetuneBG_finetuneFluid_v2.sh, with (L) and without (S) the reference's dropped pair of encoder calls.

Warm-up, then the two sides alternated (ROUNDS rounds of STEPS steps, device events around every block of steps): the median with
min - max; a difference is claimed only where it exceeds the spread of the rounds.  Unless --no-trace, one child process per variant
under `rocprofv3 --kernel-trace` for the launches and the sum of kernel time of a step, and each new kernel's time against its bytes at
8 TB/s.  No threshold: the numbers are recorded.  Prints one JSON document (--out FILE writes it too).  A device is required.

    python tools/two_layer_train_bench.py --out profiles/two_layer_train_step.json

--v1: the same rules for what train_alpha_finetuneBG_finetuneFluid_v1.sh adds:

  alpha0     blend_alpha0 forward + backward at [2,.,256,256] and [16,.,256,256]: A tests/two_layer_v1_f64.py's definition from torch
             operators, B slr_sfs_amd.blend_alpha0.
  splat      the C = 1 splat_blend call of the alpha plane (shared c0 logits, no clamp, no maximum) against the C = 64 call of the
             features, forward + backward, at [2,.,256,256] on Euler flows t = 30 / 30: device time, and kernel time from the traces.
  iteration  one iteration through Trainer with TwoLayerAlpha0TrainingModel (V1) against TwoLayerTrainingModel (V2) of the same build,
             and the C = 1 call's share of the V1 iteration's kernel time.

    python tools/two_layer_train_bench.py --v1 --out profiles/two_layer_v1_train_step.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import two_layer_f64 as D  # noqa: E402
import two_layer_v1_f64 as V  # noqa: E402

HW, PEAK_BW = 256, 8.0e12
# planes of N H W floats each new kernel has to read and write once (the stencil's neighbours come from the cache)
PLANES = {"layer_composite_forward_kernel": 8 + 10, "layer_composite_backward_kernel": 8 + 9 + 8, "alpha_losses_forward_kernel": 7 + 2,
          "alpha_losses_backward_kernel": 7 + 3, "blend_alpha0_forward_kernel": 4 + 1, "blend_alpha0_backward_kernel": 5 + 2}
MARKER = "slr::normalize_kernel("        # a kernel of the library that no variant launches: brackets the traced steps
GRAD = (0.7, 1.3, 2.1, 0.4)


def head_stepper(S, variant, N):
    d = {k: v.cuda() for k, v in D.head_inputs(N, HW, HW, seed=N, dtype=torch.float32).items()}
    gen = torch.Generator().manual_seed(3)
    go = [torch.randn(N, 3, HW, HW, generator=gen).cuda() for _ in range(3)]
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("fluid_raw", "bg_raw", "fluid_alpha_raw", "a_start")}
    comp, alph = (S.layer_composite, S.alpha_losses) if variant == "B" else (D.layer_composite, D.alpha_losses)

    def run():
        for t in leaves.values():
            t.grad = None
        a = leaves["a_start"]
        pred, fluid, bg, _ = comp(leaves["fluid_raw"], leaves["bg_raw"], leaves["fluid_alpha_raw"], a[:, 0:1].contiguous())
        losses, _, _ = alph(a, d["mask_rock"], d["small_motion_alpha"], d["warped_alpha"], d["norm"], leaves["fluid_alpha_raw"])
        total = (pred * go[0]).sum() + (fluid * go[1]).sum() + (bg * go[2]).sum()
        for w, n in zip(GRAD, D.LOSS_NAMES):
            total = total + losses[n] * w
        total.backward()
        return total
    return run


def alpha0_stepper(S, variant, N):
    """blend_alpha0 forward + backward with gradients reaching c0 and both losses."""
    a, rock, sma = (t.cuda() for t in V.alpha0_inputs(N, HW, HW, seed=N, dtype=torch.float32))
    go = torch.randn(N, 1, HW, HW, generator=torch.Generator().manual_seed(3)).cuda()
    a.requires_grad_(True)
    op = S.blend_alpha0 if variant == "B" else V.blend_alpha0

    def run():
        a.grad = None
        c0, losses = op(a, rock, sma, 0.25)
        total = (c0 * go).sum() + losses["FluidRegionLoss"] * 3.0 + losses["RockRegionLoss"] * 30.0
        total.backward()
        return total
    return run


def splat_stepper(S, C):
    """One splat_blend call forward + backward at [2,C,256,256] on Euler flows t = 30 / 30: C = 1 as the v1 model makes it for the alpha
    plane (one c0 tensor as both directions' logits, clamp_z=None, subtract_max=False), C = 64 as it makes it for the features."""
    gen = torch.Generator().manual_seed(8)
    y, x = torch.meshgrid(torch.arange(HW, dtype=torch.float32), torch.arange(HW, dtype=torch.float32), indexing="ij")
    motion = torch.stack([0.6 * torch.sin(y / 40 + x / 70), 0.4 * torch.cos(x / 35 - y / 60)])[None].repeat(2, 1, 1, 1).cuda().contiguous()
    euler, steps = S.EulerIntegration(None), torch.tensor([30, 30]).cuda()
    with torch.no_grad():
        flow_f, flow_p = euler(motion, steps).contiguous(), euler(-motion, steps).contiguous()
    alpha = torch.tensor([0.5, 0.5]).cuda()
    vs, ve = (torch.randn(2, C, HW, HW, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    go = torch.randn(2, C, HW, HW, generator=gen).cuda()
    ff, fp = flow_f.clone().requires_grad_(True), flow_p.clone().requires_grad_(True)
    if C == 1:
        z = [torch.rand(2, 1, HW, HW, generator=gen).cuda().requires_grad_(True)] * 2
        kw = dict(clamp_z=None, subtract_max=False)
    else:
        z, kw = [(0.7 * torch.randn(2, 1, HW, HW, generator=gen)).cuda().requires_grad_(True) for _ in range(2)], {}

    def run():
        for t in (vs, ve, ff, fp, *z):
            t.grad = None
        out = S.splat_blend(vs, z[0], ff, ve, z[1], fp, alpha, **kw)
        out.backward(go)
        return out
    return run


def iteration_stepper(S, literal, v1=False):
    import losses_fixture as LF
    opts = (V.options if v1 else D.options)(W=HW, ngf=64, out_channel=65, ndf=64, discriminator_losses="pix2pixHD")
    vgg = S.losses.load_vgg19_state_dict(S.losses.VGG19Features(), LF.vgg19_state_dict())
    torch.manual_seed(5)
    model = (S.TwoLayerAlpha0TrainingModel if v1 else S.TwoLayerTrainingModel)(opts, vgg, literal_encoder_calls=literal)
    trainer = S.Trainer(model, opts).cuda().train()
    gen = torch.Generator().manual_seed(6)
    y, x = torch.meshgrid(torch.arange(HW, dtype=torch.float32), torch.arange(HW, dtype=torch.float32), indexing="ij")
    base = torch.stack([torch.sin(x / 23 + c) * torch.cos(y / 31 - c) for c in range(3)])
    img = [(0.7 * base + 0.25 * torch.randn(2, 3, HW, HW, generator=gen)).clamp(-1, 1).cuda() for _ in range(4)]
    motion = torch.stack([0.6 * torch.sin(y / 40 + x / 70), 0.4 * torch.cos(x / 35 - y / 60)])[None].repeat(2, 1, 1, 1).cuda().contiguous()
    batch = {"images": img[:3], "mean_video": [img[3]], "motions": motion, "mask_rock": (y < 90).float()[None, None].repeat(2, 1, 1, 1).cuda(),
             "index": torch.tensor([[0, 30, 59], [3, 10, 40]]).cuda()}

    def run():
        return trainer(iter([batch]))[0]["Total Loss"]
    return run


def stepper(S, name):
    kind, variant, *n = name.split("_")
    if kind == "alpha0":
        return alpha0_stepper(S, variant, int(n[0]))
    if kind == "splat":
        return splat_stepper(S, int(variant))
    if kind == "iteration" and variant in ("V1", "V2"):
        return iteration_stepper(S, True, v1=variant == "V1")
    return head_stepper(S, variant, int(n[0])) if kind == "head" else iteration_stepper(S, variant == "L")


def run_only(S, args):
    run = stepper(S, args.only)
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.trace_warmup):
        run()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.trace_steps):
        run()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_step(args, name, pixels):
    """Launches and kernel time of one step of one variant, from a child process under rocprofv3 (kernel trace only)."""
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
    res = dict(kernel_us_per_step=round(total, 2), launches_per_step=round(sum(len(v) for v in per.values()) / n, 2))
    new = {}
    for kernel, planes in PLANES.items():
        v = [t for k, ts in per.items() if kernel in k for t in ts]
        if v:
            us, by = sum(v) / len(v) / 1e3, 4.0 * planes * pixels
            new[kernel] = dict(us_per_launch=round(us, 2), launches_per_step=round(len(v) / n, 2), MB=round(by / 1e6, 2),
                               TBs=round(by / us / 1e6, 3), share_of_8TBs=round(by / us / 1e-6 / PEAK_BW, 4))
    if new:
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


def main_v1(S, args):
    doc = {"tool": "tools/two_layer_train_bench.py --v1", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "steps_per_round": args.steps,
           "A": "tests/two_layer_v1_f64.py's blend_alpha0 from torch operators, float32 on the device, torch autograd",
           "B": "slr_sfs_amd.blend_alpha0 (csrc/layers.hip)",
           "C1": "splat_blend forward + backward at [2,1,256,256], one c0 tensor as both directions' logits, clamp_z=None, subtract_max=False",
           "C64": "splat_blend forward + backward at [2,64,256,256], two logit planes, the default clamp and maximum",
           "V1": "Trainer(TwoLayerAlpha0TrainingModel), one iteration with the discriminator, the v1 script's weights",
           "V2": "Trainer(TwoLayerTrainingModel) of the same build, the v2 script's weights"}
    for N in (2, 16):
        names = {"A": f"alpha0_A_{N}", "B": f"alpha0_B_{N}"}
        runs = {k: stepper(S, v) for k, v in names.items()}
        a, b = float(runs["A"]()), float(runs["B"]())
        r = alternate(runs, args)
        r["B_vs_A_total"] = abs(b - a) / abs(a)
        if not args.no_trace:
            for k, v in names.items():
                r[f"{k}_trace"] = kernel_time_per_step(args, v, N * HW * HW)
        doc[f"alpha0_{N}x256x256"] = r
        del runs
        torch.cuda.empty_cache()
    for key, names in (("splat_2x256x256_euler_30_30", {"C64": "splat_64", "C1": "splat_1"}),
                       ("iteration_2x3x256x256", {"V2": "iteration_V2", "V1": "iteration_V1"})):
        runs = {k: stepper(S, v) for k, v in names.items()}
        r = alternate(runs, args)
        if not args.no_trace:
            for k, v in names.items():
                r[f"{k}_trace"] = kernel_time_per_step(args, v, 2 * HW * HW)
        doc[key] = r
        del runs
        torch.cuda.empty_cache()
    if not args.no_trace:
        c1 = doc["splat_2x256x256_euler_30_30"]["C1_trace"]["kernel_us_per_step"]
        v1, v2 = (doc["iteration_2x3x256x256"][f"{k}_trace"]["kernel_us_per_step"] for k in ("V1", "V2"))
        doc["second_call"] = {"C1_kernel_us": c1, "V1_iteration_kernel_us": v1, "share_of_V1_iteration_kernel_time": round(c1 / v1, 5),
                              "V1_minus_V2_iteration_kernel_us": round(v1 - v2, 2),
                              "note": "the share takes the C = 1 call alone on the Euler 30 / 30 flows; V1 - V2 also holds blend_alpha0 "
                                      "and the 65th plane the V2 splat carries"}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


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
    ap.add_argument("--v1", action="store_true", help="measure what the v1 script adds: blend_alpha0, the C = 1 splat call, the v1 iteration")
    ap.add_argument("--only", help="(child of a trace) run this variant's steps and nothing else: head_A_2, head_B_16, iteration_L, ...")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/two_layer_train_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    if args.v1:
        return main_v1(S, args)
    doc = {"tool": "tools/two_layer_train_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "steps_per_round": args.steps,
           "A": "tests/two_layer_f64.py's definition from torch operators, float32 on the device, torch autograd",
           "B": "slr_sfs_amd.layer_composite + alpha_losses (csrc/layers.hip)",
           "L": "Trainer(TwoLayerTrainingModel(literal_encoder_calls=True)), one iteration with the discriminator",
           "S": "the same with literal_encoder_calls=False"}
    for N in (2, 16):
        names = {"A": f"head_A_{N}", "B": f"head_B_{N}"}
        runs = {k: stepper(S, v) for k, v in names.items()}
        a, b = float(runs["A"]()), float(runs["B"]())
        r = alternate(runs, args)
        r["B_vs_A_total"] = abs(b - a) / abs(a)
        if not args.no_trace:
            for k, v in names.items():
                r[f"{k}_trace"] = kernel_time_per_step(args, v, N * HW * HW)
        doc[f"head_{N}x256x256"] = r
        del runs
        torch.cuda.empty_cache()
    runs = {"L": stepper(S, "iteration_L"), "S": stepper(S, "iteration_S")}
    r = alternate(runs, args)
    if not args.no_trace:
        for k in runs:
            r[f"{k}_trace"] = kernel_time_per_step(args, f"iteration_{k}", 2 * HW * HW)
    doc["iteration_2x3x256x256"] = r
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
