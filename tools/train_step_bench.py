#!/usr/bin/env python
"""One whole training iteration (slr_sfs_amd.Trainer: generator forward, both losses, backward, optimizer_G, the discriminator step,
optimizer_D) at [2, 3, 256, 256] with the reference's widths, ndf = 64 and the Euler steps t = (30, 59) of a 60-frame clip, two ways in
one process on models of the same state:

  deferred   the generator's gradients to weight_orig by the list-wide pair (slr_spectral_weight_grad_multi): two launches per group
             run, so six per generator backward (the encoder runs twice, the decoder once);
  per_layer  the per-tensor pair (slr_spectral_weight_grad): two launches per used tensor per run.

Nobody measured an iteration before: no figure is fixed here, the per-layer iteration of the same build and process is the yardstick.
Warm-up, then the two alternated (ROUNDS rounds of STEPS iterations, device events around every block): median, min and max of the
rounds per iteration, and the peak memory of one iteration of each.  Unless --no-trace, one child process per variant under
`rocprofv3 --kernel-trace` (kernel trace only): launches and summed kernel time per iteration, and those of the gradient pair's
kernels.  The VGG19 of the content loss has random weights (its cost does not depend on them).  Prints one JSON document (--out FILE
writes it too).  A device is required.

    python tools/train_step_bench.py --out profiles/train_step.json

--deterministic: the deferred iteration of ``TrainingModel(..., deterministic=True)`` against the deferred iteration of the default model,
alternated the same way (the default model of the same build and process is the yardstick; the ratio is reported as it comes out).

    python tools/train_step_bench.py --deterministic --out profiles/train_step_deterministic.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("deferred", "per_layer")
DET_VARIANTS = ("default", "deterministic")
MARKER = "slr::normalize_kernel("        # a kernel of the library that an iteration does not launch: brackets the traced iterations
PAIR = ("slr::spectral_dot_multi_kernel", "slr::spectral_grad_multi_kernel", "slr::spectral_dot_kernel", "slr::spectral_grad_kernel")
B, W, T = 2, 256, (0, 30, 59)


def options():
    return types.SimpleNamespace(refine_model_type="resnet_256W8UpDown64_de_resnet_pconv2_nonorm", pconv="pconv_pbn_woresbias",
                                 norm_G="sync:spectral_batch", normalize_image=True, train_Z=True, losses=["1.0_l1", "10.0_content"],
                                 discriminator_losses="pix2pixHD", ndf=64, ngf=64, out_channel=64, W=W, Z_model="encoder")


def make(S, deferred, deterministic=False):
    torch.manual_seed(1234)
    model = S.TrainingModel(options(), S.losses.VGG19Features(), deterministic=deterministic)
    trainer = S.Trainer(model, options()).cuda().train()
    model.defer_weight_grad(deferred)
    return trainer


def batch():
    gen = torch.Generator().manual_seed(99)
    y, x = torch.meshgrid(torch.arange(W, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([torch.sin(x / 23 + c) * torch.cos(y / 31 - c) for c in range(3)])
    images = [(0.7 * base + 0.2 * torch.randn(B, 3, W, W, generator=gen)).clamp(-1, 1).cuda() for _ in range(3)]
    motion = torch.stack([0.6 * torch.sin(y / 40 + x / 70), 0.4 * torch.cos(x / 50 - y / 60)])[None].repeat(B, 1, 1, 1).contiguous().cuda()
    return {"images": images, "motions": motion, "index": torch.tensor([T] * B).cuda()}


def run_only(S, args):
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    trainer, b = make(S, args.only != "per_layer", args.only == "deterministic"), batch()
    for _ in range(args.warmup):
        trainer(iter([b]))
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        trainer(iter([b]))
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def trace(args, variant):
    """Launches and kernel time of one iteration of one variant, from a child process under rocprofv3 (kernel trace only)."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--steps", str(args.trace_steps), "--warmup", str(args.trace_warmup)]
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
    pair = {k: v for k, v in per.items() if k.startswith(PAIR)}
    top = sorted((dict(us_per_iteration=round(sum(v) / n / 1e3, 2), launches_per_iteration=round(len(v) / n, 2), kernel=k[:120]) for k, v in per.items()),
                 key=lambda r: -r["us_per_iteration"])
    return dict(kernel_us_per_iteration=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
                launches_per_iteration=round(sum(len(v) for v in per.values()) / n, 2),
                gradient_pair=dict(kernel_us_per_iteration=round(sum(sum(v) for v in pair.values()) / n / 1e3, 2),
                                   launches_per_iteration=round(sum(len(v) for v in pair.values()) / n, 2),
                                   kernels={k.split("(")[0]: round(len(v) / n, 2) for k, v in pair.items()}),
                top=top[:8])


def summary(t):
    return dict(step_ms=round(float(np.median(t)), 3), step_ms_min_max=[round(min(t), 3), round(max(t), 3)], step_ms_rounds=[round(x, 3) for x in t])


def main_deterministic(S, args):
    doc = {"tool": "tools/train_step_bench.py --deterministic", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shape": [B, 3, W, W], "ndf": 64, "euler_steps": [T[1] - T[0], T[2] + 1 - T[1]],
           "default": "TrainingModel(...): the default forward splat", "deterministic": "TrainingModel(..., deterministic=True)",
           "rounds": args.rounds, "steps_per_round": args.steps,
           "step_ms": "device events around a block of iterations, per iteration: what a training loop waits for, host launch cost included"}
    trainers, b = {v: make(S, True, v == "deterministic") for v in DET_VARIANTS}, batch()
    times = {v: [] for v in DET_VARIANTS}
    for t in trainers.values():
        for _ in range(args.warmup):
            t(iter([b]))
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v, t in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                t(iter([b]))
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) / args.steps)
    for v in DET_VARIANTS:
        doc[v] = dict(summary(times[v]), what=doc[v])
    feats = torch.empty(B, 64, W, W, device="cuda")
    doc["fallback_count"] = int(S.training.splat_blend_fallback_count(feats).item())
    doc["deterministic_over_default"] = round(doc["deterministic"]["step_ms"] / doc["default"]["step_ms"], 4)
    doc["difference_inside_the_spread_of_the_rounds"] = bool(max(times["default"]) >= min(times["deterministic"]) and max(times["deterministic"]) >= min(times["default"]))
    if not args.no_trace:
        del trainers
        torch.cuda.empty_cache()
        for v in DET_VARIANTS:
            doc[v]["trace"] = trace(args, v)
    else:
        doc["kernel_time"] = "not measured (--no-trace)"
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
    ap.add_argument("--trace-steps", type=int, default=3)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--deterministic", action="store_true", help="the deterministic forward splat against the default one (both deferred)")
    ap.add_argument("--only", choices=VARIANTS + DET_VARIANTS, help="(child of a trace) run this variant's iterations and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_step_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    from slr_sfs_amd import spectral
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    if args.deterministic:
        return main_deterministic(S, args)
    doc = {"tool": "tools/train_step_bench.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shape": [B, 3, W, W], "ndf": 64, "euler_steps": [T[1] - T[0], T[2] + 1 - T[1]],
           "deferred": "slr_spectral_weight_grad_multi: one pair of launches per group run (six launches per generator backward)",
           "per_layer": "slr_spectral_weight_grad: one pair of launches per used tensor per run",
           "rounds": args.rounds, "steps_per_round": args.steps,
           "step_ms": "device events around a block of iterations, per iteration: what a training loop waits for, host launch cost included"}
    trainers, b = {v: make(S, v == "deferred") for v in VARIANTS}, batch()
    used = {name: len(spectral.group_of(net).leaves) for name, net in (("encoder", trainers["deferred"].model.encoder),
                                                                        ("projector", trainers["deferred"].model.projector))}
    doc["normalised_tensors"] = dict(used, per_generator_backward=2 * used["encoder"] + used["projector"])
    doc["gradient_pair_launches_derived"] = dict(deferred=2 * 3, per_layer=2 * (2 * used["encoder"] + used["projector"]),
                                                 note="two per group run against two per used tensor per run: derived, not measured")
    times = {v: [] for v in VARIANTS}
    for t in trainers.values():
        for _ in range(args.warmup):
            t(iter([b]))
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v, t in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                t(iter([b]))
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) / args.steps)
    for v, t in trainers.items():
        doc[v] = dict(summary(times[v]), what=doc[v])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t(iter([b]))
        torch.cuda.synchronize()
        doc[v]["peak_memory_MiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    doc["memory_note"] = "peak of one iteration with both trainers (parameters, optimiser states) resident"
    doc["deferred_over_per_layer"] = round(doc["deferred"]["step_ms"] / doc["per_layer"]["step_ms"], 4)
    doc["deferred_faster_by_more_than_the_spread"] = bool(min(times["per_layer"]) > max(times["deferred"]))
    doc["per_layer_faster_by_more_than_the_spread"] = bool(min(times["deferred"]) > max(times["per_layer"]))
    if not args.no_trace:
        del trainers
        torch.cuda.empty_cache()
        for v in VARIANTS:
            doc[v]["trace"] = trace(args, v)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
