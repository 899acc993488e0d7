#!/usr/bin/env python
"""Whole training iterations of joint training (slr_sfs_amd.Trainer around JointTrainingModel, --train_motion) at [2, 3, 256, 256] with
the reference's widths, the motion network at nf = 32, ndf = 64 and the Euler steps t = (30, 59) of a 60-frame clip, three ways in one
process on models of the same state, all with deterministic=True:

  plain     TrainingModel on the ground-truth motion (the parent's iteration);
  frozen    JointTrainingModel after freeze_motion(): the difference to plain is the motion network's forward and its loss;
  unfrozen  JointTrainingModel whose motion network learns: the difference to frozen is the order-free Euler gradient, the motion
            network's backward and its share of the optimiser step.

Warm-up, then the three alternated (ROUNDS rounds of STEPS iterations, device events around every block): median, min and max of the
rounds per iteration.  Unless --no-trace, one child process per variant under `rocprofv3 --kernel-trace` (kernel trace only): launches
and summed kernel time per iteration.  The VGG19 of the content loss has random weights.  The Euler step on its own (forward + backward
of the pair operator against the parent's path) is tools/euler_pair_bench.py's.  Prints one JSON document (--out FILE writes it too).
A device is required.

    python tools/joint_train_bench.py --out profiles/joint_train_step.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import train_step_bench as TB  # noqa: E402

VARIANTS = ("plain", "frozen", "unfrozen")


def options(joint):
    opt = TB.options()
    if joint:
        for k, v in dict(train_motion=True, motion_model_type="SPADE_unet_mask_motion", motion_norm_G="sync:spectral_instance",
                         use_mask_as_motion_input=True, use_hint_as_motion_input=True, motionH=TB.W, motionW=TB.W, div_flow=1.0,
                         motion_losses=["10.0_EndPointError"]).items():
            setattr(opt, k, v)
    return opt


def make(S, variant):
    torch.manual_seed(1234)
    if variant == "plain":
        model = S.TrainingModel(options(False), S.losses.VGG19Features(), deterministic=True)
    else:
        model = S.JointTrainingModel(options(True), S.losses.VGG19Features(), deterministic=True)
        if variant == "frozen":
            model.freeze_motion()
    return S.Trainer(model, options(variant != "plain")).cuda().train()


def batch():
    b = TB.batch()
    y, x = torch.meshgrid(torch.arange(TB.W), torch.arange(TB.W), indexing="ij")
    lattice = ((x % 32 == 16) & (y % 32 == 16)).float().cuda()
    b["hints"] = (b["motions"] * lattice).contiguous()
    return b


def run_only(S, args):
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    trainer, b = make(S, args.only), batch()
    for _ in range(args.warmup):
        trainer(iter([b]))
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        trainer(iter([b]))
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=2)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=VARIANTS, help="(child of a trace) run this variant's iterations and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/joint_train_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/joint_train_bench.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "shape": [TB.B, 3, TB.W, TB.W], "ndf": 64, "motion_nf": 32, "euler_steps": [TB.T[1] - TB.T[0], TB.T[2] + 1 - TB.T[1]],
           "rounds": args.rounds, "steps_per_round": args.steps,
           "step_ms": "device events around a block of iterations, per iteration: what a training loop waits for, host launch cost included"}
    what = {"plain": "TrainingModel(deterministic=True) on the ground-truth motion", "frozen": "JointTrainingModel after freeze_motion()",
            "unfrozen": "JointTrainingModel, the motion network learns"}
    trainers, b = {v: make(S, v) for v in VARIANTS}, batch()
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
    for v in VARIANTS:
        doc[v] = dict(TB.summary(times[v]), what=what[v])
    doc["fallback_count"] = int(S.training.splat_blend_fallback_count(torch.empty(TB.B, 64, TB.W, TB.W, device="cuda")).item())
    for a, c in (("frozen", "plain"), ("unfrozen", "frozen")):
        doc[f"{a}_over_{c}"] = round(doc[a]["step_ms"] / doc[c]["step_ms"], 4)
        doc[f"{a}_and_{c}_inside_the_spread_of_the_rounds"] = bool(max(times[c]) >= min(times[a]) and max(times[a]) >= min(times[c]))
    if not args.no_trace:
        del trainers
        torch.cuda.empty_cache()
        me = os.path.abspath(__file__)
        for v in VARIANTS:
            TB.__file__, keep = me, TB.__file__             # (trace() starts `this file --only variant`)
            try:
                doc[v]["trace"] = TB.trace(args, v)
            finally:
                TB.__file__ = keep
    else:
        doc["kernel_time"] = "not measured (--no-trace)"
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
