#!/usr/bin/env python
"""What spectral normalisation of the generator costs per training iteration, over the generator's real list of normalised tensors
(TrainableDecoderPconv2 + TrainableEncoderWithZ at ngf = 64 with spectral=True; the tool prints the count), two ways in one process on
tensors of the same shapes:

  A  the parametrisation composed per layer from torch operators: adversarial.spectral_weight's formula (power iteration and 1 / sigma),
     weight_orig * scale, the existing preparation entries for the forward buffer and -- after flip / transpose / contiguous -- the
     backward buffer, and torch autograd from the gradient at the effective weight back to weight_orig;
  B  slr_sfs_amd.SpectralGroup.run() (slr_spectral_sigma + slr_conv_prep_scaled_multi: four launches for the list) and one
     slr_spectral_weight_grad per tensor (csrc/spectral.hip, csrc/conv.hip).

One "step" is one forward's normalisation of every tensor plus the gradient to every weight_orig from a given gradient at the effective
weight -- what a training iteration adds to the convolutions themselves.  Warm-up, then A and B alternated (ROUNDS rounds of STEPS steps,
device events around every block of steps): median, min and max of the rounds per step.  Unless --no-trace, one child process per variant
under `rocprofv3 --kernel-trace` (kernel trace only): launches and summed kernel time per step with the largest kernels, and a third
child that runs slr_spectral_sigma on the list's largest matrix alone ([256, 2304]) -- the summed time of its (up to three) kernels
against the bytes it reads (W twice).
Then one decoder training step (forward + backward) at [2, 64, 256, 256] with spectral=False and spectral=True, alternated the same way.
No target figure: what comes out is recorded.  Prints one JSON document (--out FILE writes it too).  A device is required.

    python tools/spectral_bench.py --out profiles/spectral_step.json
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

VARIANTS = ("A", "B")
MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: brackets the traced steps
LARGEST = (256, 2304)


def leaves_of(S):
    """The normalised layers of the generator, on the device, with a gradient at the effective weight each."""
    torch.manual_seed(1234)
    nets = [S.TrainableDecoderPconv2(spectral=True).cuda().train(), S.TrainableEncoderWithZ(spectral=True).cuda().train()]
    group = S.SpectralGroup(nets)
    grads = [1e-2 * torch.randn_like(m.weight_orig) for m in group.leaves]
    return nets, group, grads


def step_A(S, leaves, grads):
    from slr_sfs_amd import _lib
    for m, dW in zip(leaves, grads):
        w = m.weight_orig
        inv = S.spectral_weight(w, m.weight_u, m.weight_v, True)
        w_eff = w * inv
        if w.dim() == 4:
            conv = "conv3x3" if w.shape[2] == 3 else "conv1x1"
            nbytes = getattr(_lib.lib(), f"slr_{conv}_weight_bytes")
            with torch.no_grad():
                fwd = torch.empty(int(nbytes(w.shape[0], w.shape[1])), dtype=torch.uint8, device=w.device)
                _lib.call(f"slr_{conv}_f32_weights", w.device, w_eff, fwd, w.shape[0], w.shape[1])
                wb = w_eff.flip(2, 3).transpose(0, 1).contiguous()
                bwd = torch.empty(int(nbytes(w.shape[1], w.shape[0])), dtype=torch.uint8, device=w.device)
                _lib.call(f"slr_{conv}_f32_weights", w.device, wb, bwd, w.shape[1], w.shape[0])
        w.grad = None
        w_eff.backward(dW)


def step_B(S, group, grads):
    state = group.run()
    for m, dW in zip(group.leaves, grads):
        sn = m._sn
        m.weight_orig.grad = sn.weight_grad(dW, m.weight_orig)
        object.__setattr__(m, "_sn", None)
    return state


def list_shape(group):
    n = [m.weight_orig.numel() for m in group.leaves]
    shapes = [tuple(m.weight_orig.shape) for m in group.leaves]
    return dict(tensors=len(n), convolutions=len(group.convs), linears=len(n) - len(group.convs), elements=int(sum(n)),
                smallest=list(min(shapes, key=lambda s: int(np.prod(s)))), largest=list(max(shapes, key=lambda s: int(np.prod(s)))))


def run_only(S, args):
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    if args.only == "largest":
        gen = torch.Generator().manual_seed(5)
        W = (torch.randn(*LARGEST, generator=gen) / LARGEST[1] ** 0.5).cuda()
        u, v = torch.nn.functional.normalize(torch.randn(LARGEST[0]), dim=0).cuda(), torch.nn.functional.normalize(torch.randn(LARGEST[1]), dim=0).cuda()
        step = lambda: S.spectral_sigma([W], [u], [v], training=True)          # noqa: E731
    else:
        nets, group, grads = leaves_of(S)
        step = (lambda: step_A(S, group.leaves, grads)) if args.only == "A" else (lambda: step_B(S, group, grads))
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        step()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def trace(args, variant):
    """Launches and kernel time of one step of one variant, from a child process under rocprofv3 (kernel trace only)."""
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
    top = sorted((dict(us_per_step=round(sum(v) / n / 1e3, 2), launches_per_step=round(len(v) / n, 2), kernel=k[:120]) for k, v in per.items()),
                 key=lambda r: -r["us_per_step"])
    return dict(kernel_us_per_step=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
                launches_per_step=round(sum(len(v) for v in per.values()) / n, 2), top=top[:6])


def alternate(args, steps, fns):
    """fns: name -> callable; warm-up, then the callables alternated: per-step times of every round, in microseconds."""
    times = {k: [] for k in fns}
    for f in fns.values():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / steps)
    return times


def summary(t):
    return dict(step_us=round(float(np.median(t)), 2), step_us_min_max=[round(min(t), 2), round(max(t), 2)], step_us_rounds=[round(x, 2) for x in t])


def decoder_step(S, args):
    """One training step (forward + backward) of the decoder at [2, 64, 256, 256], spectral=False and spectral=True."""
    torch.manual_seed(7)
    x = torch.randn(2, 64, 256, 256, device="cuda")
    x = x * (torch.rand(2, 1, 256, 256, device="cuda") > 0.3)
    g = torch.randn(2, 3, 256, 256, device="cuda")
    nets = {k: S.TrainableDecoderPconv2(spectral=sn).cuda().train() for k, sn in (("spectral_false", False), ("spectral_true", True))}

    def step(net):
        for p in net.parameters():
            p.grad = None
        net(x).backward(g)
    times = alternate(args, args.decoder_steps, {k: (lambda n=n: step(n)) for k, n in nets.items()})
    res = {k: summary(t) for k, t in times.items()}
    res["true_over_false"] = round(res["spectral_true"]["step_us"] / res["spectral_false"]["step_us"], 4)
    res["added_us_per_step"] = round(res["spectral_true"]["step_us"] - res["spectral_false"]["step_us"], 1)
    res["difference_exceeds_the_spread"] = bool(min(times["spectral_true"]) > max(times["spectral_false"]) or
                                                min(times["spectral_false"]) > max(times["spectral_true"]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--decoder-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--no-decoder", action="store_true", help="skip the decoder training step")
    ap.add_argument("--trace-steps", type=int, default=3)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=VARIANTS + ("largest",), help="(child of a trace) run this variant's steps and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/spectral_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/spectral_bench.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "A": "per layer: adversarial.spectral_weight's formula, weight * scale, torch autograd, the existing preparation entries",
           "B": "SpectralGroup.run() (slr_spectral_sigma + slr_conv_prep_scaled_multi) and slr_spectral_weight_grad per tensor",
           "rounds": args.rounds, "steps_per_round": args.steps,
           "step_us": "device events around a block of steps, per step: what a training loop waits for, host launch cost included"}
    nets, group, grads = leaves_of(S)
    _, group_a, grads_a = leaves_of(S)                   # A moves u and v of tensors of its own
    doc["list"] = list_shape(group)
    print(f"{doc['list']['tensors']} normalised tensors ({doc['list']['convolutions']} convolutions, {doc['list']['linears']} linears)", file=sys.stderr)
    times = alternate(args, args.steps, {"A": lambda: step_A(S, group_a.leaves, grads_a), "B": lambda: step_B(S, group, grads)})
    for v in VARIANTS:
        doc[v + "_step"] = summary(times[v])
    doc["B_over_A"] = round(doc["B_step"]["step_us"] / doc["A_step"]["step_us"], 4)
    doc["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
    doc["A_faster_than_B_by_more_than_the_spread"] = bool(min(times["B"]) > max(times["A"]))
    if not args.no_trace:
        for v in VARIANTS:
            doc[v + "_step"]["trace"] = trace(args, v)
        big = trace(args, "largest")
        sig = [r for r in big["top"] if "slr::spectral_" in r["kernel"]]         # the band kernels and the finishing kernel
        us = round(sum(r["us_per_step"] for r in sig), 2)
        by = 2 * 4 * LARGEST[0] * LARGEST[1]
        doc["sigma_largest_alone"] = dict(shape=list(LARGEST), bytes_read=by, note="W is read twice (W^T u, then W v); banded over workgroups",
                                          kernels={r["kernel"].split("(")[0]: r["us_per_step"] for r in sig},
                                          kernel_us=us if sig else None, GBs=round(by / us / 1e3, 1) if sig else None)
    if not args.no_decoder:
        del nets, group, grads, group_a, grads_a
        doc["decoder_step_2x64x256x256"] = decoder_step(S, args)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
