#!/usr/bin/env python
"""The adversarial part of a training step on the training crop ([2,3,256,256] fake + real = 4 images, ndf = 64): the generator-side step
(run_generator_one_step + backward to the fake image and the discriminator's parameters) and the discriminator step
(run_discriminator_one_step + backward to the parameters), two ways in one process with the same seeded weights, u / v and images:

  A  the same losses from torch operators: F.conv2d (MIOpen) inside torch.nn.utils.spectral_norm(nn.Conv2d), nn.InstanceNorm2d,
     nn.LeakyReLU, F.avg_pool2d, F.l1_loss and torch autograd;
  B  slr_sfs_amd.DiscriminatorLoss (csrc/disc.hip).

Warm-up, then A and B alternated (ROUNDS rounds of STEPS steps, device events around every block of steps) for each of the two steps, the
peak memory of a step of each, and -- unless --no-trace -- one child process per variant under `rocprofv3 --kernel-trace` for the sum of
kernel time and the launches of one generator-side + one discriminator step, and the time of every kernel of csrc/disc.hip against its
flops at the fp32 matrix peak (157.3 TFLOP/s) or its bytes at 8 TB/s.  No threshold: the numbers are recorded.  Prints one JSON document
(--out FILE writes it too).  A device is required.

    python tools/disc_train_bench.py --out profiles/disc_train_step.json
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_HALF, HW, NDF = 2, 256, 64
PEAK_F32, PEAK_BW = 157.3e12, 8.0e12
STRIDES = (2, 2, 2, 1, 1)


def layer_table(n=2 * N_HALF, hw=HW, ndf=NDF):
    """Per convolution of the two discriminators: (name, N, Cin, Cout, H, W, stride, OH, OW)."""
    rows = []
    for d in range(2):
        h, cin, nf = hw, 3, ndf
        for j, s in enumerate(STRIDES):
            cout = 1 if j == 4 else nf
            rows.append((f"D{d}.model{j}", n, cin, cout, h, h, s, h // s + 1, h // s + 1))
            h, cin = h // s + 1, cout
            if j < 3:
                nf = min(nf * 2, 512)
        hw = (hw - 1) // 2 + 1
    return rows


def work_per_training_step():
    """Flops (2 per multiply-add) and the bytes each pass has to move, per kernel family, of one generator-side + one discriminator
    step (two forwards; backward-data everywhere in the first and from model1 up in the second; two weight gradients)."""
    w = {k: dict(flop=0.0, bytes=0.0) for k in ("forward", "backward_data", "weight_grad", "instnorm_forward", "instnorm_backward")}
    for name, n, cin, cout, h, _, s, oh, _ in layer_table():
        mac = 2.0 * n * cout * oh * oh * cin * 16
        xin, out, wt = 4.0 * n * cin * h * h, 4.0 * n * cout * oh * oh, 4.0 * cout * cin * 16
        w["forward"]["flop"] += 2 * mac
        w["forward"]["bytes"] += 2 * (xin + out + wt)
        bd = 2 if "model0" not in name else 1
        w["backward_data"]["flop"] += bd * mac
        w["backward_data"]["bytes"] += bd * (xin + out + wt)
        w["weight_grad"]["flop"] += 2 * mac
        w["weight_grad"]["bytes"] += 2 * (xin + out + wt)
        if name[-1] in "123":
            w["instnorm_forward"]["bytes"] += 2 * 2 * out               # read x (three passes from cache), write y
            w["instnorm_backward"]["bytes"] += 2 * 3 * out              # read x and gy, write gx
    return w


FAMILIES = (("forward", r"conv4x4_kernel<\(?(?:slr::)?\(?(?:int\))?[01][,>]"), ("backward_data", r"conv4x4_kernel<\(?(?:slr::)?\(?(?:int\))?[23][,>]"),
            ("weight_grad", r"conv4x4_wgrad_kernel"), ("weight_grad_sum", r"conv4x4_wgrad_sum_kernel"), ("weights", r"conv4x4_weights_kernel"),
            ("bias_grad", r"conv4x4_bias_grad_kernel"), ("instnorm_forward", r"instnorm_lrelu_fwd_kernel"),
            ("instnorm_backward", r"instnorm_lrelu_bwd_kernel"))


class TorchNLayer(nn.Module):
    def __init__(self, ndf):
        super().__init__()
        nf = ndf
        self.model0 = nn.Sequential(nn.Conv2d(3, nf, 4, 2, 2), nn.LeakyReLU(0.2, False))
        for n in (1, 2, 3):
            prev, nf = nf, min(nf * 2, 512)
            conv = nn.utils.spectral_norm(nn.Conv2d(prev, nf, 4, 1 if n == 3 else 2, 2, bias=False))
            self.add_module(f"model{n}", nn.Sequential(nn.Sequential(conv, nn.InstanceNorm2d(nf, affine=False)), nn.LeakyReLU(0.2, False)))
        self.model4 = nn.Sequential(nn.Conv2d(nf, 1, 4, 1, 2))

    def forward(self, x):
        out = []
        for m in self.children():
            x = m(x)
            out.append(x)
        return out


class TorchLoss(nn.Module):
    """Variant A, with the state-dict names of the package's DiscriminatorLoss."""

    def __init__(self, ndf, lambda_feat=10.0):
        super().__init__()
        self.netD = nn.Module()
        self.netD.netD = nn.Module()
        for d in range(2):
            self.netD.netD.add_module(f"discriminator_{d}", TorchNLayer(ndf))
        self.lambda_feat = lambda_feat

    def features(self, x):
        out = []
        for D in self.netD.netD.children():
            out.append(D(x))
            x = F.avg_pool2d(x, 3, stride=2, padding=[1, 1], count_include_pad=False)
        return out

    def run_generator_one_step(self, fake, real):
        n = fake.shape[0]
        feats = self.features(torch.cat([fake, real]))
        gan = sum(-f[4][:n].mean().reshape(1) for f in feats) / len(feats)
        feat = fake.new_zeros(1)
        for f in feats:
            for t in f[:4]:
                feat = feat + F.l1_loss(t[:n], t[n:].detach()) * self.lambda_feat / len(feats)
        return {"GAN": gan, "GAN_Feat": feat, "Total Loss": (gan + feat).mean()}

    def run_discriminator_one_step(self, fake, real):
        n = fake.shape[0]
        feats = self.features(torch.cat([fake.detach(), real]))
        d_fake = sum(-torch.clamp_max(-f[4][:n] - 1, 0).mean().reshape(1) for f in feats) / len(feats)
        d_real = sum(-torch.clamp_max(f[4][n:] - 1, 0).mean().reshape(1) for f in feats) / len(feats)
        return {"D_Fake": d_fake, "D_real": d_real, "Total Loss": (d_fake + d_real).mean()}


def make_state(ndf):
    """Seeded weights (randn / sqrt(fan-in): the default initialisation makes the maps vanish), biases, unit u / v and the two images."""
    import slr_sfs_amd as S
    g = torch.Generator().manual_seed(1234)
    sd = {}
    for k, v in S.DiscriminatorLoss(ndf=ndf).state_dict().items():
        t = torch.randn(v.shape, generator=g)
        sd[k] = t / t.norm() if k.endswith(("_u", "_v")) else 0.3 * t if k.endswith("bias") else t / float(v.shape[1] * 16) ** 0.5
    imgs = [0.7 * torch.randn(N_HALF, 3, HW, HW, generator=g) for _ in range(2)]
    return sd, imgs


def stepper(S, variant, sd, imgs, ndf):
    loss = (TorchLoss(ndf) if variant == "A" else S.DiscriminatorLoss(ndf=ndf))
    loss.load_state_dict(sd)
    loss = loss.cuda().train()
    fake, real = imgs[0].cuda().requires_grad_(True), imgs[1].cuda()
    params = list(loss.parameters())

    def run(mode):
        fake.grad = None
        for p in params:
            p.grad = None
        out = (loss.run_generator_one_step if mode == "g" else loss.run_discriminator_one_step)(fake, real)
        out["Total Loss"].backward()
        return out, fake.grad
    return run, loss


MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: brackets the traced steps


def run_only(S, args):
    sd, imgs = make_state(args.ndf)
    run, _ = stepper(S, args.only, sd, imgs, args.ndf)
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.warmup):
        run("g"), run("d")
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        run("g"), run("d")
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_step(args, variant):
    """Kernel time of one generator-side + one discriminator step of one variant, from a child process under rocprofv3."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--steps", str(args.trace_steps), "--warmup", str(args.trace_warmup),
               "--ndf", str(args.ndf)]
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
    row = lambda k, v: dict(us_per_step=round(sum(v) / n / 1e3, 2), launches_per_step=round(len(v) / n, 2),           # noqa: E731
                            us_per_launch=round(sum(v) / len(v) / 1e3, 2), kernel=k[:140])
    top = sorted((row(k, v) for k, v in per.items()), key=lambda r: -r["us_per_step"])
    res = dict(kernel_us_per_step=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
               launches_per_step=round(sum(len(v) for v in per.values()) / n, 2), top=top[:12])
    if variant == "B":
        work, fam = work_per_training_step(), {}
        for name, pat in FAMILIES:
            us = sum(sum(v) for k, v in per.items() if re.search(pat, k)) / n / 1e3
            launches = sum(len(v) for k, v in per.items() if re.search(pat, k)) / n
            e = dict(us_per_step=round(us, 2), launches_per_step=round(launches, 2))
            if name in work and us > 0:
                fl, by = work[name]["flop"], work[name]["bytes"]
                e.update(GFLOP=round(fl / 1e9, 2), MB=round(by / 1e6, 1))
                if fl:
                    e.update(TFLOPs=round(fl / us / 1e6, 2), share_of_fp32_matrix_peak=round(fl / us / 1e-6 / PEAK_F32, 4))
                else:
                    e.update(TBs=round(by / us / 1e6, 3), share_of_8TBs=round(by / us / 1e-6 / PEAK_BW, 4))
            fam[name] = e
        res["new_kernels"] = fam
        res["new_kernels_unmatched"] = [k[:100] for k in per if ("conv4x4" in k or "instnorm_lrelu" in k) and not any(re.search(p, k) for _, p in FAMILIES)]
    return res


def measure(S, args):
    sd, imgs = make_state(args.ndf)
    runs = {v: stepper(S, v, sd, imgs, args.ndf)[0] for v in "AB"}
    res = {"shape": dict(fake=[N_HALF, 3, HW, HW], real=[N_HALF, 3, HW, HW], ndf=args.ndf), "rounds": args.rounds, "steps_per_round": args.steps,
           "layers": [dict(zip(("name", "N", "Cin", "Cout", "H", "W", "stride", "OH", "OW"), r)) for r in layer_table(ndf=args.ndf)]}
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())        # noqa: E731
    first = {}
    for mode in "gd":                                    # the first step of each from the same state: u / v move alike in A and B
        (la, ga), (lb, gb) = runs["A"](mode), runs["B"](mode)
        first[mode] = {k: rel(lb[k], la[k]) for k in la}
        if mode == "g":
            first[mode]["grad_fake"] = rel(gb, ga)
    res["B_vs_A_first_step"] = first
    for mode, label in (("g", "generator_step"), ("d", "discriminator_step")):
        times = {v: [] for v in "AB"}
        r = {}
        for v in "AB":
            for _ in range(args.warmup):
                runs[v](mode)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            runs[v](mode)
            torch.cuda.synchronize()
            r[f"{v}_peak_step_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        for _ in range(args.rounds):
            for v in "AB":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    runs[v](mode)
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / args.steps)
        for v in "AB":
            t = times[v]
            r[f"{v}_step_us_rounds"] = [round(x, 2) for x in t]
            r[f"{v}_step_us"] = round(float(np.median(t)), 2)
            r[f"{v}_step_us_min_max"] = [round(min(t), 2), round(max(t), 2)]
        r["B_over_A"] = round(r["B_step_us"] / r["A_step_us"], 3)
        r["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
        r["A_faster_than_B_by_more_than_the_spread"] = bool(min(times["B"]) > max(times["A"]))
        res[label] = r
    if not args.no_trace:
        for v in "AB":
            res[f"{v}_trace_generator_plus_discriminator_step"] = kernel_time_per_step(args, v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ndf", type=int, default=NDF)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=3)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["A", "B"], help="(child of a trace) run this variant's steps and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/disc_train_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/disc_train_bench.py", "device": torch.cuda.get_device_name(0),
           "A": "F.conv2d (MIOpen) in torch.nn.utils.spectral_norm(nn.Conv2d), nn.InstanceNorm2d, nn.LeakyReLU, F.avg_pool2d, F.l1_loss + torch autograd",
           "B": "slr_sfs_amd.DiscriminatorLoss (csrc/disc.hip)", "work_per_training_step": work_per_training_step()}
    doc.update(measure(S, args))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
