#!/usr/bin/env python
"""One training step of the SPADE motion U-Net with its loss (forward + backward to every parameter) at the per-GPU shape of the
reference's train_motion_EPE_MotionGAN.sh, input [4,6,256,256], num_filters = 32, --motion_losses 10.0_EndPointError, two ways in one
process with the same seeded state and batch:

  A  the same network from torch.nn modules: torch.nn.utils.spectral_norm(nn.Conv2d) (F.conv2d on MIOpen), F.instance_norm, F.interpolate,
     torch.norm / mean and torch autograd;
  B  slr_sfs_amd.TrainableSPADEUnet4MaskMotion + MotionLoss (csrc/motion_grad.hip, csrc/conv4x4.hip, csrc/disc.hip, the fp32 3x3 rung).

Warm-up, then A and B alternated (ROUNDS rounds of STEPS steps, device events around every block of steps): the median with min - max,
the peak memory of a step of each, and -- unless --no-trace -- one child process per variant under `rocprofv3 --kernel-trace` for the sum
of kernel time and the launches of a step, the time of every new kernel against its bytes at 8 TB/s (the 4x4 kernels: their flops at the
fp32 matrix peak, 157.3 TFLOP/s), and the share of the torch elementwise operators B leaves to torch (the ReLU of mlp_shared, the sum of
the two gradients reaching each e_i, pred * div_flow).  No threshold: the numbers are recorded.  Prints one JSON document (--out FILE
writes it too).  A device is required.

    python tools/motion_train_bench.py --out profiles/motion_train_step.json
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
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, HW, NF = 4, 256, 32
PEAK_F32, PEAK_BW = 157.3e12, 8.0e12
ENC_NORM = {2: "2_0", 3: "4_0", 4: "8_0", 5: "8_1", 6: "8_2", 7: "8_3"}
DEC_NORM = {1: "8_4", 2: "8_5", 3: "8_6", 4: "8_7", 5: "4_1", 6: "2_1", 7: ""}


def widths(nf):
    enc = [6, nf, nf * 2, nf * 4, nf * 8, nf * 8, nf * 8, nf * 8, nf * 8]
    dec = [(nf * 8, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 4), (nf * 8, nf * 2), (nf * 4, nf), (nf * 2, 2)]
    return enc, dec


def work_per_step(n=N, hw=HW, nf=NF):
    """Flops (2 per multiply-add) of the 4x4 kernels and the bytes the other new kernels have to move in one step."""
    enc, dec = widths(nf)
    w = {k: dict(flop=0.0, bytes=0.0) for k in ("conv4x4s2_backward_data", "conv4x4s2_weight_grad", "instnorm_spade_forward",
                                                "instnorm_spade_backward", "upsample2x_concat_backward", "motion_loss", "motion_loss_grad")}
    h = hw
    for i in range(1, 9):
        mac = 2.0 * n * enc[i] * (h // 2) ** 2 * enc[i - 1] * 16
        if i > 1:
            w["conv4x4s2_backward_data"]["flop"] += mac
        w["conv4x4s2_weight_grad"]["flop"] += mac
        h //= 2
    planes = [(enc[i], hw >> i) for i in ENC_NORM] + [(dec[k - 1][1], hw >> (8 - k)) for k in DEC_NORM]
    for c, s in planes:
        el = 4.0 * n * c * s * s
        w["instnorm_spade_forward"]["bytes"] += 4 * el              # x, gamma, beta in, out
        w["instnorm_spade_backward"]["bytes"] += 7 * el             # x, gamma, g in; gx, d gamma, d beta out (+ the second pass over g)
    for k in range(0, 8):                                           # the eight up-samplings: sources at hw >> (8 - k)
        s = hw >> (8 - k)
        c = enc[8] if k == 0 else dec[k - 1][1] + enc[8 - k]
        w["upsample2x_concat_backward"]["bytes"] += 4.0 * n * c * s * s * (4 + 4 + 1)      # g and the gate (4x each), the result
    w["motion_loss"]["bytes"] = 4.0 * n * 2 * hw * hw * 2
    w["motion_loss_grad"]["bytes"] = 4.0 * n * 2 * hw * hw * 3
    return w


FAMILIES = (("conv4x4s2_forward", r"conv4x4_kernel<\(?(?:slr::)?\(?(?:int\))?4[,>]"), ("conv4x4s2_backward_data", r"conv4x4_kernel<\(?(?:slr::)?\(?(?:int\))?5[,>]"),
            ("conv4x4s2_weight_grad", r"conv4x4_wgrad_kernel"), ("conv4x4s2_weight_grad_sum", r"conv4x4_wgrad_sum_kernel"),
            ("conv4x4_weights", r"conv4x4_weights_kernel"), ("conv4x4_bias_grad", r"conv4x4_bias_grad_kernel"),
            ("instnorm_spade_forward", r"instnorm_spade_kernel"), ("instnorm_spade_backward", r"instnorm_spade_bwd_kernel"),
            ("upsample2x_concat_forward", r"upsample2x_concat_kernel"), ("upsample2x_concat_backward", r"upsample2x_concat_bwd_kernel"),
            ("motion_loss", r"motion_loss_kernel|motion_loss_sum_kernel"), ("motion_loss_grad", r"motion_loss_grad_kernel"),
            ("conv3x3_fp32_rung", r"conv3x3|conv_f32|wgrad_kernel"), ("spectral", r"spectral_"),
            ("torch_elementwise", r"at::native"))


class TorchSPADE(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.mlp_shared = nn.Sequential(nn.Conv2d(6, 128, 3, padding=1), nn.ReLU())
        self.mlp_gamma, self.mlp_beta = nn.Conv2d(128, C, 3, padding=1), nn.Conv2d(128, C, 3, padding=1)

    def forward(self, x, seg):
        size = x.shape[2:]
        seg = torch.cat([F.interpolate(seg[:, :3], size=size, mode="bilinear", align_corners=False),
                         F.interpolate(seg[:, 3:4], size=size, mode="nearest"),
                         F.interpolate(seg[:, 4:6], size=size, mode="bilinear", align_corners=False)], 1)
        actv = self.mlp_shared(seg)
        return F.instance_norm(x) * (1 + self.mlp_gamma(actv)) + self.mlp_beta(actv)


class TorchNet(nn.Module):
    """Variant A, with the reference's state-dict names."""

    def __init__(self, nf):
        super().__init__()
        enc, dec = widths(nf)
        sn = nn.utils.spectral_norm
        for i in range(1, 9):
            setattr(self, f"conv{i}", sn(nn.Conv2d(enc[i - 1], enc[i], 4, 2, 1)))
            setattr(self, f"dconv{i}", sn(nn.Conv2d(dec[i - 1][0], dec[i - 1][1], 3, 1, 1)))
        for i, s in ENC_NORM.items():
            setattr(self, f"spade_layer{s}", TorchSPADE(enc[i]))
        for k, s in DEC_NORM.items():
            setattr(self, f"spade_layer{s}", TorchSPADE(dec[k - 1][1]))

    @staticmethod
    def up(x):
        b = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)      # noqa: E731
        return torch.cat([b(x[:, :3]), F.interpolate(x[:, 3:4], scale_factor=2, mode="nearest"), b(x[:, 4:])], 1)

    def forward(self, x):
        e = [self.conv1(x)]
        for i in range(2, 9):
            y = getattr(self, f"conv{i}")(F.leaky_relu(e[-1], 0.2))
            e.append(getattr(self, f"spade_layer{ENC_NORM[i]}")(y, x) if i < 8 else y)
        d = self.up(F.relu(e[7]))
        for k in range(1, 8):
            d_ = getattr(self, f"spade_layer{DEC_NORM[k]}")(getattr(self, f"dconv{k}")(d), x)
            d = F.relu(torch.cat([self.up(d_), self.up(e[7 - k])], 1))
        return self.dconv8(d)


def make_state(nf):
    """Seeded weights (randn * sqrt(2 / fan-in); small SPADE maps), biases, unit u / v, and the input + target."""
    import slr_sfs_amd as S
    g = torch.Generator().manual_seed(4321)
    sd = {}
    for k, v in S.TrainableSPADEUnet4MaskMotion(nf=nf).reference_state_dict().items():
        t = torch.randn(v.shape, generator=g)
        if k.endswith(("_u", "_v")):
            sd[k] = t / t.norm()
        elif k.endswith("bias"):
            sd[k] = 0.1 * t
        else:
            sd[k] = t * (0.1 if "mlp_gamma" in k or "mlp_beta" in k else 1.0) * (2.0 / (v[0].numel())) ** 0.5
    x = torch.cat([torch.rand(N, 3, HW, HW, generator=g) * 2 - 1, (torch.rand(N, 1, HW, HW, generator=g) > 0.5).float(),
                   torch.randn(N, 2, HW, HW, generator=g)], 1)
    return sd, x, torch.randn(N, 2, HW, HW, generator=g)


def stepper(S, variant, sd, x, gt, nf):
    if variant == "A":
        net = TorchNet(nf)
        net.load_state_dict(sd)
    else:
        net = S.TrainableSPADEUnet4MaskMotion(nf=nf).load_reference_state_dict(sd)
        loss_fn = S.MotionLoss(types.SimpleNamespace(motion_losses=["10.0_EndPointError"]))
    net = net.cuda().train()
    x, gt = x.cuda(), gt.cuda()
    params = list(net.parameters())

    def run():
        for p in params:
            p.grad = None
        pred = net(x)
        if variant == "A":
            loss = torch.norm(pred * 1.0 - gt, 2, 1).mean() * 10.0
        else:
            loss = loss_fn(pred * 1.0, gt)["Total Loss"]
        loss.backward()
        return loss, pred
    return run, net


MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: brackets the traced steps


def run_only(S, args):
    sd, x, gt = make_state(args.nf)
    run, _ = stepper(S, args.only, sd, x, gt, args.nf)
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        run()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_step(args, variant):
    """Kernel time of one step of one variant, from a child process under rocprofv3 (kernel trace only)."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--steps", str(args.trace_steps), "--warmup", str(args.trace_warmup),
               "--nf", str(args.nf)]
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
    total = sum(sum(v) for v in per.values()) / n / 1e3
    res = dict(kernel_us_per_step=round(total, 2), launches_per_step=round(sum(len(v) for v in per.values()) / n, 2), top=top[:14])
    if variant == "B":
        work, fam, seen = work_per_step(nf=args.nf), {}, set()
        for name, pat in FAMILIES:
            keys = [k for k in per if re.search(pat, k) and k not in seen]
            seen.update(keys)
            us = sum(sum(per[k]) for k in keys) / n / 1e3
            e = dict(us_per_step=round(us, 2), launches_per_step=round(sum(len(per[k]) for k in keys) / n, 2), share_of_step=round(us / total, 4))
            if name in work and us > 0:
                fl, by = work[name]["flop"], work[name]["bytes"]
                if fl:
                    e.update(GFLOP=round(fl / 1e9, 2), TFLOPs=round(fl / us / 1e6, 2), share_of_fp32_matrix_peak=round(fl / us / 1e-6 / PEAK_F32, 4))
                else:
                    e.update(MB=round(by / 1e6, 1), TBs=round(by / us / 1e6, 3), share_of_8TBs=round(by / us / 1e-6 / PEAK_BW, 4))
            fam[name] = e
        res["kernel_families"] = fam
        res["unmatched_us_per_step"] = round(sum(sum(v) for k, v in per.items() if k not in seen) / n / 1e3, 2)
    return res


def measure(S, args):
    sd, x, gt = make_state(args.nf)
    runs = {v: stepper(S, v, sd, x, gt, args.nf)[0] for v in "AB"}
    res = {"shape": dict(input=[N, 6, HW, HW], nf=args.nf), "rounds": args.rounds, "steps_per_round": args.steps}
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())        # noqa: E731
    (la, pa), (lb, pb) = runs["A"](), runs["B"]()         # the first step from the same state: u / v move alike in A and B
    res["B_vs_A_first_step"] = dict(loss=rel(lb, la), prediction=rel(pb, pa))
    times, r = {v: [] for v in "AB"}, {}
    for v in "AB":
        for _ in range(args.warmup):
            runs[v]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        runs[v]()
        torch.cuda.synchronize()
        r[f"{v}_peak_step_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    for _ in range(args.rounds):
        for v in "AB":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                runs[v]()
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) / args.steps)
    for v in "AB":
        t = times[v]
        r[f"{v}_step_ms_rounds"] = [round(x, 3) for x in t]
        r[f"{v}_step_ms"] = round(float(np.median(t)), 3)
        r[f"{v}_step_ms_min_max"] = [round(min(t), 3), round(max(t), 3)]
    r["B_over_A"] = round(r["B_step_ms"] / r["A_step_ms"], 3)
    r["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
    r["A_faster_than_B_by_more_than_the_spread"] = bool(min(times["B"]) > max(times["A"]))
    res["training_step"] = r
    if not args.no_trace:
        for v in "AB":
            res[f"{v}_trace_training_step"] = kernel_time_per_step(args, v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nf", type=int, default=NF)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=2)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["A", "B"], help="(child of a trace) run this variant's steps and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/motion_train_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/motion_train_bench.py", "device": torch.cuda.get_device_name(0),
           "A": "spectral_norm(nn.Conv2d) (MIOpen), F.instance_norm, F.interpolate, torch.norm + torch autograd",
           "B": "slr_sfs_amd.TrainableSPADEUnet4MaskMotion + MotionLoss", "work_per_step": work_per_step(nf=args.nf)}
    doc.update(measure(S, args))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
