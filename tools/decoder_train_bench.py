#!/usr/bin/env python
"""One training step (forward + backward to the input and every parameter) of the generator's networks in train() mode on the training
crop, two ways in one process with the same seeded weights and noise:

  A  the net from torch operators: the reference's batch-norm formulas (models/layers/normalization.py:319-354), PartialConv2d's ops
     (models/layers/partialconv2d.py:61-74) with the [N,C,H,W] mask (x != 0) in the decoder's first block and full-channel masks after
     it (the mask convolution under no_grad), F.conv2d (MIOpen), F.avg_pool2d / F.interpolate / F.max_pool2d, and torch autograd;
  B  slr_sfs_amd.TrainableDecoderPconv2 / TrainableEncoderWithZ (channel-blocked activations where the channel counts allow).

Cases: the decoder at [2,64,256,256], EncoderWithZ at [2,3,256,256].  Per case: warm-up, then A and B alternated (ROUNDS rounds of STEPS
steps, device events around every block of steps; the median with the min - max of the rounds), the peak memory of a step of each, and
-- unless --no-trace -- one child process per variant under `rocprofv3 --kernel-trace` for the sum of kernel time, the launches per step
and the time of every kernel only the decoder's first block launches, those of the decoder against the bytes they must move at block 0's shape and
8 TB/s.  No threshold: the numbers are recorded.  Prints one JSON document (--out FILE writes it too).  A device is required.

    python tools/decoder_train_bench.py --out profiles/decoder_train_step.json
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"decoder_2x64x256x256": ("decoder", 2, 64, 256, 256), "encoder_with_z_2x3x256x256": ("encoder", 2, 3, 256, 256)}
EPS = 1e-5
HBM = 8e12
# bytes the tensor-sized kernels of the decoder's first block must move per element of it (64 -> 64, identity skip), in tensors of
# 4 N C H W bytes: x | x (+ plane) | x, a | x, ga | x, ga, addend, dx | raw, residual, out.  The batch-norm kernels are the nonzero-mask
# instantiations `<layout, true...` of csrc/block_grad.hip's family, the other two csrc/decoder_grad.hip's.
_NONZERO_BN = {"bn_stats_kernel": 1, "bn_train_forward_kernel": 2, "bn_backward_reduce_kernel": 2, "bn_backward_dx_kernel": 4}
TENSORS_MOVED = {f"{k}<{b8}, true": t for k, t in _NONZERO_BN.items() for b8 in ("false", "true")}
TENSORS_MOVED.update({"nz_count_plane": 1, "pconv_train_epilogue": 3})
# (the two finalize kernels are shared with the batch-norms of all other blocks: their rows sum over every block of the net)
NEW_KERNELS = tuple(TENSORS_MOVED) + ("bn_stats_final_kernel", "bn_backward_final_kernel")


def make_case(case):
    """Seeded input, output gradient, noise, and the parameters of the net as the B module holds them (CPU)."""
    import slr_sfs_amd as S
    kind, N, C, H, W = CASES[case]
    g = torch.Generator(device="cpu").manual_seed(C)
    r = lambda *s: torch.randn(*s, generator=g)                              # noqa: E731
    net = S.TrainableDecoderPconv2() if kind == "decoder" else S.TrainableEncoderWithZ()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 4:
                p.copy_(r(*p.shape) / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5)
            else:
                p.copy_(0.1 * r(*p.shape))
    x = r(N, C, H, W) + 0.5
    if kind == "decoder":                                # holes of whole pixels and single zero elements, as a splatted feature map has
        m = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
        m[:, :, H // 3:H // 3 + H // 6, W // 4:W // 4 + W // 5] = 0.0
        x = x * m * (torch.rand(N, C, H, W, generator=g) > 0.05).float()
    cout = 3 if kind == "decoder" else 65
    return dict(kind=kind, net=net, x=x, g=r(N, cout, H, W), noise=[(r(N, 20), r(N, 20)) for _ in net.blocks])


def torch_net(c):
    """Variant A: the parameters of B's module as leaves on the device, and step()."""
    kind = c["kind"]
    blocks = []
    for blk in c["net"].blocks:
        t = lambda p: None if p is None else p.detach().clone().cuda().requires_grad_(True)      # noqa: E731
        blocks.append(dict(w_aa=t(blk.conv_aa.weight), b_aa=t(blk.conv_aa.bias), w_ab=t(blk.conv_ab.weight), b_ab=t(blk.conv_ab.bias),
                           w_b=t(blk.conv_b.weight) if blk.conv_b is not None else None,
                           b_b=t(blk.conv_b.bias) if blk.conv_b is not None and blk.conv_b.bias is not None else None,
                           lin=[t(blk.bn1.gain.weight), t(blk.bn1.bias.weight), t(blk.bn2.gain.weight), t(blk.bn2.bias.weight)], kind=blk.kind))
    leaves = [p for b in blocks for p in [b["w_aa"], b["b_aa"], b["w_ab"], b["b_ab"], b["w_b"], b["b_b"]] + b["lin"] if p is not None]
    x, g = c["x"].cuda().requires_grad_(True), c["g"].cuda()
    noise = [tuple(t.cuda() for t in nz) for nz in c["noise"]]
    ones = {}

    def bn(t, mask, nz, wg, wb):                         # (partial_)manual_bn + partial_fused_bn
        gain, bias = (1 + nz @ wg.t())[:, :, None, None], (nz @ wb.t())[:, :, None, None]
        if mask is None:
            m, m2 = torch.mean(t, [0, 2, 3], keepdim=True), torch.mean(t ** 2, [0, 2, 3], keepdim=True)
        else:
            cnt = torch.sum(mask, [0, 2, 3], keepdim=True) + EPS
            m, m2 = torch.sum(t, [0, 2, 3], keepdim=True) / cnt, torch.sum(t ** 2, [0, 2, 3], keepdim=True) / cnt
        scale = torch.rsqrt(m2 - m ** 2 + EPS) * gain
        return t * scale - (m * scale - bias)

    def pconv(t, mask, w, b):
        co, ci = w.shape[:2]
        if (co, ci) not in ones:
            ones[(co, ci)] = torch.ones(co, ci, 3, 3, device="cuda")
        with torch.no_grad():
            um_raw = F.conv2d(mask, ones[(co, ci)], padding=1)
            ratio = (ci * 9) / (um_raw + 1e-8)
            um = torch.clamp(um_raw, 0, 1)
            ratio = ratio * um
        raw = F.conv2d(t * mask, w, b, padding=1)
        bv = b.view(1, -1, 1, 1)
        return ((raw - bv) * ratio + bv) * um, um

    def resample(t, k):
        if k == "Down":
            return F.avg_pool2d(t, 3, stride=2, padding=1)
        return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False) if k == "Up" else t

    def step():
        x.grad = None
        for p in leaves:
            p.grad = None
        y = x
        mask = (x != 0).float() if kind == "decoder" else None
        for b, (n1, n2) in zip(blocks, noise):
            if kind == "decoder":
                a, m = pconv(F.relu(bn(y, mask, n1, b["lin"][0], b["lin"][1])), mask, b["w_aa"], b["b_aa"])
                a, m = pconv(F.relu(bn(a, m, n2, b["lin"][2], b["lin"][3])), m, b["w_ab"], b["b_ab"])
                k = b["kind"]
                mask = F.max_pool2d(m, 3, stride=2, padding=1) if k == "Down" else F.interpolate(m, scale_factor=2, mode="nearest") if k == "Up" else m
            else:
                a = F.conv2d(F.relu(bn(y, None, n1, b["lin"][0], b["lin"][1])), b["w_aa"], b["b_aa"], padding=1)
                a = F.conv2d(F.relu(bn(a, None, n2, b["lin"][2], b["lin"][3])), b["w_ab"], b["b_ab"], padding=1)
            skip = F.conv2d(y, b["w_b"], b["b_b"]) if b["w_b"] is not None else y
            y = resample(a, b["kind"]) + resample(skip, b["kind"])
        y.backward(g)
        return y, x.grad
    return step


def hip_net(c):
    """Variant B."""
    net = c["net"].cuda().train()
    x, g = c["x"].cuda().requires_grad_(True), c["g"].cuda()
    noise = [tuple(t.cuda() for t in nz) for nz in c["noise"]]

    def step():
        x.grad = None
        for p in net.parameters():
            p.grad = None
        y = net(x, noise=noise)
        y = torch.cat(y, 1) if isinstance(y, tuple) else y
        y.backward(g)
        return y, x.grad
    return step


MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: brackets the traced steps


def run_only(S, args):
    c = make_case(args.case)
    step = torch_net(c) if args.only == "A" else hip_net(c)
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        step()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_step(args, case, variant):
    """Kernel time per step of one variant from a child process under rocprofv3: the kernels between the two markers of run_only."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--case", case, "--steps", str(args.trace_steps),
               "--warmup", str(args.trace_warmup)]
        p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise SystemExit(f"trace of {case} {variant} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
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
    new = [r for r in top if any(k in r["kernel"] for k in NEW_KERNELS)]
    if CASES[case][0] == "decoder":                      # block 0 is the only caller of these kernels: one launch each per step
        _, N, C, H, W = CASES[case]
        for r in new:
            for k, tensors in TENSORS_MOVED.items():
                if k in r["kernel"]:
                    r["bytes"] = tensors * 4 * N * C * H * W
                    r["fraction_of_8TBps"] = round(r["bytes"] / HBM / (r["us_per_launch"] * 1e-6), 3)
    return dict(kernel_us_per_step=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
                launches_per_step=round(sum(len(v) for v in per.values()) / n, 2), top=top[:12], new_kernels=new,
                conv3x3_us_per_step=round(sum(r["us_per_step"] for r in top if "conv3x3" in r["kernel"] or "conv_few" in r["kernel"]
                                              or "conv_split" in r["kernel"] or "conv_grad_scale" in r["kernel"]), 2))


def measure(S, args, case):
    kind, N, C, H, W = CASES[case]
    c = make_case(case)
    steps = {"A": torch_net(c), "B": hip_net(c)}
    res = {"input": dict(N=N, C=C, H=H, W=W), "rounds": args.rounds, "steps_per_round": args.steps}
    ya, yb = [t.detach() for t in steps["A"]()], [t.detach() for t in steps["B"]()]
    res["B_vs_A"] = dict(y=float((yb[0] - ya[0]).abs().max() / ya[0].abs().max()), dx=float((yb[1] - ya[1]).abs().max() / ya[1].abs().max()),
                         note="the inputs are not kept away from the ReLU gates: dx differs by gate decisions, not by arithmetic")
    del ya, yb
    times = {v: [] for v in "AB"}
    for v in "AB":
        for _ in range(args.warmup):
            steps[v]()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        steps[v]()
        torch.cuda.synchronize()
        res[f"{v}_peak_step_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    for _ in range(args.rounds):
        for v in "AB":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                steps[v]()
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for v in "AB":
        t = times[v]
        res[f"{v}_step_us_rounds"] = [round(x, 2) for x in t]
        res[f"{v}_step_us"] = round(float(np.median(t)), 2)
        res[f"{v}_step_us_min_max"] = [round(float(min(t)), 2), round(float(max(t)), 2)]
    res["B_over_A"] = round(res["B_step_us"] / res["A_step_us"], 3)
    res["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
    res["A_faster_than_B_by_more_than_the_spread"] = bool(min(times["B"]) > max(times["A"]))
    if not args.no_trace:
        for v in "AB":
            res[f"{v}_trace"] = kernel_time_per_step(args, case, v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=3)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["A", "B"], help="(child of a trace) run this variant's steps and nothing else")
    ap.add_argument("--case", choices=list(CASES), default="decoder_2x64x256x256")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/decoder_train_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/decoder_train_bench.py", "device": torch.cuda.get_device_name(0),
           "A": "torch operators (reference BN formulas, PartialConv2d ops with the [N,C,H,W] mask, F.conv2d / MIOpen, F.avg_pool2d / F.interpolate) + torch autograd",
           "B": "slr_sfs_amd.TrainableDecoderPconv2 / TrainableEncoderWithZ (channel-blocked where C % 8 == 0)", "cases": {}}
    for name in args.cases:
        doc["cases"][name] = measure(S, args, name)
        if args.out:                                     # (written after every case: a run cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
