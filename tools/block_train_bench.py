#!/usr/bin/env python
"""One training step (forward + backward to the input and every parameter) of one decoder block, ResNet_Block_Pconv2 in train() mode, on the
training crop, two ways in one process with the same seeded weights and noise:

  A  the block from torch operators: the reference's batch-norm formulas (models/layers/normalization.py:319-354), PartialConv2d's ops
     (models/layers/partialconv2d.py:61-74, full-channel masks, the mask convolution under no_grad), F.conv2d (MIOpen),
     F.avg_pool2d / F.interpolate / F.max_pool2d, and torch autograd;
  B  slr_sfs_amd.TrainablePconvResBlock on channel-blocked activations where the channel counts allow.

Per shape: warm-up, then A and B alternated (ROUNDS rounds of STEPS steps, device events around every block of steps), the peak memory of
a step of each, and -- unless --no-trace -- one child process per variant under `rocprofv3 --kernel-trace` for the sum of kernel time,
the launches per step and the time of every kernel of csrc/block_grad.hip.  No threshold: the numbers are recorded.  Prints one JSON
document (--out FILE writes it too).  A device is required.

    python tools/block_train_bench.py --out profiles/block_train_step.json
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

# name: (N, Cin, Cout, H, W, resample)
SHAPES = {"block_2x64to128x256x256_down": (2, 64, 128, 256, 256, "Down"), "block_2x128to256x128x128_down": (2, 128, 256, 128, 128, "Down"),
          "block_2x256to256x64x64": (2, 256, 256, 64, 64, None), "block_2x256to128x64x64_up": (2, 256, 128, 64, 64, "Up"),
          "block_2x128to3x256x256": (2, 128, 3, 256, 256, None)}
NEW_KERNELS = ("bn_stats", "bn_tables", "bn_train_forward", "bn_backward", "conv1x1_wgrad", "avgpool3x3s2_backward", "upsample2x_backward")
EPS = 1e-5


def to_blocked(x):
    N, C, H, W = x.shape
    return x.reshape(N, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().view(N, C, H, W)


def make_case(shape):
    N, cin, cout, H, W, kind = shape
    g = torch.Generator(device="cpu").manual_seed(cin * 1000 + cout)
    r = lambda *s: torch.randn(*s, generator=g)                              # noqa: E731
    m = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
    m[:, :, H // 3:H // 3 + H // 6, W // 4:W // 4 + W // 5] = 0.0
    OH, OW = {None: (H, W), "Down": ((H - 1) // 2 + 1, (W - 1) // 2 + 1), "Up": (2 * H, 2 * W)}[kind]
    return dict(x=(r(N, cin, H, W) + 0.5) * m, mask=m, g=r(N, cout, OH, OW), noise=(r(N, 20), r(N, 20)),
                w_aa=r(cout, cin, 3, 3) / (3.0 * cin ** 0.5), b_aa=0.1 * r(cout), w_ab=r(cout, cout, 3, 3) / (3.0 * cout ** 0.5),
                b_ab=0.1 * r(cout), w_b=r(cout, cin, 1, 1) / cin ** 0.5 if (kind or cin != cout) else None,
                lin=[0.1 * r(cin, 20), 0.1 * r(cin, 20), 0.1 * r(cout, 20), 0.1 * r(cout, 20)])


def torch_block(shape, c):
    """Variant A: parameters (leaves on the device) and step()."""
    N, cin, cout, H, W, kind = shape
    x = c["x"].cuda().requires_grad_(True)
    prm = {k: c[k].cuda().requires_grad_(True) for k in ("w_aa", "b_aa", "w_ab", "b_ab", "w_b") if c[k] is not None}
    lin = [t.cuda().requires_grad_(True) for t in c["lin"]]
    n1, n2 = (t.cuda() for t in c["noise"])
    mfull, g = c["mask"].cuda().expand(N, cin, H, W).contiguous(), c["g"].cuda()
    ones = {ci: torch.ones(cout, ci, 3, 3, device="cuda") for ci in {cin, cout}}

    def bn(t, mask, noise, wg, wb):                     # partial_manual_bn + partial_fused_bn
        gain, bias = (1 + noise @ wg.t())[:, :, None, None], (noise @ wb.t())[:, :, None, None]
        cnt = torch.sum(mask, [0, 2, 3], keepdim=True) + EPS
        m, m2 = torch.sum(t, [0, 2, 3], keepdim=True) / cnt, torch.sum(t ** 2, [0, 2, 3], keepdim=True) / cnt
        scale = torch.rsqrt(m2 - m ** 2 + EPS) * gain
        return t * scale - (m * scale - bias)

    def pconv(t, mask, w, b):
        ci = t.shape[1]
        with torch.no_grad():
            um_raw = F.conv2d(mask, ones[ci], padding=1)
            ratio = (ci * 9) / (um_raw + 1e-8)
            um = torch.clamp(um_raw, 0, 1)
            ratio = ratio * um
        raw = F.conv2d(t * mask, w, b, padding=1)
        bv = b.view(1, -1, 1, 1)
        return ((raw - bv) * ratio + bv) * um, um

    def resample(t):
        if kind == "Down":
            return F.avg_pool2d(t, 3, stride=2, padding=1)
        return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False) if kind == "Up" else t

    def step():
        x.grad = None
        for t in list(prm.values()) + lin:
            t.grad = None
        a, m = pconv(F.relu(bn(x, mfull, n1, lin[0], lin[1])), mfull, prm["w_aa"], prm["b_aa"])
        a, m = pconv(F.relu(bn(a, m, n2, lin[2], lin[3])), m, prm["w_ab"], prm["b_ab"])
        y = resample(a) + resample(F.conv2d(x, prm["w_b"]) if "w_b" in prm else x)
        um = F.max_pool2d(m, 3, stride=2, padding=1) if kind == "Down" else F.interpolate(m, scale_factor=2, mode="nearest") if kind == "Up" else m
        y.backward(g)
        return y, um, x.grad
    return step


def hip_block(S, shape, c):
    """Variant B."""
    N, cin, cout, H, W, kind = shape
    blk = S.TrainablePconvResBlock(cin, cout, kind).cuda().train()
    with torch.no_grad():
        blk.conv_aa.weight.copy_(c["w_aa"]), blk.conv_aa.bias.copy_(c["b_aa"]), blk.conv_ab.weight.copy_(c["w_ab"]), blk.conv_ab.bias.copy_(c["b_ab"])
        if c["w_b"] is not None:
            blk.conv_b.weight.copy_(c["w_b"])
        for lin, w in zip((blk.bn1.gain, blk.bn1.bias, blk.bn2.gain, blk.bn2.bias), c["lin"]):
            lin.weight.copy_(w)
    ib8, ob8 = cin % 8 == 0, (cout % 8 == 0 if blk.conv_b is not None else cin % 8 == 0)
    x = (to_blocked(c["x"]) if ib8 else c["x"]).cuda().requires_grad_(True)
    g = (to_blocked(c["g"]) if ob8 else c["g"]).cuda()
    mask, noise = c["mask"].cuda(), tuple(t.cuda() for t in c["noise"])

    def step():
        x.grad = None
        for p in blk.parameters():
            p.grad = None
        y, um, _ = blk(x, mask, ib8, noise=noise)
        y.backward(g)
        return y, um, x.grad
    return step


def stepper(S, shape, c, variant):
    return torch_block(shape, c) if variant == "A" else hip_block(S, shape, c)


MARKER = "slr::normalize_kernel("        # a kernel of the library that neither variant launches: brackets the traced steps


def run_only(S, args):
    shape = SHAPES[args.shape]
    step = stepper(S, shape, make_case(shape), args.only)
    tiny = torch.ones(1, 2, 1, 1, device="cuda")
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    S.softsplat.splat_normalize(tiny)
    for _ in range(args.steps):
        step()
    S.softsplat.splat_normalize(tiny)
    torch.cuda.synchronize()


def kernel_time_per_step(args, shape_name, variant):
    """Kernel time per step of one variant from a child process under rocprofv3: the kernels between the two markers of run_only."""
    with tempfile.TemporaryDirectory(dir=args.trace_dir) as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--only", variant, "--shape", shape_name, "--steps", str(args.trace_steps),
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
    row = lambda k, v: dict(us_per_step=round(sum(v) / n / 1e3, 2), launches_per_step=round(len(v) / n, 2),           # noqa: E731
                            us_per_launch=round(sum(v) / len(v) / 1e3, 2), kernel=k[:140])
    top = sorted((row(k, v) for k, v in per.items()), key=lambda r: -r["us_per_step"])
    return dict(kernel_us_per_step=round(sum(sum(v) for v in per.values()) / n / 1e3, 2),
                launches_per_step=round(sum(len(v) for v in per.values()) / n, 2), top=top[:10],
                new_kernels=[r for r in top if any(k in r["kernel"] for k in NEW_KERNELS)],
                conv3x3_us_per_step=round(sum(r["us_per_step"] for r in top if "conv3x3" in r["kernel"] or "conv_few" in r["kernel"]
                                              or "conv_split" in r["kernel"] or "conv_grad_scale" in r["kernel"]), 2))


def measure(S, args, shape_name):
    shape = SHAPES[shape_name]
    N, cin, cout, H, W, kind = shape
    c = make_case(shape)
    steps = {v: stepper(S, shape, c, v) for v in "AB"}
    res = {"shape": dict(N=N, Cin=cin, Cout=cout, H=H, W=W, resample=kind), "rounds": args.rounds, "steps_per_round": args.steps}
    ya, yb = steps["A"](), steps["B"]()
    def un(t, b8):
        t = t.detach().cpu()
        return t.view(N, t.shape[1] // 8, t.shape[2], t.shape[3], 8).permute(0, 1, 4, 2, 3).reshape(t.shape) if b8 else t
    ib8 = cin % 8 == 0
    ob8 = cout % 8 == 0 if c["w_b"] is not None else ib8
    res["B_vs_A"] = dict(y=float((un(yb[0], ob8) - ya[0].detach().cpu()).abs().max() / ya[0].abs().max()),
                         dx=float((un(yb[2], ib8) - ya[2].cpu()).abs().max() / ya[2].abs().max()),
                         update_mask_equal=bool(torch.equal(yb[1][:, :1], ya[1][:, :1])))
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
        res[f"{v}_step_us_spread"] = round(float(max(t) - min(t)), 2)
    res["B_over_A"] = round(res["B_step_us"] / res["A_step_us"], 3)
    res["B_faster_than_A_by_more_than_the_spread"] = bool(min(times["A"]) > max(times["B"]))
    res["A_faster_than_B_by_more_than_the_spread"] = bool(min(times["B"]) > max(times["A"]))
    if not args.no_trace:
        for v in "AB":
            res[f"{v}_trace"] = kernel_time_per_step(args, shape_name, v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--trace-steps", type=int, default=5)
    ap.add_argument("--trace-warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None, help="where the traces' temporary directories go")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["A", "B"], help="(child of a trace) run this variant's steps and nothing else")
    ap.add_argument("--shape", choices=list(SHAPES), default="block_2x64to128x256x256_down")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/block_train_bench.py: no ROCm device -- a timing has no CPU path")
    import slr_sfs_amd as S
    S._lib.lib()
    if args.only:
        return run_only(S, args)
    doc = {"tool": "tools/block_train_bench.py", "device": torch.cuda.get_device_name(0),
           "A": "torch operators (reference BN formulas, PartialConv2d ops, F.conv2d / MIOpen, F.avg_pool2d / F.interpolate) + torch autograd",
           "B": "slr_sfs_amd.TrainablePconvResBlock (channel-blocked where C % 8 == 0)", "cases": {}}
    for name in args.shapes:
        doc["cases"][name] = measure(S, args, name)
        if args.out:                                     # (written after every shape: a run cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
