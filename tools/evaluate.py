#!/usr/bin/env python
"""Score animated clips against ground truth on the GPU -- counterpart of the reference's evaluation/animation/eval_CLAW.py and
eval_eulerian_data.py (with --fluid: eval_CLAW_fluid.py / eval_eulerian_data_fluid.py):

    python tools/evaluate.py PRED_DIR GT_DIR [--frames 60] [--fluid] [--perceptual-weights VGG16.pth]
                             [--lpips-alexnet ALEXNET.pth --lpips-linear ALEX_LIN.pth] [--out PATH]

PRED_DIR/NAME/PredImg/%06d.png is what tools/animate.py writes.  Ground truth of scene NAME: a frame directory GT_DIR/NAME/%06d.{png,jpg},
GT_DIR/NAME.npy (uint8 [n,h,w,3]), or GT_DIR/NAME.mp4 / NAME_gt.mp4, decoded only when an ffmpeg binary is on PATH (that path is not
exercised by the tests).  Ground truth is resized to the prediction's size as eval_CLAW.py:100-103 does (ToPILImage, PIL bilinear).
The first --frames frames of every scene are scored; scenes without as many predicted and ground-truth frames are listed and skipped
(eval_CLAW.py:66-77).  Writes metric.json (metric_fluid.json with --fluid) next to PRED_DIR, as the reference does, in its layout:
Total<metric>, Total<metric>_std, per-scene means <metric> and np.std <metric>_std.  Metrics: PSNR, SSIM, and Perceptual (VGG16, with
--perceptual-weights: a torchvision vgg16 state dict), and LPIPS (lpips.LPIPS(net='alex', version='0.1') as eval_CLAW.py:24,37 calls it:
on the [0, 1] images as they are), with --lpips-alexnet (a torchvision alexnet state dict) and --lpips-linear (the lpips package's
weights/v0.1/alex.pth), both or neither.  Nothing is downloaded."""
import argparse
import json
import os
import shutil
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slr_sfs_amd import evaluation, metrics  # noqa: E402


def select_scenes(pred_dir, gt_dir, frames):
    """([(name, gt source)] to score, [(name, reason)] skipped), names sorted."""
    scenes, skipped = [], []
    for name in sorted(os.listdir(pred_dir)):
        if not os.path.isdir(os.path.join(pred_dir, name)):
            continue
        n = evaluation.count_frames(os.path.join(pred_dir, name, "PredImg"))
        src = evaluation.gt_source(gt_dir, name)
        if n < frames:
            skipped.append((name, f"{n} predicted frames, {frames} needed"))
        elif src is None:
            skipped.append((name, "no ground truth"))
        elif src[0] == "frames" and evaluation.count_frames(src[1]) < frames:
            skipped.append((name, f"{evaluation.count_frames(src[1])} ground-truth frames, {frames} needed"))
        elif src[0] == "video" and shutil.which("ffmpeg") is None:
            skipped.append((name, f"{os.path.basename(src[1])} needs ffmpeg on PATH to be decoded"))
        else:
            scenes.append((name, src))
    return scenes, skipped


def check_lpips_args(ap, a):
    """--lpips-alexnet and --lpips-linear: both or neither (an argument error otherwise).  True when LPIPS is asked for."""
    if bool(a.lpips_alexnet) != bool(a.lpips_linear):
        ap.error("--lpips-alexnet and --lpips-linear go together: the trunk and the linear heads of LPIPS are two files")
    return bool(a.lpips_alexnet)


def score_scene(pred_dir, gt_dir, name, src, frames, vgg, fluid, dev, lpips=None):
    """Per-frame metrics of one scene: {metric: [floats]}."""
    pred = evaluation.read_frames(os.path.join(pred_dir, name, "PredImg"), frames)
    gt = evaluation.load_gt(src, frames)
    if gt is None or gt.shape[0] < frames:
        raise ValueError(f"{name}: {0 if gt is None else gt.shape[0]} ground-truth frames, {frames} needed")
    hw = pred.shape[1:3]
    gt = torch.from_numpy(evaluation.resize_like_reference(gt, hw)).to(dev)
    pred = torch.from_numpy(pred).to(dev)
    if fluid:
        flo = os.path.join(gt_dir, name + ".flo")
        flow_path = flo if os.path.exists(flo) else os.path.join(gt_dir, name + "_motion.pth")
        mask = evaluation.fluid_mask(evaluation.fluid_flow_tensor(flow_path), hw).to(dev)
        image = evaluation.load_input_image(os.path.join(gt_dir, name + "_input.jpg"), hw).to(dev)
        pred = evaluation.fluid_composite(pred, image, mask)
        gt = (gt.permute(0, 3, 1, 2).float() / 255.0).contiguous()
    res = metrics.evaluate_clip(pred, gt, perceptual=vgg, lpips=lpips)
    return {k: v.cpu().tolist() for k, v in res.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pred_dir"), ap.add_argument("gt_dir")
    ap.add_argument("--frames", type=int, default=60, help="frames scored per scene (default 60)")
    ap.add_argument("--fluid", action="store_true",
                    help="score the fluid region only (eval_CLAW_fluid.py): mask from GT_DIR/NAME.flo (or NAME_motion.pth), prediction "
                         "composited over GT_DIR/NAME_input.jpg; writes metric_fluid.json")
    ap.add_argument("--perceptual-weights", default=None, help="torchvision VGG16 state dict (vgg16-*.pth): adds the Perceptual metric")
    ap.add_argument("--lpips-alexnet", default=None, help="torchvision AlexNet state dict (alexnet-*.pth): with --lpips-linear, adds LPIPS")
    ap.add_argument("--lpips-linear", default=None, help="the lpips package's weights/v0.1/alex.pth (lin0 .. lin4)")
    ap.add_argument("--out", default=None, help="output JSON (default: PRED_DIR/../metric.json, ../metric_fluid.json with --fluid)")
    a = ap.parse_args(argv)
    want_lpips = check_lpips_args(ap, a)                 # (before anything touches the device)
    dev = torch.device("cuda", torch.cuda.current_device())
    lpips = metrics.LPIPSAlex.from_files(a.lpips_alexnet, a.lpips_linear, dev) if want_lpips else None
    vgg = metrics.PerceptualVGG16.from_file(a.perceptual_weights, dev) if a.perceptual_weights else None
    scenes, skipped = select_scenes(a.pred_dir, a.gt_dir, a.frames)
    for name, why in skipped:
        print(f"do not eval {name}: {why}")
    print(len(scenes), "scenes")
    per = {}
    for name, src in scenes:
        per[name] = score_scene(a.pred_dir, a.gt_dir, name, src, a.frames, vgg, a.fluid, dev, lpips)
        print(name, {k: round(float(np.mean(v)), 5) for k, v in per[name].items()})
    keys = evaluation.metric_keys(vgg is not None, lpips is not None)
    res = evaluation.aggregate(per, keys) if per else {}
    out = a.out or os.path.join(a.pred_dir, "..", "metric_fluid.json" if a.fluid else "metric.json")
    with open(out, "w") as f:
        json.dump(res, f)
    print("wrote", out)
    return res


if __name__ == "__main__":
    main()
