#!/usr/bin/env python
"""Animate one still image on MI355X -- counterpart of the reference's
    python test_animating/test_baseline_4eval_rawsize.py IMG FLOW OUTDIR CKPT NAME W N SPEED ALIGN
(test_animating/CLAW/test_all_CLAW_scenes.py:86-96) with the same positional arguments; writes
OUTDIR/NAME/PredImg/%06d.png (--v1: also FluidImg/, CompositeFluidAlpha/, BGImg.png).  Without a checkpoint (CKPT = None)
the networks are random-initialised (plumbing / timing only).  --v1 runs the 2-layer SLR model (test_v1_4eval_rawsize.py).
Under torchrun the frames of the clip are rendered by all ranks (slr_sfs_amd/runner.py).
--motion-ckpt MOTION.pth (or a CKPT trained with --train_motion plus --predict-motion): the motion is predicted from the image by the
motion U-Net (test_animating/test_motion_4eval_rawsize_threshold.py), FLOW only supplies its moving-region mask and hints."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slr_sfs_amd import runner  # noqa: E402


def init_ranks():
    """(rank, world, device): one process per GPU under torchrun (RCCL), a single process otherwise."""
    import torch.distributed as dist
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("WORLD_SIZE", 1), ("LOCAL_RANK", 0)))
    one_gpu = os.environ.get("SLR_ONE_GPU_GLOO") == "1"        # development: all ranks on cuda:0, collectives over gloo
    dev = torch.device("cuda", 0 if one_gpu else local)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    return rank, world, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("image"), ap.add_argument("flow"), ap.add_argument("outdir"), ap.add_argument("ckpt")
    ap.add_argument("name"), ap.add_argument("W", type=int), ap.add_argument("N", type=int)
    ap.add_argument("speed", type=float), ap.add_argument("align", nargs="?", default="None")
    ap.add_argument("--H", type=int, default=None, help="working height (default: W, square like the reference)")
    ap.add_argument("--v1", action="store_true")
    ap.add_argument("--half-size", action="store_true", help="write frames at half the raw size (test_baseline_4eval.py / test_v1_4eval.py)")
    ap.add_argument("--motion-ckpt", default=None,
                    help="motion checkpoint (train_motion_unet.py): predict the motion from the image; FLOW then only gives the moving-region "
                         "mask and the motion hints.  With a mask + hint network the clip is animated at speed 1 whatever SPEED says "
                         "(the reference's motion test script forces it)")
    ap.add_argument("--predict-motion", action="store_true",
                    help="predict the motion with the motion regressor of CKPT (trained with --train_motion); implied by --motion-ckpt")
    ap.add_argument("--hint-points", default=None,
                    help="the 5 hint pixels 'y,x;y,x;...' at the flow's resolution (default: a deterministic k-means of the moving region, "
                         "whose positions are not those of the reference's sklearn KMeans)")
    ap.add_argument("--write-motion", action="store_true", help="also write the motion field used as OUTDIR/NAME/Motion.flo")
    ap.add_argument("--gt-frames", default=None,
                    help="ground truth of the clip (a directory of %%06d.png / .jpg frames or a uint8 [n,h,w,3] .npy): score the frames on "
                         "the device (PSNR, SSIM; tools/evaluate.py's metric.json for this one scene), from the uint8 frames written")
    ap.add_argument("--metrics-json", default=None, help="where --gt-frames writes its JSON (default OUTDIR/../metric.json)")
    ap.add_argument("--perceptual-weights", default=None, help="with --gt-frames: a torchvision VGG16 state dict, adds Perceptual")
    ap.add_argument("--lpips-alexnet", default=None, help="with --gt-frames and --lpips-linear: a torchvision AlexNet state dict, adds LPIPS")
    ap.add_argument("--lpips-linear", default=None, help="the lpips package's weights/v0.1/alex.pth (lin0 .. lin4)")
    a = ap.parse_args()
    if bool(a.lpips_alexnet) != bool(a.lpips_linear):
        ap.error("--lpips-alexnet and --lpips-linear go together: the trunk and the linear heads of LPIPS are two files")
    rank, world, dev = init_ranks()
    model = runner.load_model(a.ckpt, a.v1, dev, motion_ckpt=a.motion_ckpt)
    points = None if a.hint_points is None else [tuple(int(v) for v in p.split(",")) for p in a.hint_points.split(";")]
    score = None
    if a.gt_frames and rank == 0:
        def score(frames):
            import json
            from slr_sfs_amd import evaluation, metrics
            src = ("npy", a.gt_frames) if a.gt_frames.endswith(".npy") else ("frames", a.gt_frames)
            gt = evaluation.load_gt(src, frames.shape[0])
            if gt is None or gt.shape[0] < frames.shape[0]:
                raise ValueError(f"--gt-frames {a.gt_frames}: fewer than {frames.shape[0]} frames")
            gt = torch.from_numpy(evaluation.resize_like_reference(gt, tuple(frames.shape[1:3]))).to(frames.device)
            vgg = metrics.PerceptualVGG16.from_file(a.perceptual_weights, frames.device) if a.perceptual_weights else None
            lp = metrics.LPIPSAlex.from_files(a.lpips_alexnet, a.lpips_linear, frames.device) if a.lpips_alexnet else None
            per = {k: v.cpu().tolist() for k, v in metrics.evaluate_clip(frames.contiguous(), gt, perceptual=vgg, lpips=lp).items()}
            res = evaluation.aggregate({a.name: per}, evaluation.metric_keys(vgg is not None, lp is not None))
            path = a.metrics_json or os.path.join(a.outdir, "..", "metric.json")
            with open(path, "w") as f:
                json.dump(res, f)
            print(f"metrics of {a.name}: PSNR {res['TotalPSNR']:.4f} SSIM {res['TotalSSIM']:.5f} -> {path}")
    dt, out = runner.animate_scene(model, a.image, a.flow, a.outdir, a.name, a.H or a.W, a.W, a.N, a.speed, a.align, rank, world,
                                   half_size=a.half_size, predict_motion=bool(a.motion_ckpt or a.predict_motion), hint_points=points,
                                   write_motion=a.write_motion, score=score)
    if rank == 0:
        print(f"{a.N} frames at {a.H or a.W}x{a.W} on {world} GPU(s) in {dt:.2f} s ({a.N / dt:.1f} frames/s) -> {out}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
