"""Host side of the reference's runners, for one or several GPUs of a node.

test_animating/test_baseline_4eval_rawsize.py / test_v1_4eval_rawsize.py animate ONE scene per process on one GPU;
test_animating/CLAW/test_all_CLAW_scenes.py:70-96 walks a directory of ``<scene>_input.jpg`` + ``<scene>.flo`` pairs and
starts that script once per scene.  Here a scene is one call: the frames of its clip are rendered round-robin by the
ranks of the job (parallel.shard_frames: t = r mod G), assembled by ONE all-gather (RCCL over xGMI) and written by rank 0
-- config C5 of BASELINE.json.  With one process it is the reference's flow unchanged.  tools/animate.py (one scene) and
tools/animate_scenes.py (a directory) are the command lines."""
import os
import time

import torch

from . import io, motion as motion_mod, nets, parallel, pipeline

V1_NETS = ("encoder", "projector", "net_bg", "net_alpha_encoder", "net_alpha_decoder")


def load_model(ckpt, v1, dev, motion_ckpt=None):
    """BaselineAnimator / SLRv1Animator on ``dev``; ``ckpt``: a reference checkpoint (``state_dict`` with
    ``model.module.<net>.`` keys, ``opts`` = the training Namespace) or None / 'None' for random-init networks.
    The animator gets a motion regressor (motion.MotionRegressor) when the checkpoint was trained with --train_motion (its
    ``model.module.motion_regressor.motion_predictor.`` keys) or from ``motion_ckpt``, a motion checkpoint of train_motion_unet.py
    (``model.module.motion_predictor.`` keys; it wins over the one of ``ckpt``).
    (Like the reference's scripts, this unpickles the file -- the Namespace is a pickled object: only load checkpoints you trust.)"""
    opts, sd = None, None
    if ckpt not in (None, "None", "none", ""):
        blob = torch.load(ckpt, map_location="cpu", weights_only=False)
        sd, opts = blob["state_dict"], blob.get("opts")
    regressor = None
    if motion_ckpt not in (None, "None", "none", ""):
        mblob = torch.load(motion_ckpt, map_location="cpu", weights_only=False)
        regressor = motion_mod.MotionRegressor(mblob.get("opts"), mblob["state_dict"])
    elif sd is not None and pipeline._flag(opts, "train_motion"):
        regressor = motion_mod.MotionRegressor(opts, sd, motion_mod.PREFIX_JOINT)
    if sd is None:
        torch.manual_seed(0)                       # random-init networks (plumbing / timing): the same on every rank
    model = pipeline.SLRv1Animator(opts=opts) if v1 else pipeline.BaselineAnimator(opts=opts)
    if sd is not None:
        for name in (V1_NETS if v1 else V1_NETS[:2]):
            nets.load_reference_state_dict(getattr(model, name), sd, "model.module." + name + ".")
    model.motion_regressor = regressor
    return model.to(dev).eval()


def predict_scene_motion(model, image, flow, W, points=None):
    """The motion test script's prediction (test_motion_4eval_rawsize_threshold.py:155-219) on a [1,3,W,W] device image: mask (and
    hints) from the scene's flow [1,2,h,w] (motion.motion_inputs_from_flow), then the regressor.  Returns (motion [1,2,W,W] on the
    device, speed override): the hint branch animates at speed 1 whatever the command line says (:164), else None."""
    reg = model.motion_regressor
    if reg is None:
        raise ValueError("predict_motion: the model has no motion regressor (a checkpoint trained with --train_motion, or --motion-ckpt)")
    mask = hint = None
    if reg.use_mask:
        mask, hint = motion_mod.motion_inputs_from_flow(flow, W, points=points, hints=reg.use_hint)
        mask = mask.to(image.device)
        hint = None if hint is None else hint.to(image.device)
    pred = reg.forward_flow(image, mask, hint)["PredMotion"]
    return pred, (1.0 if reg.use_hint else None)


def animate_scene(model, image_path, flow_path, out_dir, name, H, W, N, speed, align=None, rank=0, world=1, group=None,
                  video=True, half_size=False, predict_motion=False, hint_points=None, write_motion=False, score=None):
    """One scene -> out_dir/name/PredImg/%06d.png (2-layer model: + FluidImg/, CompositeFluidAlpha/, BGImg.png;
    test_v1_4eval_rawsize.py:240-284), written by rank 0, at the raw size of the image (the *_rawsize scripts) or at half
    of it (half_size: test_baseline_4eval.py / test_v1_4eval.py:160-161).  predict_motion: the motion is predicted from the image by
    the model's motion regressor, with the mask / hints derived from the scene's flow (predict_scene_motion; ``hint_points`` [(y, x)]
    pins the hints; the hint branch forces speed 1), every rank predicting it; write_motion: rank 0 also writes the field used as
    out_dir/name/Motion.flo; score: rank 0 calls score(frames) with the uint8 [n,h,w,3] device frames it writes.
    Returns (seconds of device work, frame dir)."""
    v1 = isinstance(model, pipeline.SLRv1Animator)
    dev = next(model.parameters()).device
    image, (raw_w, raw_h) = io.load_image(image_path, H, W)
    image = image.to(dev)
    if predict_motion:
        if H != W:
            raise ValueError("predict_motion: the motion test script works on a square W x W grid")
        pred, forced = predict_scene_motion(model, image, io.load_motion(flow_path), W, hint_points)
        motion = pipeline.prepare_motion(pred, H, W, speed if forced is None else forced, io.speed_align(align, name), N)
    else:
        motion = pipeline.prepare_motion(io.load_motion(flow_path), H, W, speed, io.speed_align(align, name), N)
    if half_size:
        raw_w, raw_h = raw_w // 2, raw_h // 2
    motion = motion.to(dev)
    mine = parallel.shard_frames(N, rank, world)      # (N < world: some ranks render nothing -- they still enter every
    shard = (rank, world, group) if world > 1 else None   # collective below, with empty [0,.,H,W] contributions)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if v1:
        keys = pipeline.SLRv1Animator.KEYS
        outs = model.synthesize(image, motion, N, frames=mine, shard=shard, keys=keys)
        clips = {k: (v if k == "BGImg" else parallel.gather_clip(v.contiguous(), N, rank, world, group))     # BGImg: one
                 for k, v in outs.items()}                                                             # frame-invariant image
    else:
        clips = {"PredImg": parallel.gather_clip(model.synthesize(image, motion, N, frames=mine, shard=shard), N, rank, world, group)}
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    scene = os.path.join(out_dir, name)
    frame_dir = os.path.join(scene, "PredImg")
    if rank == 0:
        if write_motion:
            os.makedirs(scene, exist_ok=True)
            io.write_flo(os.path.join(scene, "Motion.flo"), motion[0].permute(1, 2, 0).cpu().numpy())
        pred_u8 = io.frames_to_uint8(clips["PredImg"], (raw_h, raw_w))
        io.save_frames(pred_u8, scene)
        if score is not None:
            score(pred_u8)
        if v1:
            io.save_frames(io.frames_to_uint8(clips["FluidImg"], (raw_h, raw_w)), scene, key="FluidImg")
            io.save_frames(io.alpha_to_uint8(clips["CompositeFluidAlpha"], (raw_h, raw_w)), scene, key="CompositeFluidAlpha")
            io.save_image(io.frames_to_uint8(clips["BGImg"], (raw_h, raw_w))[0], os.path.join(scene, "BGImg.png"))
        if video:
            io.encode_video(frame_dir, os.path.join(scene, f"PredImg_{name}.mp4"))            # needs ffmpeg; None without
    return dt, frame_dir


def list_scenes(image_dir, flow_dir=None, align=None, start=-1, end=-1):
    """[(scene, image file, flow file)] the way test_all_CLAW_scenes.py:68-83 picks them: ``*_input.jpg`` sorted, the
    i-th kept if start <= i <= end (-1: open), scenes missing from the alignment table skipped; the flow is
    ``<scene>.flo`` next to the image (the reference ignores its flow_dir argument) or in ``flow_dir``."""
    import json
    table = None
    if align and align != "None" and os.path.exists(align):
        with open(align) as f:
            table = json.load(f)
    out = []
    images = sorted(x for x in os.listdir(image_dir) if x.endswith("_input.jpg"))
    for i, fn in enumerate(images):
        if (start != -1 and i < start) or (end != -1 and i > end):
            continue
        scene = fn[:-len("_input.jpg")]
        if table is not None and scene not in table:
            continue
        flow = os.path.join(image_dir, scene + ".flo")
        if not os.path.exists(flow) and flow_dir:
            flow = os.path.join(flow_dir, scene + ".flo")
        out.append((scene, os.path.join(image_dir, fn), flow))
    return out
