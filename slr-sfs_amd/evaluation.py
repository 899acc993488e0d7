"""Scoring animated clips against ground truth -- the host side of tools/evaluate.py and tools/animate.py --gt-frames, counterparts of
the reference's evaluation/animation/eval_CLAW.py, eval_CLAW_fluid.py and eval_eulerian_data*.py: reading predicted and ground-truth
frames, the fluid-region mask and composite, and the metric.json layout.  The metrics themselves run on the device (metrics.py)."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

from . import io

KEYS = ("Perceptual", "PSNR", "SSIM")         # metric.json without LPIPS (no LPIPS weights given)
KEYS_LPIPS = ("LPIPS",) + KEYS                # ... and with it (metrics.LPIPSAlex): the reference's own key order, eval_CLAW.py:83-87


def metric_keys(perceptual, lpips):
    """The keys of metric.json for the metrics that were computed, in the reference's order: PSNR and SSIM always, Perceptual / LPIPS
    with their networks."""
    return tuple(k for k in KEYS_LPIPS if not ((k == "LPIPS" and not lpips) or (k == "Perceptual" and not perceptual)))


def read_frames(frame_dir, n):
    """The first ``n`` frames %06d.png / %06d.jpg of a directory -> uint8 [n,h,w,3]."""
    from PIL import Image
    out = []
    for t in range(n):
        for ext in ("png", "jpg"):
            p = os.path.join(frame_dir, "%06d.%s" % (t, ext))
            if os.path.exists(p):
                out.append(np.asarray(Image.open(p).convert("RGB")))
                break
        else:
            raise FileNotFoundError(f"{frame_dir}: frame {t} (%06d.png / .jpg) is missing")
    return np.stack(out)


def count_frames(frame_dir):
    if not os.path.isdir(frame_dir):
        return 0
    n = 0
    while any(os.path.exists(os.path.join(frame_dir, "%06d.%s" % (n, e))) for e in ("png", "jpg")):
        n += 1
    return n


def decode_video(path, n):
    """The first ``n`` frames of a video file through the ``ffmpeg`` binary -> uint8 [m,h,w,3] (m <= n); None without ffmpeg on PATH."""
    exe = shutil.which("ffmpeg")
    if exe is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call([exe, "-loglevel", "quiet", "-i", path, "-frames:v", str(n), "-start_number", "0",
                               os.path.join(d, "%06d.png")])
        return read_frames(d, count_frames(d))


def gt_source(gt_dir, name):
    """Where the ground truth of scene ``name`` is: GT_DIR/NAME/ (frames), GT_DIR/NAME.npy (uint8 [n,h,w,3]), GT_DIR/NAME.mp4 or
    GT_DIR/NAME_gt.mp4 (eval_CLAW.py:95 / eval_eulerian_data.py:84; decoded only with ffmpeg) -- (kind, path) or None."""
    for kind, path in (("frames", os.path.join(gt_dir, name)), ("npy", os.path.join(gt_dir, name + ".npy")),
                       ("video", os.path.join(gt_dir, name + ".mp4")), ("video", os.path.join(gt_dir, name + "_gt.mp4"))):
        if (kind == "frames" and count_frames(path)) or (kind != "frames" and os.path.isfile(path)):
            return kind, path
    return None


def load_gt(source, n):
    """uint8 [m,h,w,3] (m >= n when the source has enough frames) of a gt_source; None when a video cannot be decoded here."""
    kind, path = source
    if kind == "frames":
        return read_frames(path, min(n, count_frames(path)))
    if kind == "npy":
        arr = np.load(path, mmap_mode="r")
        if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
            raise ValueError(f"{path}: uint8 [n,h,w,3] expected, got {arr.dtype} {arr.shape}")
        return np.ascontiguousarray(arr[:n])
    return decode_video(path, n)


def resize_like_reference(frames_u8, hw):
    """eval_CLAW.py:100-103 per frame: v / 255 -> ToPILImage (x 255, truncated to uint8) -> Resize(hw, BILINEAR) (PIL) -> uint8 [n,h,w,3]."""
    from PIL import Image
    x = (torch.from_numpy(np.ascontiguousarray(frames_u8)).float() / 255.0).mul(255).byte().numpy()     # ToPILImage of a float tensor
    if tuple(x.shape[1:3]) == tuple(hw):
        return x
    return np.stack([np.asarray(Image.fromarray(f).resize((hw[1], hw[0]), Image.BILINEAR)) for f in x])


def fluid_mask(flow, hw):
    """eval_CLAW_fluid.py:90-95 / eval_eulerian_data_fluid.py:89-94 on the tensor as those scripts build it: F.interpolate(flow, hw,
    'bilinear').squeeze(), speed = sqrt(ch0^2 + ch1^2), mask = speed > 0.1 mean(speed) -> float [1,h,w].  Note: for a .flo file the
    reference passes read_flo's [h,w,2] array as a [1,h,w,2] tensor (fluid_flow_tensor), so its "channels" 0 and 1 are the first two
    ROWS of the flow, interpolated over a (w, 2) grid; this reproduces that, so the masks -- and metric_fluid.json -- are the reference's."""
    f = F.interpolate(flow.float(), tuple(hw), mode="bilinear").squeeze()
    speed = (f[0:1, :, :] ** 2 + f[1:2, :, :] ** 2).sqrt()
    return (speed > speed.mean() * 0.1).float()


def fluid_flow_tensor(path):
    """The flow of a fluid-mode scene as the reference's scripts hold it: .flo -> torch.FloatTensor(read_flo(path)).unsqueeze(0)
    ([1,h,w,2], eval_CLAW_fluid.py:90); .pth -> load_compressed_tensor ([1,2,h,w], eval_eulerian_data_fluid.py:89)."""
    if path.endswith(".flo"):
        return torch.from_numpy(io.read_flo(path)).unsqueeze(0)
    return io.load_motion(path)


def load_input_image(path, hw):
    """NAME_input.jpg -> Resize(hw, BILINEAR) -> ToTensor: float [3,h,w] (eval_CLAW_fluid.py:97-99)."""
    from PIL import Image
    img = Image.open(path).convert("RGB").resize((hw[1], hw[0]), Image.BILINEAR)
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()


def fluid_composite(pred_u8, image, mask):
    """pred * mask + image * (1 - mask) (eval_CLAW_fluid.py:109) with pred = ToTensor(frame): uint8 [n,h,w,3] -> float [n,3,h,w]."""
    pred = pred_u8.permute(0, 3, 1, 2).float() / 255.0
    return (pred * mask + image * (1.0 - mask)).contiguous()


def aggregate(per_scene, keys=KEYS):
    """metric.json of eval_CLAW.py:79-160 (keys=KEYS_LPIPS: all of it; the default: without LPIPS): {name: {key: [per-frame values]}} ->
    Total<key> (np.mean over every frame of every scene), Total<key>_std (np.std), <key> {name: mean} and <key>_std {name: std}, in the
    reference's key order."""
    res = {}
    for k in keys:
        res[f"Total{k}"] = {}
    for k in keys:
        res[f"Total{k}_std"] = {}
    for k in keys:
        res[k] = {}
    for k in keys:
        res[f"{k}_std"] = {}
    for name, vals in per_scene.items():
        for k in keys:
            v = np.array(vals[k])
            res[k][name] = float(np.mean(v))
            res[f"{k}_std"][name] = float(np.std(v))
    for k in keys:
        allv = np.array([x for vals in per_scene.values() for x in vals[k]])
        res[f"Total{k}"] = float(np.mean(allv))
        res[f"Total{k}_std"] = float(np.std(allv))
    return res
