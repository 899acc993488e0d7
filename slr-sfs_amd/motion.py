"""Motion prediction from a still image: the motion regressor of the reference (models/unet_motion.py:30-191) on this package's
kernels (nets.Unet4Motion / nets.SPADEUnet4MaskMotion, csrc/motion.hip), and the input preparation of its motion test script
(test_animating/test_motion_4eval_rawsize_threshold.py:155-219): moving-region mask and motion hints derived from a flow file.

Hint positions: the reference clusters the moving pixels with sklearn's KMeans (5 clusters, np.random.seed(5)), whose result depends on
sklearn's version.  Here ``hint_points`` is a small deterministic k-means of our own (k-means++ seeding from a fixed generator, Lloyd
iterations to a fixed point, int() of the cluster means like :186-189): its positions are NOT sklearn's, so a predicted field can differ
from the reference's where the hints differ.  Pass ``points`` to pin them."""
import numpy as np
import torch
import torch.nn.functional as F

from . import nets

MOTION_MODEL_TYPES = ("unet_motion", "SPADE_unet_mask_motion")
SPEED_THRESHOLD = 0.2161635                   # :178
MAX_HINT = 5                                  # :182

PREFIX_JOINT = "model.module.motion_regressor.motion_predictor."   # an animating checkpoint trained with --train_motion
PREFIX_MOTION = "model.module.motion_predictor."                    # a motion checkpoint of train_motion_unet.py (models/base_model_motion.py)


def _get(opts, name, default=None):
    if opts is None:
        return default
    if isinstance(opts, dict):
        return opts.get(name, default)
    return getattr(opts, name, default)


def _has(opts, name):
    return opts is not None and ((name in opts) if isinstance(opts, dict) else hasattr(opts, name))


class MotionRegressor(torch.nn.Module):
    """UnetMotion / SPADEUnetMaskMotion (unet_motion.py:30-191) for inference.  ``opts``: the pickled training Namespace (or a dict).  The
    network is opts.model_type when that is a motion model (a motion checkpoint), else opts.motion_model_type (an animating checkpoint
    with --train_motion: the reference's get_model(opts with model_type = motion_model_type), animating_softmax_splating.py:190-193).
    Input channels: 3 + use_mask_as_motion_input + 2 * use_hint_as_motion_input (:34-41); div_flow = opts.div_flow when the Namespace
    has it, else 20.0 (:33).  ``state_dict``: a reference state dict, loaded under ``prefix`` (default: the joint-checkpoint prefix if
    present, else the motion-checkpoint one)."""

    def __init__(self, opts, state_dict=None, prefix=None):
        super().__init__()
        mt = _get(opts, "model_type")
        if mt not in MOTION_MODEL_TYPES:
            mt = _get(opts, "motion_model_type")
        if mt not in MOTION_MODEL_TYPES:
            raise ValueError(f"MotionRegressor: motion model type {mt!r} is not supported (one of {MOTION_MODEL_TYPES})")
        self.model_type = mt
        self.use_mask = bool(_get(opts, "use_mask_as_motion_input", False))
        self.use_hint = bool(_get(opts, "use_hint_as_motion_input", False))
        cin = 3 + int(self.use_mask) + 2 * int(self.use_hint)
        self.div_flow = float(_get(opts, "div_flow")) if _has(opts, "div_flow") else 20.0
        if mt == "unet_motion":
            norm = str(_get(opts, "norm_G", "")).split(":")
            if len(norm) < 2 or norm[1] not in ("batch", "spectral_batch"):
                raise ValueError(f"MotionRegressor: unet_motion with norm_G {_get(opts, 'norm_G')!r}: only the BatchNorm forms are supported")
            self.motion_predictor = nets.Unet4Motion(cin)
        else:
            if _has(opts, "motion_norm_G") and str(_get(opts, "motion_norm_G")).split(":")[-1] != "spectral_instance":
                raise ValueError(f"MotionRegressor: SPADE_unet_mask_motion with motion_norm_G {_get(opts, 'motion_norm_G')!r}: "
                                 "only the instance-norm form is supported")
            self.motion_predictor = nets.SPADEUnet4MaskMotion(cin)
        if state_dict is not None:
            if prefix is None:
                prefix = PREFIX_JOINT if any(k.startswith(PREFIX_JOINT) for k in state_dict) else PREFIX_MOTION
            nets.load_motion_state_dict(self.motion_predictor, state_dict, prefix)
        self.eval()

    @torch.no_grad()
    def forward_flow(self, image, gt_mask=None, gt_hint=None):
        """{"PredMotion": predictor(cat(image, gt_mask, gt_hint)) * div_flow} (unet_motion.py:93-109, 174-191).  image [N,3,H,W] in
        [-1, 1] on the device, gt_mask [N,1,H,W], gt_hint [N,2,H,W] when the network takes them; H, W multiples of 256."""
        parts = [image]
        if self.use_mask:
            if gt_mask is None or (self.use_hint and gt_hint is None):
                raise ValueError("MotionRegressor.forward_flow: this network takes the moving-region mask"
                                 + (" and the motion hints" if self.use_hint else "") + " (motion_inputs_from_flow)")
            parts.append(gt_mask.to(image))
            if self.use_hint:
                parts.append(gt_hint.to(image))
        x = torch.cat(parts, 1).contiguous() if len(parts) > 1 else image.contiguous()
        return {"PredMotion": self.motion_predictor(x) * self.div_flow}

    def forward(self, image, gt_mask=None, gt_hint=None):
        return self.forward_flow(image, gt_mask, gt_hint)["PredMotion"]


def hint_points(mask, k=MAX_HINT, seed=5, max_iter=300):
    """k hint pixels [(y, x)] of a boolean [h, w] moving-region mask: deterministic k-means over the (x, y) coordinates of its pixels
    (k-means++ seeding from np.random.default_rng(seed), Lloyd iterations until the assignment no longer changes), then int() of each
    cluster's mean (:186-189).  Not sklearn's KMeans: the positions differ from the reference's."""
    m = torch.as_tensor(mask).bool().cpu().numpy()
    ys, xs = np.nonzero(m)                                     # row-major, like torch.where on the flattened mask (:184)
    X = np.stack([xs, ys], 1).astype(np.float64)
    rng = np.random.default_rng(seed)
    centers = [X[rng.integers(len(X))]]
    for _ in range(1, k):
        d2 = np.min(((X[:, None, :] - np.asarray(centers)[None]) ** 2).sum(-1), 1)
        tot = d2.sum()
        centers.append(X[rng.choice(len(X), p=d2 / tot)] if tot > 0 else X[rng.integers(len(X))])
    C = np.asarray(centers)
    labels = None
    for _ in range(max_iter):
        new = np.argmin(((X[:, None, :] - C[None]) ** 2).sum(-1), 1)
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        C = np.stack([X[labels == i].mean(0) if np.any(labels == i) else C[i] for i in range(k)])
    return [(int(c[1]), int(c[0])) for c in C]


def motion_inputs_from_flow(gt_motion, W, points=None, hints=True):
    """The motion test script's network inputs from a scene's flow [1,2,h,w] (:155-219), on the CPU.
    hints=True (the mask + hint network, :162-213): mask = speed > 0.2161635 at the flow's own resolution; 5 hints at ``points`` [(y, x)]
    (default: hint_points of the mask) spread with Gaussian weights (sigma = h / 5), normalised (a zero norm -> 1) and multiplied by the
    mask; zero hints if the mask has fewer than 5 pixels; then the mask and the hints nearest-resized to W x W.  Returns (mask, hint).
    hints=False (:214-219): the flow nearest-resized to W x W, mask = 1 - (speed < 0.1 * mean speed).  Returns (mask, None).
    (The script's hint branch also sets the animation speed to 1, :164: callers apply that themselves.)"""
    gt = torch.as_tensor(gt_motion).detach().float().cpu()
    if not hints:
        g = F.interpolate(gt, (W, W))
        sp = (g[:, 0:1] ** 2 + g[:, 1:2] ** 2).sqrt()
        return 1.0 - (sp < sp.mean([1, 2, 3], True) * 0.1).float(), None
    _, _, h, w = gt.shape
    xs = torch.linspace(0, w - 1, w).view(1, 1, w).repeat(1, h, 1)
    ys = torch.linspace(0, h - 1, h).view(1, h, 1).repeat(1, 1, w)
    xys = torch.cat((xs, ys), 1).view(2, -1)
    speed = (gt[:, 0:1] ** 2 + gt[:, 1:2] ** 2).sqrt().view(1, 1, h, w)
    mask = (speed > SPEED_THRESHOLD).float()
    if int(mask.sum().long()) < MAX_HINT:
        dense = torch.zeros(gt.shape)
    else:
        pts = hint_points(mask[0, 0] > 0) if points is None else [(int(py), int(px)) for py, px in points]
        if len(pts) != MAX_HINT:
            raise ValueError(f"motion_inputs_from_flow: {MAX_HINT} hint points expected, got {len(pts)}")
        dense = torch.zeros(gt.shape).view(1, 2, -1)
        norm = torch.zeros(gt.shape).view(1, 2, -1)
        sigma = h / MAX_HINT
        for hy, hx in pts:
            dist = ((xys - xys.view(2, h, w)[:, hy, hx].unsqueeze(1)) ** 2).sum(0, True).sqrt()
            weight = (-(dist / sigma) ** 2).exp().unsqueeze(0)
            dense += weight * gt[:, :, hy, hx].unsqueeze(2)
            norm += weight
        norm[norm == 0.0] = 1.0
        dense = (dense / norm).view(1, 2, h, w) * mask
    return F.interpolate(mask, (W, W), mode="nearest"), F.interpolate(dense, (W, W))
