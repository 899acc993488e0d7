"""Deterministic state dicts / inputs of the motion U-Net fixtures (tests/golden/motion_vs_reference.npz, tests/golden/motion_768.npz).

Like tests/nets_fixture.py: every tensor of a reference motion-net state dict is DEFINED here from its key name and shape, so that only
key / shape lists and outputs are committed.  tools/make_golden_motion.py (needs the reference checkout) builds the reference's own
UnetMotion / SPADEUnetMaskMotion through its option parser, overwrites their state dicts with these values and stores the outputs; the
tests regenerate the same state dicts and load them into slr_sfs_amd.nets through load_motion_state_dict.  Test infrastructure only."""
import numpy as np
import torch

from nets_fixture import _rng

# reference option flags (train_animating_scripts/train_motion_scripts/train_motion_EPE_MotionGAN.sh and a plain unet_motion set)
FLAGS = {
    "spade": "--model_type SPADE_unet_mask_motion --train_motion --norm_G sync:spectral_batch --motion_norm_G sync:spectral_instance "
             "--div_flow 1.0 --use_mask_as_motion_input --use_hint_as_motion_input --motionH 256 --motionW 256 --W 256",
    "unet": "--model_type unet_motion --train_motion --norm_G sync:spectral_batch --motionH 256 --motionW 256 --W 256",
}
# case: (flag set, input shape)
CASES = {
    "unet_256": ("unet", (1, 3, 256, 256)),
    "spade_256": ("spade", (1, 6, 256, 256)),
    "spade_256x512": ("spade", (1, 6, 256, 512)),
}
PREFIX = "model.module.motion_predictor."          # a motion checkpoint of train_motion_unet.py (models/base_model_motion.py)


def state_dict(net, keys, shapes):
    """keys / shapes of the reference module's state_dict() -> {key: tensor}, every value a function of (net, key)."""
    sd = {}
    shp = {k: tuple(int(v) for v in s if v >= 0) for k, s in zip(keys, shapes)}
    for k in keys:
        s, r = shp[k], _rng("motion", net, k)
        if k.endswith("weight_u") or k.endswith("weight_v"):
            continue
        if "spade_layer" in k and k.endswith("weight"):          # SPADE mlp convolutions: small gamma / beta
            fan_in = int(np.prod(s[1:]))
            gain = 0.5 if "mlp_shared" in k else 0.1
            v = r.standard_normal(s) * gain * np.sqrt(2.0 / fan_in)
        elif k.endswith("weight_orig") or (k.endswith(".weight") and len(s) == 4):
            v = r.standard_normal(s) * np.sqrt(2.0 / int(np.prod(s[1:])))
        elif k.endswith("running_mean"):
            v = r.standard_normal(s) * 0.2
        elif k.endswith("running_var"):
            v = r.uniform(0.5, 1.5, s)                           # positive
        elif k.endswith(".weight"):                              # BN affine weight
            v = 1.0 + 0.1 * r.standard_normal(s)
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.ones(s, dtype=torch.int64)
            continue
        else:
            v = r.standard_normal(s) * 0.1
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32).reshape(s))
    for k in keys:                                               # spectral norm: u random unit, v = normalize(W^T u)
        if k.endswith("weight_u"):
            base = k[:-len("weight_u")]
            w = sd[base + "weight_orig"].double().reshape(shp[base + "weight_orig"][0], -1).numpy()
            u = _rng("motion", net, k).standard_normal(shp[k])
            u = u / np.linalg.norm(u)
            v = w.T @ u
            sd[k] = torch.from_numpy(u.astype(np.float32))
            sd[base + "weight_v"] = torch.from_numpy((v / np.linalg.norm(v)).astype(np.float32))
    missing = [k for k in keys if k not in sd]
    assert not missing, missing
    return sd


def motion_input(case, shape=None):
    """Image in [-1, 1], a binary moving-region mask (a disc), a smooth hint field times the mask."""
    N, C, H, W = shape if shape is not None else CASES[case][1]
    r = _rng("motion", case, "input", H, W)
    img = r.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
    if C == 3:
        return torch.from_numpy(img)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    mask = (((x - 0.6 * W) / W) ** 2 + ((y - 0.55 * H) / H) ** 2 < 0.09).astype(np.float32)
    hint = np.stack([3.0 * np.sin(2 * np.pi * x / W + 0.3), 2.0 * np.cos(2 * np.pi * y / H)]) * mask
    parts = [img, np.broadcast_to(mask, (N, 1, H, W)), np.broadcast_to(hint, (N, 2, H, W))]
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts, 1)[:, :C]).astype(np.float32))


def digest_positions(tag, size, n=4096):
    return _rng("motion_digest", tag, size).integers(0, size, n)
