"""Deterministic state and batch of the joint-training fixture (tests/golden/joint_train_vs_reference.npz), shared by
tools/make_golden_joint_train.py (which runs the reference's ``AnimatingSoftmaxSplating`` with ``--train_motion`` on them) and the tests
(which regenerate them): only recorded results are committed.  The generator's initial state is the one of
tests/golden/train_step_vs_reference.npz (the narrow widths of tools/make_golden_train_step.py; its tensors do not depend on the image
size), the motion network's is tests/motion_train_fixture.py's at num_filters = 8; the batch is one sample at 256 x 256 with the index
triple [3, 10, 40].  Test infrastructure only."""
import functools
import os

import numpy as np
import torch

import motion_train_fixture as TF
import train_step_f64 as T
from nets_fixture import _rng

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "joint_train_vs_reference.npz")
W, NF, BS = 256, TF.NF, 1
INDEX = [[3, 10, 40]]
DIV_FLOW = 2.0                       # not 1: feeding pred * div_flow to the integration must show
LOSSES = ["1.0_l1"]
MOTION_LOSSES = ["10.0_EndPointError"]
MOTION_MODEL_TYPE = "SPADE_unet_mask_motion"
# The batch seed.  At seed 0, 98 % and 94 % of the pixels stay inside the image in the two directions of the reference's integration of
# its own predicted flow (7 steps forwards, 31 backwards; tests/test_joint_train_host.py asserts at least half).  A seed at which no
# batch-norm gate of the generator flips between float32 and float64 at 256 x 256 (DESIGN 3.17 chooses its seed that way for the motion
# network alone) was looked for among 0 .. 8 and not found: E(def32) of PredImg is 3.7e-2 at seed 0, the smallest, and 4.8e-2 .. 5.8e-1
# at the others.  PredMotion has none at any of them (E(def32) 8e-7 .. 3e-6).
SEED = 0
FLAGS = ("--model_type softmax_splating --refine_model_type resnet_256W8UpDown64_de_resnet_pconv2_nonorm --pconv pconv_pbn_woresbias "
         "--norm_G sync:spectral_batch --normalize_image --train_Z --use_softmax_splatter --use_inverse_depth "
         f"--losses {' '.join(LOSSES)} --discriminator_losses pix2pixHD --ndf {T.NDF} --ngf {T.FEAT} --out_channel {T.FEAT} --W {W} "
         f"--train_motion --motion_model_type {MOTION_MODEL_TYPE} --motion_norm_G sync:spectral_instance --use_mask_as_motion_input "
         f"--use_hint_as_motion_input --motionH {W} --motionW {W} --div_flow {DIV_FLOW} --motion_losses {' '.join(MOTION_LOSSES)}")


def options(**more):
    """The fixture's options as this package reads them (train_step_f64.options plus the flags of --train_motion)."""
    kw = dict(W=W, losses=list(LOSSES), train_motion=True, motion_model_type=MOTION_MODEL_TYPE, motion_norm_G="sync:spectral_instance",
              use_mask_as_motion_input=True, use_hint_as_motion_input=True, motionH=W, motionW=W, div_flow=DIV_FLOW,
              motion_losses=list(MOTION_LOSSES))
    kw.update(more)
    return T.options(**kw)


def batch(seed=None):
    """{"images": [start, middle, end] [1,3,256,256] in [-1, 1], sharing their low frequencies; "motions", "hints": sample 0 of
    motion_train_fixture.batch(seed); "index" [1,3]}, float32 on the host."""
    seed = SEED if seed is None else seed
    r = _rng("joint_train", "batch", seed)
    y, x = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    base = np.stack([np.sin(x / 23 + c) * np.cos(y / 31 - c) for c in range(3)])[None]
    images = [torch.from_numpy(np.clip(0.7 * base + 0.25 * r.standard_normal((BS, 3, W, W)), -1, 1).astype(np.float32)) for _ in range(3)]
    m = TF.batch(seed)
    return {"images": images, "motions": m["motions"][:BS].contiguous(), "hints": m["hints"][:BS].contiguous(),
            "index": torch.tensor(INDEX, dtype=torch.int64)}


@functools.lru_cache(maxsize=None)
def generator_fixture():
    """tests/golden/train_step_vs_reference.npz: the generator's initial state under ``sd/`` (noise and results of that fixture unused)."""
    return T.load()


def generator_state():
    """{reference key without prefix: float32 tensor} of encoder and projector (buffers included), and min_z / max_z / discretized_zs."""
    return {k[3:]: torch.from_numpy(v) for k, v in generator_fixture().items() if k.startswith("sd/")}


def motion_state():
    """{key of SPADEUnet4MaskMotion(num_filters=8): float32 tensor}."""
    return dict(TF.initial_state())


def reference_state_dict(prefix="model.module."):
    """The joint model's initial state under the reference's keys (no VGG19: the fixture's losses are L1 alone)."""
    sd = {prefix + k: v.clone() for k, v in generator_state().items()}
    sd.update({prefix + "motion_regressor.motion_predictor." + k: v.clone() for k, v in motion_state().items()})
    return sd


@functools.lru_cache(maxsize=None)
def load(path=GOLDEN):
    g = np.load(path)
    return {k: g[k] for k in g.files}


def noise_lists(g):
    """train_step_f64.noise_lists on the joint fixture's recorded noise."""
    return T.noise_lists(g)


def positions(name, size):
    return TF.positions("joint/" + name, size)
