"""Deterministic state and batch of the motion-training fixture (tests/golden/motion_train_vs_reference.npz), shared by
tools/make_golden_motion_train.py (which runs the reference on them) and the tests (which regenerate them): only recorded results are
committed.  Test infrastructure only."""
import functools

import numpy as np
import torch

import motion_fixture as MF
from nets_fixture import _rng

NF, N, SIZE = 8, 2, 256
MOTION_LOSSES = ["10.0_EndPointError"]
DIV_FLOW = 1.0
# The batch seed: the first of 0, 1, ... for which neither float32 arithmetic (torch on the CPU, the kernels) flips one of the ~1e7 gates of
# a forward against float64, in train() or in eval() mode ("Gates at 256 x 256"): seeds 0 - 4 each have a flip somewhere.
SEED = 5
PREFIX = MF.PREFIX


def state(keys, shapes, seed=0):
    """{key: float32 tensor} of SPADEUnet4MaskMotion(num_filters=NF) from motion_fixture.state_dict (u random unit, v = normalize(W^T u))."""
    return MF.state_dict(f"spade_train{seed}", list(keys), [tuple(s) for s in shapes])


def batch(seed=None):
    """images [[N,3,S,S]] in [-1, 1]; a smooth motion field that is zero outside a disc (the static region of the mask); hints: the motion
    at a sparse lattice of pixels, zero elsewhere."""
    r = _rng("motion_train", "batch", SEED if seed is None else seed)
    img = r.uniform(-1, 1, (N, 3, SIZE, SIZE)).astype(np.float32)
    y, x = np.meshgrid(np.arange(SIZE, dtype=np.float32), np.arange(SIZE, dtype=np.float32), indexing="ij")
    motions, hints = [], []
    for n in range(N):
        cx, cy, ph = 0.45 + 0.15 * n, 0.55 - 0.1 * n, 0.3 + 1.1 * n
        disc = (((x / SIZE - cx) ** 2 + (y / SIZE - cy) ** 2) < 0.1).astype(np.float32)
        m = np.stack([3.0 * np.sin(2 * np.pi * x / SIZE + ph) + 0.5, 2.0 * np.cos(2 * np.pi * y / SIZE - ph) - 0.4]) * disc
        m = m + 0.05 * r.standard_normal(m.shape) * disc
        lattice = ((x % 32 == 16) & (y % 32 == 16)).astype(np.float32)
        motions.append(m)
        hints.append(m * lattice)
    return {"images": [torch.from_numpy(img)], "motions": torch.from_numpy(np.stack(motions).astype(np.float32)),
            "hints": torch.from_numpy(np.stack(hints).astype(np.float32))}


def positions(name, size):
    return MF.digest_positions("motion_train/" + name, size, n=256)


# The biases of the convolutions in front of an instance norm (conv2..conv7, dconv1..dconv7): the norm removes every plane's mean, so
# their gradient is EXACTLY zero and what any arithmetic returns is its rounding noise (1e-16 in float64).  E = max|got - ref| / max|ref|
# means nothing there; their error is measured relative to max|.| of the same layer's weight gradient instead (the same sum over the
# output gradient, weighted by activations of order 1).
ZERO_GRAD_BIASES = tuple(f"conv{i}.bias" for i in range(2, 8)) + tuple(f"dconv{i}.bias" for i in range(1, 8))


def grad_scale(grads64, key):
    """max|.| that the error of gradient ``key`` is taken relative to."""
    return float(grads64[key.replace(".bias", ".weight_orig") if key in ZERO_GRAD_BIASES else key].double().abs().max())


@functools.lru_cache(maxsize=None)
def initial_state():
    """{reference key: float32 tensor} at num_filters = NF."""
    import motion_train_f64 as M64
    shapes = M64.param_shapes(NF)
    return state(list(shapes), list(shapes.values()))


@functools.lru_cache(maxsize=None)
def definition(dtype, training):
    """tests/motion_train_f64.model_step on the fixture's state and batch in ``dtype`` ("float64" / "float32"), computed once and shared:
    (losses, pred_dict, gradients, state after the forward).  Nobody modifies what it returns."""
    import motion_train_f64 as M64
    dt = getattr(torch, dtype)
    b = batch()
    P = {k: v.to(dt) for k, v in initial_state().items()}
    with torch.no_grad():
        return M64.model_step(P, b["images"][0].to(dt), b["motions"].to(dt), b["hints"].to(dt), MOTION_LOSSES, DIV_FLOW, training)
