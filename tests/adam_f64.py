"""torch.optim.Adam's update (no weight decay, no amsgrad) written out once, in whatever dtype its tensors have: float64 as the reference
of the tests, float32 on the CPU as the plain-fp32 yardstick E_plain32.  The scalars (lr, betas, eps, the bias corrections) are Python
floats, as they are in torch.optim.Adam."""
import functools
import math
import os
import re

import torch


def step(p, g, m, v, t, lr, beta1, beta2, eps=1e-8):
    """One update.  ``t``: the step count AFTER this step (1 for the first).  Returns the new (p, m, v); nothing is changed in place."""
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def run(p, grads, m, v, t0, lrs, beta1, beta2, eps=1e-8, dtype=torch.float64, update=None):
    """``len(grads)`` updates from the state (p, m, v, t0 steps taken) with gradient ``grads[k]`` and learning rate ``lrs[k]`` (or the one
    number ``lrs``) in step k, everything converted to ``dtype`` first; ``update``: another formula than ``step``.  Returns (p, m, v, steps taken)."""
    p, m, v = p.to(dtype), m.to(dtype), v.to(dtype)
    for k, g in enumerate(grads):
        lr = lrs[k] if isinstance(lrs, (list, tuple)) else lrs
        p, m, v = (update or step)(p, g.to(dtype), m, v, t0 + k + 1, lr, beta1, beta2, eps)
    return p, m, v, t0 + len(grads)


def E(got, ref):
    """The project's error measure: max|got - ref| / max|ref|, no floor."""
    ref = ref.double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---- the wrong formulas the criterion has to tell from the right one (tests/test_adam_host.py measures them)

def step_eps_inside_sqrt(p, g, m, v, t, lr, beta1, beta2, eps=1e-8):
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    return p - (lr / bc1) * m / (v / bc2 + eps).sqrt(), m, v


def step_without_second_correction(p, g, m, v, t, lr, beta1, beta2, eps=1e-8):
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    return p - (lr / (1 - beta1 ** t)) * m / (v.sqrt() + eps), m, v


# ---- the inputs the host and the device tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (beta1, beta2, lr, gradient scale, steps already taken): the reference's discriminator-training betas at lr_g; torch's defaults with
# small gradients; gradients of the size of eps (eps inside the root shows here); a resumed state with both moments set
SETTINGS = ((0.0, 0.9, 5e-4, 1.0, 0), (0.9, 0.999, 2e-3, 1e-3, 0), (0.0, 0.9, 2e-3, 1e-8, 0), (0.5, 0.9, 2e-3, 1.0, 1000))
KS = (1, 5)
VIEWS = ((37, 1, 2), (4101, 2, 3), (260, 3, 1))          # (elements, element offset of the parameter, of the gradient) in larger buffers


def chunk():
    """SLR_ADAM_CHUNK of include/slr_splat.h: the elements of a work item of the update kernel."""
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    return int(re.search(r"#define\s+SLR_ADAM_CHUNK\s+(\d+)", hdr).group(1))


def sizes():
    """Below, at and above a float4, a wavefront and a work item; an empty tensor; more than two work items with a scalar tail."""
    C = chunk()
    return [1, 3, 4, 5, 0, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3]


@functools.lru_cache(maxsize=None)
def case(si):
    """Setting ``si``: per tensor (the sizes above, then the views) float32 p0, m0, v0, max(KS) gradients, and the written-out update
    after K steps in float64 and in float32, computed once.  Parameters at scale 4 lr (the update is of the parameter's own size);
    every seventh element of the first gradient is exactly 0."""
    beta1, beta2, lr, gs, t0 = SETTINGS[si]
    # (seeds at which no update cancels its parameter in the one- and three-element tensors: E is relative to max|ref| per tensor, and
    #  tests/test_adam_host.py asserts that E_plain32 is fp32 rounding, below 1e-6, for every tensor of every setting)
    gen = torch.Generator().manual_seed(9300 + si)
    r = lambda n: torch.randn(n, generator=gen)                            # noqa: E731
    tensors = []
    for n in sizes() + [v[0] for v in VIEWS]:
        p0 = r(n) * (4 * lr)
        grads = [r(n) * gs for _ in range(max(KS))]
        grads[0][::7] = 0.0
        m0, v0 = (r(n) * (0.5 * gs), (r(n) * gs).square() + 1e-3 * gs * gs) if t0 else (torch.zeros(n), torch.zeros(n))
        ref = {(K, dt): run(p0, grads[:K], m0, v0, t0, lr, beta1, beta2, dtype=dt) for K in KS for dt in (torch.float64, torch.float32)}
        tensors.append(dict(p0=p0, m0=m0, v0=v0, grads=grads, ref=ref))
    return tensors
