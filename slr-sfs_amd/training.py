"""The splat half of the reference's training step (models/animating_softmax_splating.py:577-692) as one differentiable operator.

``splat_blend`` replaces the weighting by ``exp(clamp(Z - Z.max()))`` and the blend factor, the two ``torch.cat``, the two 65-plane
summation splats, the in-place adds on views, the clamp and the division -- and autograd's mirror image of all of them -- by
``slr_splat_blend_forward`` / ``slr_splat_blend_backward`` (csrc/blend.hip).  ``TrainingSynthesis`` puts the package's differentiable
``EulerIntegration`` and the blend factor in front of it, with the option flags read the way the reference's ``forward()`` reads them.
There is no fallback: CPU tensors raise, a missing library raises.
"""
import math

import torch

from ._lib import BLEND_DETERMINISTIC, WS_CLEAN, call, lib, require_device, workspace
from .euler_integration_manipulator import EulerIntegration, euler_integration_pair

_UNSUPPORTED = ("use_softmax_splatter_v2", "use_softmax_splatter_v3", "use_3d_splatter", "use_mesh_splatter", "random_ff_mask")


def _check_inputs(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha):
    """Device, dtype, contiguity and shapes -- before anything touches the device (softsplat._check_pair / _lib.require_device)."""
    tensors = (start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha)
    for t in tensors:
        if t is not None and not torch.is_tensor(t):
            raise TypeError(f"slr_sfs_amd.splat_blend: tensors required, got {type(t).__name__}")
    for t in tensors:                                   # (the reference raises NotImplementedError for CPU tensors, softsplat.py:418-419)
        if t is not None and not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype}")
    if start_fs.dim() != 4 or min(start_fs.shape) < 1:
        raise ValueError(f"splat_blend: features [N,C,H,W] with N, C, H, W >= 1 required, got {tuple(start_fs.shape)}")
    N, C, H, W = start_fs.shape
    if tuple(end_fs.shape) != (N, C, H, W):
        raise ValueError(f"splat_blend: end_fs {tuple(end_fs.shape)} does not match start_fs {(N, C, H, W)}")
    for name, f in (("flow_f", flow_f), ("flow_p", flow_p)):
        if tuple(f.shape) != (N, 2, H, W):
            raise ValueError(f"splat_blend: {name} {tuple(f.shape)}, expected {(N, 2, H, W)}")
    for name, z in (("z_start", z_start), ("z_end", z_end)):
        if z is not None and tuple(z.shape) != (N, 1, H, W):
            raise ValueError(f"splat_blend: {name} {tuple(z.shape)}, expected {(N, 1, H, W)}")
    if alpha.numel() != N:
        raise ValueError(f"splat_blend: alpha has {alpha.numel()} elements for a batch of {N}")
    for name, t in (("start_fs", start_fs), ("z_start", z_start), ("flow_f", flow_f), ("end_fs", end_fs), ("z_end", z_end),
                    ("flow_p", flow_p), ("alpha", alpha)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"splat_blend: {name} is not contiguous")
    require_device(*tensors)


def _global_max(z):
    result, scratch = z.new_empty(1), z.new_empty(1024)
    call("slr_global_max", z.device, z, z.numel(), result, scratch)
    return result


class _SplatBlend(torch.autograd.Function):
    """forward(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, lo, hi, subtract_max, eps[, deterministic]); saved: the inputs,
    the two maxima, the output and one normaliser plane per sample."""

    @staticmethod
    def forward(ctx, start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, lo, hi, subtract_max, eps, deterministic=False):
        N, C, H, W = start_fs.shape
        dev = start_fs.device
        zmax_f = _global_max(z_start) if subtract_max and z_start is not None else None
        zmax_p = (zmax_f if z_end is z_start else _global_max(z_end)) if subtract_max and z_end is not None else None
        out, norm = torch.empty_like(start_fs), start_fs.new_empty(N, 1, H, W)
        nbytes = int(lib().slr_splat_blend_ws_bytes(N, C, H, W))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ws = workspace(start_fs, "a", N, C, H, W)
        call("slr_splat_blend_forward_ex", dev, start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, zmax_f, zmax_p, lo, hi, eps,
             out, norm, N, C, H, W, ws, ws.numel(), WS_CLEAN, BLEND_DETERMINISTIC if deterministic else 0, scratch, nbytes)
        ctx.save_for_backward(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, zmax_f, zmax_p, out, norm)
        ctx.consts = (lo, hi, eps)
        ctx.mark_non_differentiable(norm)
        return out, norm

    @staticmethod
    def backward(ctx, grad_out, _grad_norm):
        start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, zmax_f, zmax_p, out, norm = ctx.saved_tensors
        lo, hi, eps = ctx.consts
        grad_out = grad_out.contiguous()
        require_device(grad_out)
        N, C, H, W = start_fs.shape
        need = ctx.needs_input_grad
        grads = [torch.empty_like(t) if need[k] and t is not None else None
                 for k, t in enumerate((start_fs, z_start, flow_f, end_fs, z_end, flow_p))]
        if any(g is not None for g in grads):
            nbytes = int(lib().slr_splat_blend_ws_bytes(N, C, H, W))
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=start_fs.device)
            call("slr_splat_blend_backward", start_fs.device, start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, zmax_f, zmax_p,
                 lo, hi, eps, out, norm, grad_out, *grads, N, C, H, W, scratch, nbytes)
        return (*grads, None, None, None, None, None, None)


def splat_blend(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, clamp_z=(-20.0, 20.0), subtract_max=True, eps=1e-8,
                return_norm=False, deterministic=False):
    """out = (splat(start_fs w_f, flow_f) + splat(end_fs w_p, flow_p)) / max(splat(w_f, flow_f) + splat(w_p, flow_p), eps), [N,C,H,W], with
    w_f = exp(clamp(z_start - z_start.max())) * alpha, w_p = exp(clamp(z_end - z_end.max())) * (1 - alpha) -- the reference's
    animating_softmax_splating.py:587-692, differentiable in all six tensors (``needs_input_grad`` is honoured: a gradient nobody
    asked for is neither computed nor allocated, and comes back as None).

    start_fs / end_fs [N,C,H,W], z_start / z_end [N,1,H,W] or None (weights alpha / 1 - alpha only: ``train_Z`` off), flow_f / flow_p
    [N,2,H,W], alpha: N values on the device (any shape; not differentiated).  clamp_z: (lo, hi) or None (``no_clamp_Z``);
    subtract_max=False: ``use_softmax_splatter_v1``.  The same tensor may serve both directions: autograd adds its two gradients.
    return_norm: also the normaliser plane [N,1,H,W] (no gradient).
    deterministic (a bool; anything else raises TypeError): the forward's deterministic tile kernels -- out and the normaliser are the same
    bits from run to run, whatever else the device is doing, while ``splat_blend_fallback_count`` reads 0.  The backward has
    that property already, given the forward's result.  torch's global deterministic-algorithms switch is not consulted.

    d/dz: zero where the clamp bites, and the maximum's element also receives minus the sum of the others'.  Where several elements
    hold the maximum, the first one in memory receives all of it -- torch splits it evenly among them; for a learnt logit plane a tie is
    a rounding accident.  A source pixel whose target coordinate is not representable (non-finite flow, |x + flow| >= 2^30) contributes
    nothing and its gradients are exactly 0.  CPU tensors raise NotImplementedError; wrong dtype, shape or layout raise before the device
    is touched."""
    if not isinstance(deterministic, bool):
        raise TypeError(f"slr_sfs_amd.splat_blend: deterministic must be a bool, got {type(deterministic).__name__}")
    _check_inputs(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha)
    lo, hi = (-math.inf, math.inf) if clamp_z is None else (float(clamp_z[0]), float(clamp_z[1]))
    if not lo <= hi:
        raise ValueError(f"splat_blend: clamp_z {clamp_z!r} is not a range")
    if not float(eps) > 0.0:
        raise ValueError(f"splat_blend: eps must be positive, got {eps!r}")
    out, norm = _SplatBlend.apply(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha.detach().reshape(-1), lo, hi,
                                  bool(subtract_max), float(eps), deterministic)
    return (out, norm) if return_norm else out


def splat_blend_fallback_count(features):
    """The capacity fallbacks that deterministic ``splat_blend`` calls on tensors of this shape, device and stream have taken so far:
    a one-element int32 DEVICE tensor -- a view of the cached splat workspace's sticky word (slr_splat_fallback_count_offset), read
    without a synchronisation; zero when the workspace is made, never reset.  The run-to-run guarantee holds while it is 0."""
    require_device(features)
    N, C, H, W = features.shape
    ws = workspace(features, "a", N, C, H, W)
    off = int(lib().slr_splat_fallback_count_offset(N, H, W))
    return ws[off:off + 4].view(torch.int32)


def _flag(opts, name):
    """``"name" in self.opt and self.opt.name`` of the reference, for an argparse.Namespace, a dict, or None."""
    if opts is None:
        return False
    return bool(opts.get(name, False) if isinstance(opts, dict) else getattr(opts, name, False))


def _has(opts, name):
    """``"name" in self.opt``: attribute EXISTENCE, whatever the value."""
    if opts is None:
        return False
    return (name in opts) if isinstance(opts, dict) else hasattr(opts, name)


def _blend_options(opts):
    """The training step's option flags -> keyword arguments of splat_blend, the way the reference's forward() reads them
    (animating_softmax_splating.py:588, 593-605): ``train_Z`` (off: the logits are not used), ``use_softmax_splatter_v1`` (nothing is
    subtracted), EXISTENCE of ``no_clamp_Z`` (whatever its value: no clamp).  The paths this operator does not implement raise
    NotImplementedError naming the flag."""
    for name in _UNSUPPORTED:
        if _flag(opts, name):
            raise NotImplementedError(f"slr_sfs_amd.TrainingSynthesis: option {name} is not implemented")
    return dict(train_z=_flag(opts, "train_Z"), subtract_max=not _flag(opts, "use_softmax_splatter_v1"),
                clamp_z=None if _has(opts, "no_clamp_Z") else (-20.0, 20.0))


class TrainingSynthesis(torch.nn.Module):
    """The reference's forward() from the Euler integration to the normalised features (animating_softmax_splating.py:577-692):
    forward(start_fs, Z_f, end_fs, Z_p, motion, start_index, middle_index, end_index) -> [B,C,H,W], differentiable in the features, the
    logits and the motion field, without a host synchronisation when the indices are device tensors.  With ``train_Z`` off Z_f / Z_p are
    ignored (the reference replaces them by ones, whose weights cancel).  ``deterministic``: passed on to ``splat_blend``.
    ``euler_pair``: both integrations through ``euler_integration_pair`` -- the same flows bit for bit, one launch, and a gradient
    w.r.t. the motion field that is the same bits from run to run (for a motion field that is itself being trained)."""

    def __init__(self, opts=None, deterministic=False, euler_pair=False):
        super().__init__()
        if not isinstance(deterministic, bool):
            raise TypeError(f"slr_sfs_amd.TrainingSynthesis: deterministic must be a bool, got {type(deterministic).__name__}")
        if not isinstance(euler_pair, bool):
            raise TypeError(f"slr_sfs_amd.TrainingSynthesis: euler_pair must be a bool, got {type(euler_pair).__name__}")
        self.euler_pair = euler_pair
        self.opts = opts
        self.deterministic = deterministic
        self.options = _blend_options(opts)
        self.euler_integration = EulerIntegration(opts)

    def forward(self, start_fs, Z_f, end_fs, Z_p, motion, start_index, middle_index, end_index):
        bs = start_fs.shape[0]
        dev = start_fs.device
        start_index, middle_index, end_index = (torch.as_tensor(v, device=dev) for v in (start_index, middle_index, end_index))
        if self.euler_pair:
            flow_f, flow_p = euler_integration_pair(motion.contiguous(), (middle_index.long() - start_index.long()).reshape(-1)[:bs],
                                                    (end_index.long() + 1 - middle_index.long()).reshape(-1)[:bs])   # :579-580
        else:
            flow_f = self.euler_integration(motion, middle_index.long() - start_index.long())                  # :579
            flow_p = self.euler_integration(-motion, end_index.long() + 1 - middle_index.long())               # :580
        alpha = (1.0 - (middle_index.float() - start_index.float()).float() / (
            end_index.float() - start_index.float() + 1.0).float()).reshape(bs).contiguous()                   # :585-586
        if not self.options["train_z"]:
            Z_f = Z_p = None
        else:
            Z_f, Z_p = Z_f.reshape(bs, 1, *start_fs.shape[2:]), Z_p.reshape(bs, 1, *start_fs.shape[2:])       # :590 / :639
        # (the keyword travels only when it is set: the default call is the one it always was)
        return splat_blend(start_fs, Z_f, flow_f, end_fs, Z_p, flow_p, alpha, clamp_z=self.options["clamp_z"],
                           subtract_max=self.options["subtract_max"], **({"deterministic": True} if self.deterministic else {}))
