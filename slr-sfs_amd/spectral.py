"""Spectral normalisation of the generator as the reference trains it (``--norm_G sync:spectral_batch``, the option of every training
script it ships): ``torch.nn.utils.spectral_norm`` around every 3x3, partial 3x3 and 1x1 convolution (models/layers/blocks.py:5-35) and
around the bias-free linear maps of the noise layers (models/layers/normalization.py:6-16).  The parameter is ``weight_orig``, the buffers
``weight_u`` / ``weight_v``; the effective weight is ``weight_orig / sigma``, ``sigma = u^T W v`` after one power iteration per forward in
training mode.

``SpectralGroup`` does this for every normalised tensor of a network in at most four launches, whatever their number (csrc/spectral.hip,
csrc/conv.hip): ``slr_spectral_sigma`` (power iteration, 1 / sigma, the copies of u and v the backward needs) and
``slr_conv_prep_scaled_multi`` (the forward and backward fragment buffers of every convolution, scaled by its 1 / sigma).
``spectral_weight_grad`` is the gradient to ``weight_orig`` (``slr_spectral_weight_grad``, two launches per tensor);
``spectral_weight_grad_multi`` is the same for a list of tensors in two launches, bit-equal per tensor
(``slr_spectral_weight_grad_multi``), and ``defer_weight_grad`` makes a network's group use it: one pair per forward's backward instead
of one per layer.  The loader takes a reference state dict
without folding, ``reference_state_dict`` writes one.  Nothing synchronises the host.  There is no fallback: CPU tensors raise.
"""
import ctypes
import weakref

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ._lib import call, check, lib

EPS = 1e-12                                              # torch.nn.utils.spectral_norm's default
MAX_DIM = 3072                                           # SLR_SPECTRAL_MAX_DIM of include/slr_splat.h: rows and cols of one matrix


def _require(name, t, shape=None, what="tensor"):
    """float32, ROCm, contiguous (and of ``shape``) -- before anything touches the device."""
    if not torch.is_tensor(t):
        raise TypeError(f"slr_sfs_amd.{name}: {what}: a tensor is required, got {type(t).__name__}")
    if not t.is_cuda:
        raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
    if t.dtype != torch.float32:
        raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {what} {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {what} is not contiguous")


def check_spectral(name, weight, weight_scale, spectral):
    """The checks of the operators' ``weight_scale`` / ``spectral`` arguments: a one-element scale, u [rows] and v [cols] of ``weight``
    viewed as [shape[0], -1], everything float32, contiguous and on ``weight``'s device."""
    if spectral is not None and weight_scale is None:
        raise ValueError(f"{name}: spectral=(u, v) goes with weight_scale (the 1 / sigma of the same forward)")
    if weight_scale is None:
        return
    _require(name, weight_scale, (1,), "weight_scale")
    if weight_scale.device != weight.device:
        raise ValueError(f"{name}: weight_scale lives on {weight_scale.device}, the weight on {weight.device}")
    if spectral is None:
        return
    if not isinstance(spectral, (tuple, list)) or len(spectral) != 2:
        raise TypeError(f"{name}: spectral is the pair (u, v)")
    rows = weight.shape[0]
    cols = weight.numel() // rows
    _require(name, spectral[0], (rows,), "spectral u")
    _require(name, spectral[1], (cols,), "spectral v")
    if spectral[0].device != weight.device or spectral[1].device != weight.device:
        raise ValueError(f"{name}: u and v live on the weight's device")


def spectral_weight_grad(dw, weight_orig, u, v, inv_sigma):
    """``(dw - <dw, W_eff> u v^T) * inv_sigma`` with ``W_eff = weight_orig * inv_sigma``: the gradient autograd returns for
    ``weight_orig`` through torch's spectral_norm when ``dw`` is the gradient at the effective weight (u, v: constants).  ``dw`` and
    ``weight_orig`` have one shape, [rows, ...]; u [rows], v [numel / rows], inv_sigma [1].  Two launches, the same bits every run."""
    _require("spectral_weight_grad", weight_orig, what="weight_orig")
    if weight_orig.dim() < 2 or weight_orig.numel() == 0:
        raise ValueError(f"spectral_weight_grad: weight_orig [rows, ...] with at least two dimensions required, got {tuple(weight_orig.shape)}")
    _require("spectral_weight_grad", dw, weight_orig.shape, "dw")
    check_spectral("spectral_weight_grad", weight_orig, inv_sigma, (u, v))
    if dw.device != weight_orig.device:
        raise ValueError("spectral_weight_grad: dw lives on the weight's device")
    return _weight_grad(dw, weight_orig, u, v, inv_sigma)


def _weight_grad(dw, weight_orig, u, v, inv_sigma):
    rows = weight_orig.shape[0]
    cols = weight_orig.numel() // rows
    out = torch.empty_like(dw)
    ws = torch.empty(int(lib().slr_spectral_grad_ws_bytes(rows, cols)), dtype=torch.uint8, device=dw.device)
    call("slr_spectral_weight_grad", dw.device, dw, weight_orig, u, v, inv_sigma, out, rows, cols, ws, ws.numel())
    return out


def _grad_plan(dws, weights, outs, offsets, slots, device):
    """The uploaded plan of ``slr_spectral_weight_grad_multi``: (device copy, the pinned host block it came from, n_work)."""
    n = len(dws)
    addr = [np.array([t.data_ptr() for t in ts], dtype=np.uint64) for ts in (dws, weights, outs)]
    rows = np.array([w.shape[0] for w in weights], dtype=np.int32)
    cols = np.array([w.numel() // w.shape[0] for w in weights], dtype=np.int32)
    u_off = np.array([o[0] for o in offsets], dtype=np.int64)
    v_off = np.array([o[1] for o in offsets], dtype=np.int64)
    slot = np.array(slots, dtype=np.int32)
    nbytes = int(lib().slr_spectral_grad_plan_bytes(n, rows.ctypes.data, cols.ctypes.data))
    if nbytes == 0:
        raise ValueError(f"spectral_weight_grad_multi: a matrix side outside 1 .. {MAX_DIM} (or an empty list)")
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)              # a fresh pinned block per plan: an earlier upload may be in flight
    check(lib().slr_spectral_grad_plan_fill(host.data_ptr(), nbytes, n, *(a.ctypes.data for a in addr), rows.ctypes.data, cols.ctypes.data,
                                            u_off.ctypes.data, v_off.ctypes.data, slot.ctypes.data), "slr_spectral_grad_plan_fill")
    dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dev.copy_(host, non_blocking=True)
    return dev, host, int(host.numpy()[12:16].view(np.uint32)[0])


def spectral_weight_grad_multi(dws, weights, saved_u, saved_v, offsets, inv_sigma, slots=None, inplace=False):
    """``spectral_weight_grad`` of every tensor of a list in TWO launches (``slr_spectral_weight_grad_multi``), each result bit-equal to
    the per-tensor call.  ``dws[i]`` is the gradient at the effective weight of ``weights[i]`` (= weight_orig, [rows, ...]); its u lies at
    ``saved_u[offsets[i][0]:]``, its v at ``saved_v[offsets[i][1]:]``, its 1 / sigma at ``inv_sigma[slots[i]]`` (default i): the arrays
    and offsets ``spectral_sigma`` returns, or any subset of its list.  Returns the list of gradients; ``inplace``: written over ``dws``.
    The plan is built and uploaded at every call; a network keeps it in a ``SpectralGroup`` (``defer_weight_grad``)."""
    dws, weights, offsets = list(dws), list(weights), [tuple(int(k) for k in o) for o in offsets]
    slots = list(range(len(weights))) if slots is None else [int(k) for k in slots]
    if not weights or not (len(dws) == len(offsets) == len(slots) == len(weights)):
        raise ValueError("spectral_weight_grad_multi: one dw, one (u_off, v_off) and one slot per weight, at least one weight")
    for name, t in (("saved_u", saved_u), ("saved_v", saved_v), ("inv_sigma", inv_sigma)):
        _require("spectral_weight_grad_multi", t, what=name)
        if t.dim() != 1:
            raise ValueError(f"spectral_weight_grad_multi: {name} is one-dimensional, got {tuple(t.shape)}")
    device = saved_u.device
    for w, dw, (u_off, v_off), k in zip(weights, dws, offsets, slots):
        _require("spectral_weight_grad_multi", w, what="weight_orig")
        if w.dim() < 2 or w.numel() == 0:
            raise ValueError(f"spectral_weight_grad_multi: weight_orig [rows, ...] with at least two dimensions required, got {tuple(w.shape)}")
        _require("spectral_weight_grad_multi", dw, w.shape, "dw")
        rows = w.shape[0]
        if not (0 <= u_off <= saved_u.numel() - rows and 0 <= v_off <= saved_v.numel() - w.numel() // rows and 0 <= k < inv_sigma.numel()):
            raise ValueError(f"spectral_weight_grad_multi: offsets ({u_off}, {v_off}) / slot {k} outside the saved arrays")
        if not (w.device == dw.device == device == saved_v.device == inv_sigma.device):
            raise ValueError("spectral_weight_grad_multi: every tensor lives on one device")
    outs = dws if inplace else [torch.empty_like(dw) for dw in dws]
    plan, host, n_work = _grad_plan(dws, weights, outs, offsets, slots, device)
    call("slr_spectral_weight_grad_multi", device, plan, len(weights), n_work, inv_sigma, saved_u, saved_v)
    return outs


class Normalised:
    """What an operator needs of its weight's normalisation in one forward: ``scale`` (1 / sigma), ``u`` and ``v`` (the constants of the
    backward; None: the plain gradient times scale), the prepared forward / backward fragment buffers (None: made by the single-tensor
    entries when they are needed) -- tensors or device addresses -- and ``keep``, whatever owns the memory behind the addresses.
    ``weight``: None, or under a group's deferred gradient the alias of ``weight_orig`` the layer computes with -- its gradient is the
    raw one at the effective weight, and the group turns every layer's into the gradient to ``weight_orig`` at once."""
    __slots__ = ("scale", "u", "v", "fwd", "bwd", "keep", "weight")

    def __init__(self, scale, u=None, v=None, fwd=None, bwd=None, keep=None, weight=None):
        self.scale, self.u, self.v, self.fwd, self.bwd, self.keep, self.weight = scale, u, v, fwd, bwd, keep, weight

    def __deepcopy__(self, memo):                        # one forward's state does not travel with a copied or saved module
        return None

    def __reduce__(self):
        return (type(None), ())

    def buffer(self, weight, backward):
        """The fp32 rung's fragment buffer of ``weight * scale`` (``backward``: of the backward-data convolution)."""
        buf = self.bwd if backward else self.fwd
        if buf is None:
            cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
            conv = "conv3x3" if k == 3 else "conv1x1"
            nbytes = getattr(lib(), f"slr_{conv}_weight_bytes")(*((cin, cout) if backward else (cout, cin)))
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=weight.device)
            call(f"slr_{conv}_f32_weights_scaled", weight.device, weight, self.scale, buf, cout, cin, int(backward))
            if backward:
                self.bwd = buf
            else:
                self.fwd = buf
        return buf

    def weight_grad(self, dw, weight):
        """The gradient to ``weight`` (= weight_orig) from the gradient ``dw`` at the effective weight."""
        if self.weight is not None:
            return dw                                    # (deferred: ``weight`` is the group's alias, the group's backward does the rest)
        if self.u is None:
            return dw * self.scale                       # (scale alone: the functional form with a tensor; a constant factor)
        return _weight_grad(dw, weight, self.u, self.v, self.scale)


class _EffectiveWeight(torch.autograd.Function):
    """weight_orig * inv_sigma of a noise linear; the backward is ``slr_spectral_weight_grad``."""

    @staticmethod
    def forward(ctx, weight_orig, sn):
        ctx.sn = sn
        ctx.save_for_backward(weight_orig)
        return weight_orig * sn.scale

    @staticmethod
    def backward(ctx, g):
        (weight_orig,) = ctx.saved_tensors
        g = g.contiguous()
        _require("SpectralLinear", g, weight_orig.shape, "gradient")
        return ctx.sn.weight_grad(g, weight_orig), None


def _fresh_uv(rows, cols):
    """u and v as torch.nn.utils.spectral_norm makes them: normalised normal vectors."""
    return F.normalize(torch.randn(rows), dim=0, eps=EPS), F.normalize(torch.randn(cols), dim=0, eps=EPS)


def make_spectral(module, name="weight"):
    """Turns ``module.weight`` into the parametrisation of torch's spectral_norm: the parameter ``weight_orig`` (the same values), the
    buffers ``weight_u`` and ``weight_v``; no ``weight`` parameter is left."""
    w = module._parameters.pop(name)
    module.register_parameter(name + "_orig", nn.Parameter(w.detach().clone(), requires_grad=True))
    u, v = _fresh_uv(w.shape[0], w.numel() // w.shape[0])
    module.register_buffer(name + "_u", u)
    module.register_buffer(name + "_v", v)
    module.spectral_leaf = True
    object.__setattr__(module, "_sn", None)
    return module


class SpectralLinear(nn.Module):
    """``spectral_norm(nn.Linear(cin, cout, bias=False))`` of the noise layers: x -> x (weight_orig / sigma)^T.  The product stays in
    torch ([N, 20] x [20, C] is not tensor-sized)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(nn.Linear(cin, cout, bias=False).weight.detach())
        make_spectral(self)

    def forward(self, x):
        w, sn = taken(self)
        return F.linear(x, _EffectiveWeight.apply(w, sn))


class UnusedSpectralConv(nn.Module):
    """The ``conv_b`` that ResNet_Block_Pconv2 constructs in every block (blocks.py:192-195) and never calls where the block neither
    resamples nor changes its width (:243-247): its ``weight_orig`` / ``weight_u`` / ``weight_v`` are in every reference state dict.
    Held as buffers so that a checkpoint loads strictly and is written back whole; nothing computes with them."""

    def __init__(self, cin, cout):
        super().__init__()
        self.register_buffer("weight_orig", torch.randn(cout, cin, 1, 1) * (1.0 / cin) ** 0.5)
        u, v = _fresh_uv(cout, cin)
        self.register_buffer("weight_u", u)
        self.register_buffer("weight_v", v)


def leaves_of(modules):
    """Every normalised layer under ``modules``, each once, in module order."""
    seen, out = set(), []
    for root in modules:
        for m in root.modules():
            if getattr(m, "spectral_leaf", False) and id(m) not in seen:
                seen.add(id(m))
                out.append(m)
    return out


def take(leaf):
    """The ``Normalised`` of ``leaf`` for this forward, handed out by the group that ran last; a layer used on its own runs a group of
    its own.  Every forward takes it once: the next one iterates again."""
    sn = leaf._sn
    if sn is None:
        group_of(leaf).run()
        sn = leaf._sn
    object.__setattr__(leaf, "_sn", None)
    return sn


def taken(leaf):
    """(the tensor the layer computes with, ``take(leaf)``): ``weight_orig``, or its alias under a deferred gradient."""
    sn = take(leaf)
    return (leaf.weight_orig if sn.weight is None else sn.weight), sn


def defer_weight_grad(module, on=True):
    """Opt-in: the group of ``module`` (a network, or whatever runs its own group) computes the gradients to every ``weight_orig`` of one
    forward in ONE ``slr_spectral_weight_grad_multi`` (two launches) when that forward's backward is complete, instead of two launches
    per layer.  The same bits as without it.  Off: exactly the per-layer path."""
    object.__setattr__(module, "_sn_defer", bool(on))     # (kept on the module: a copied module makes a new group and stays as it was)
    return module


class _DeferredGrad(torch.autograd.Function):
    """The hook at the end of one forward's backward: the inputs are the ``weight_orig`` of a group's leaves, the outputs aliases of
    them that the layers compute with.  Autograd calls the backward once every consumer of the aliases has run, with the raw gradient at
    each effective weight (None: a leaf this forward did not use, which gets no gradient)."""

    @staticmethod
    def forward(ctx, group, state, *weights):
        ctx.group, ctx.state = group, state
        ctx.set_materialize_grads(False)                 # (an alias nothing consumed arrives as None, not as zeros)
        ctx.save_for_backward(*weights)
        return tuple(w.detach() for w in weights)

    @staticmethod
    def backward(ctx, *gs):
        weights = ctx.saved_tensors
        used = tuple(i for i, g in enumerate(gs) if g is not None and ctx.needs_input_grad[2 + i])
        out = [None] * len(gs)
        if used:
            dws = []
            for i in used:
                g = gs[i].contiguous()
                _require("SpectralGroup", g, weights[i].shape, "gradient at the effective weight")
                dws.append(g)
            # In place over the gradients autograd handed in, against its general rule: an alias is an output of this node with exactly
            # one consumer (a layer takes its Normalised once per run), so the incoming tensor is that layer's fresh dW (or autograd's
            # own sum), which nothing else holds -- the aliases are internal: no hook, no retain_grad, no create_graph reaches them.
            ctx.group._weight_grads(ctx.state, used, dws, [weights[i] for i in used])
            for i, g in zip(used, dws):
                out[i] = g
        return (None, None, *out)


def group_of(module):
    """The ``SpectralGroup`` of everything normalised under ``module``, made at first use."""
    g = module.__dict__.get("_sn_group")
    if g is None:
        g = SpectralGroup([module])
        object.__setattr__(module, "_sn_group", g)
    return g


def begin(module, force=False):
    """At the start of ``module.forward``: run its group unless an enclosing forward already did (``force``: a network always does)."""
    g = group_of(module)
    if g.leaves and (force or any(m._sn is None for m in g.leaves)):        # (a forward that raised midway leaves some taken: all are made again)
        g.run()


def _sigma_plan(triples, device):
    """The uploaded plan of ``slr_spectral_sigma`` for (weight_orig, u, v) triples: (device copy, the pinned host block it came from, n_work)."""
    n = len(triples)
    addr = np.ascontiguousarray(np.array([[t.data_ptr() for t in tr] for tr in triples], dtype=np.uint64).T)
    rows = np.array([tr[0].shape[0] for tr in triples], dtype=np.int32)
    cols = np.array([tr[0].numel() // tr[0].shape[0] for tr in triples], dtype=np.int32)
    nbytes = int(lib().slr_spectral_plan_bytes(n, rows.ctypes.data, cols.ctypes.data))
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)              # a fresh pinned block per plan: an earlier upload may be in flight
    check(lib().slr_spectral_plan_fill(host.data_ptr(), nbytes, n, *(addr[k].ctypes.data for k in range(3)), rows.ctypes.data,
                                       cols.ctypes.data), "slr_spectral_plan_fill")
    dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dev.copy_(host, non_blocking=True)
    return dev, host, int(host.numpy()[12:16].view(np.uint32)[0])


def spectral_sigma(weights, us, vs, training=True):
    """The functional form of the group's first launch: for weight_orig tensors ``weights`` [rows, ...] with their ``us`` [rows] and ``vs``
    [cols], ONE ``slr_spectral_sigma`` -- training: one power iteration that moves every u and v in place; eval: they are read only.
    Returns (inv_sigma [n], saved_u, saved_v, offsets): the saved arrays hold the u and v this call used, tensor i's at
    offsets[i] = (u_off, v_off).  The plan is built and uploaded at every call; a network keeps it in a ``SpectralGroup``."""
    weights, us, vs = list(weights), list(us), list(vs)
    if not weights or len(us) != len(weights) or len(vs) != len(weights):
        raise ValueError("spectral_sigma: one u and one v per weight, at least one weight")
    for w, u, v in zip(weights, us, vs):
        _require("spectral_sigma", w, what="weight_orig")
        if w.dim() < 2 or w.numel() == 0:
            raise ValueError(f"spectral_sigma: weight_orig [rows, ...] with at least two dimensions required, got {tuple(w.shape)}")
        _require("spectral_sigma", u, (w.shape[0],), "u")
        _require("spectral_sigma", v, (w.numel() // w.shape[0],), "v")
        if not (w.device == u.device == v.device == weights[0].device):
            raise ValueError("spectral_sigma: the tensors of a list share one device")
    device = weights[0].device
    plan, host, n_work = _sigma_plan(list(zip(weights, us, vs)), device)
    offsets, u_off, v_off = [], 0, 0
    for u, v in zip(us, vs):
        offsets.append((u_off, v_off))
        u_off, v_off = u_off + u.numel(), v_off + v.numel()
    inv_sigma = torch.empty(len(weights), dtype=torch.float32, device=device)
    saved_u = torch.empty(u_off, dtype=torch.float32, device=device)
    saved_v = torch.empty(v_off, dtype=torch.float32, device=device)
    call("slr_spectral_sigma", device, plan, len(weights), n_work, inv_sigma, saved_u, saved_v, int(bool(training)))
    if training:
        torch.autograd.graph.increment_version(us + vs)
    return inv_sigma, saved_u, saved_v, offsets


def prepare_scaled(weights, scales, slots=None):
    """The functional form of the group's second launch: the forward and backward fragment buffers of every convolution weight
    [Cout,Cin,k,k] (k 3 or 1) of ``weights``, weight i multiplied by ``scales[slots[i]]`` (default i), in ONE
    ``slr_conv_prep_scaled_multi``.  Returns [(forward buffer, backward buffer)] as byte tensors (views of one block)."""
    weights = list(weights)
    slots = list(range(len(weights))) if slots is None else [int(k) for k in slots]
    _require("prepare_scaled", scales, what="scales")
    for w in weights:
        _require("prepare_scaled", w, what="weight")
        if w.dim() != 4 or w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3):
            raise ValueError(f"prepare_scaled: weight [Cout,Cin,k,k] with k 3 or 1 required, got {tuple(w.shape)}")
    if len(slots) != len(weights) or not weights or any(k < 0 or k >= scales.numel() for k in slots):
        raise ValueError("prepare_scaled: one slot inside scales per weight, at least one weight")
    bufs = _BufferSet(weights, slots, weights[0].device)
    call("slr_conv_prep_scaled_multi", weights[0].device, bufs.plan, bufs.n, bufs.n_work, scales)
    views = [bufs.block[o:o + n] for o, n in zip(bufs.offs, bufs.sizes)]
    return [(views[2 * i], views[2 * i + 1]) for i in range(len(weights))]


class _BufferSet:
    """The fragment buffers of every convolution of a group, forward and backward, in one block, with the uploaded plan of
    ``slr_conv_prep_scaled_multi`` that fills them.  One per forward whose backward is still to come."""

    def __init__(self, weights, slots, device):
        n = 2 * len(weights)
        cout = np.array([w.shape[0] for w in weights for _ in (0, 1)], dtype=np.int32)
        cin = np.array([w.shape[1] for w in weights for _ in (0, 1)], dtype=np.int32)
        taps = np.array([w.shape[2] ** 2 for w in weights for _ in (0, 1)], dtype=np.int32)
        backward = np.array([b for _ in weights for b in (0, 1)], dtype=np.int32)
        slot = np.array([k for k in slots for _ in (0, 1)], dtype=np.int32)
        sizes = []
        for k in range(n):
            nbytes = (lib().slr_conv3x3_weight_bytes if taps[k] == 9 else lib().slr_conv1x1_weight_bytes)
            co, ci = (int(cin[k]), int(cout[k])) if backward[k] else (int(cout[k]), int(cin[k]))
            sizes.append((int(nbytes(co, ci)) + 255) & ~255)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.block = torch.empty(int(offs[-1]), dtype=torch.uint8, device=device)
        base = self.block.data_ptr()
        self.addr = [base + int(o) for o in offs[:-1]]                          # [2 i] forward, [2 i + 1] backward of convolution i
        w = np.array([t.data_ptr() for t in weights for _ in (0, 1)], dtype=np.uint64)
        self.sizes, self.offs = sizes, [int(o) for o in offs[:-1]]
        wf = np.array(self.addr, dtype=np.uint64)
        args = [a.ctypes.data for a in (cout, cin, taps, backward)]
        nbytes = int(lib().slr_conv_prep_plan_bytes(n, *args))
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        check(lib().slr_conv_prep_plan_fill(host.data_ptr(), nbytes, n, w.ctypes.data, wf.ctypes.data, slot.ctypes.data, *args),
              "slr_conv_prep_plan_fill")
        self.n, self.n_work = n, int(host.numpy()[12:16].view(np.uint32)[0])
        self.plan = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.plan.copy_(host, non_blocking=True)
        self.host = host                                                       # (the upload may be in flight)


class _State:
    """One forward's normalisation: inv_sigma [n], the saved u and v, the buffer set.  The autograd nodes of that forward keep it; when
    the last one goes, the buffer set returns to its group."""

    def __init__(self, group, key, n, total_u, total_v, device, bufs):
        self.group, self.key, self.bufs = weakref.ref(group), key, bufs
        self.inv_sigma = torch.empty(n, dtype=torch.float32, device=device)
        self.saved_u = torch.empty(total_u, dtype=torch.float32, device=device)
        self.saved_v = torch.empty(total_v, dtype=torch.float32, device=device)

    def __del__(self):
        g = self.group()
        if g is not None and self.bufs is not None and g._key == self.key:
            g._free.append(self.bufs)


class SpectralGroup:
    """Every spectrally normalised tensor under ``modules`` (layers made by ``make_spectral``: ``weight_orig``, ``weight_u``,
    ``weight_v``).  ``run()``: one ``slr_spectral_sigma`` over all of them -- in ``train()`` mode one power iteration that moves u and v
    in place, as the reference's forward pre-hook does; in ``eval()`` mode u and v are read only and the result is kept while no tensor's
    address or version changes -- then one ``slr_conv_prep_scaled_multi`` for the forward and backward buffers of every convolution.
    Each run has its own inv_sigma, saved u / v and buffers: a network called twice before its backward iterates twice, and each
    call's backward uses the values of its own forward.  The plans live in device memory and are uploaded again only when an address
    changes."""

    def __deepcopy__(self, memo):                        # plans and buffers belong to these tensors' addresses: a copied or saved module
        return None                                      # makes its own group at its next forward (group_of)

    def __reduce__(self):
        return (type(None), ())

    def __init__(self, modules):
        self.modules = list(modules)
        self.leaves = leaves_of(self.modules)
        self.convs = [m for m in self.leaves if m.weight_orig.dim() == 4]
        self._key, self._plan, self._free, self._eval = None, None, [], None
        self._grad_plans = {}                            # the plans of the list-wide gradient (deferred mode) by address tuple
        self._layout()

    @property
    def deferred(self):
        """``defer_weight_grad`` of the module the group was made for."""
        return bool(self.modules[0].__dict__.get("_sn_defer", False))

    def _layout(self):
        u_off = v_off = 0
        self.offsets = []
        for i, m in enumerate(self.leaves):
            rows = m.weight_orig.shape[0]
            cols = m.weight_orig.numel() // rows
            self.offsets.append((u_off, v_off, rows, cols))
            u_off += rows
            v_off += cols
        self.total_u, self.total_v = u_off, v_off

    def tensors(self):
        return [t for m in self.leaves for t in (m.weight_orig, m.weight_u, m.weight_v)]

    def _check(self):
        if not self.leaves:
            raise ValueError("SpectralGroup: no spectrally normalised layer under these modules")
        device = self.leaves[0].weight_orig.device
        for m, (_, _, rows, cols) in zip(self.leaves, self.offsets):
            _require("SpectralGroup", m.weight_orig, what="weight_orig")
            _require("SpectralGroup", m.weight_u, (rows,), "weight_u")
            _require("SpectralGroup", m.weight_v, (cols,), "weight_v")
            if any(t.device != device for t in (m.weight_orig, m.weight_u, m.weight_v)):
                raise ValueError("SpectralGroup: the tensors of a group share one device")
        return device

    def _sigma_plan(self, device):
        return _sigma_plan([(m.weight_orig, m.weight_u, m.weight_v) for m in self.leaves], device)

    def run(self):
        return self._run(torch.is_grad_enabled())

    @torch.no_grad()
    def _run(self, grad):
        device = self._check()
        tensors = self.tensors()
        key = tuple(t.data_ptr() for t in tensors)
        if key != self._key:                                                   # an address changed: new plans, new buffers
            self._key, self._free, self._eval = key, [], None
            self._plan = self._sigma_plan(device)
            for i, m in enumerate(self.leaves):
                object.__setattr__(m, "_sn_index", i)
        training = self.modules[0].training
        state = None
        if not training:
            versions = tuple(t._version for t in tensors)
            if self._eval is not None and self._eval[0] == versions:
                state = self._eval[1]
        if state is None:
            bufs = None
            if self.convs:
                bufs = self._free.pop() if self._free else _BufferSet([m.weight_orig for m in self.convs],
                                                                        [m._sn_index for m in self.convs], device)
            state = _State(self, key, len(self.leaves), self.total_u, self.total_v, device, bufs)
            call("slr_spectral_sigma", device, self._plan[0], len(self.leaves), self._plan[2], state.inv_sigma, state.saved_u, state.saved_v, int(training))
            if training:                                                       # u and v moved: whatever is keyed on their versions sees it
                torch.autograd.graph.increment_version([t for m in self.leaves for t in (m.weight_u, m.weight_v)])
            if bufs is not None:
                call("slr_conv_prep_scaled_multi", device, bufs.plan, bufs.n, bufs.n_work, state.inv_sigma)
            self._eval = None if training else (tuple(t._version for t in tensors), state)
        self._hand_out(state, grad)
        return state

    def _hand_out(self, state, grad=False):
        s0, u0, v0 = state.inv_sigma.data_ptr(), state.saved_u.data_ptr(), state.saved_v.data_ptr()
        P = ctypes.c_void_p
        k = 0
        alias = [None] * len(self.leaves)
        if self.deferred and grad and any(m.weight_orig.requires_grad for m in self.leaves):
            with torch.enable_grad():
                alias = _DeferredGrad.apply(self, state, *(m.weight_orig for m in self.leaves))
        for i, (m, (u_off, v_off, _, _)) in enumerate(zip(self.leaves, self.offsets)):
            if m.weight_orig.dim() == 4:
                sn = Normalised(P(s0 + 4 * i), P(u0 + 4 * u_off), P(v0 + 4 * v_off), P(state.bufs.addr[2 * k]), P(state.bufs.addr[2 * k + 1]), state,
                                alias[i])
                k += 1
            else:                                                              # a linear: torch multiplies by the scale
                sn = Normalised(state.inv_sigma[i:i + 1], P(u0 + 4 * u_off), P(v0 + 4 * v_off), keep=state, weight=alias[i])
            object.__setattr__(m, "_sn", sn)

    GRAD_PLANS_MAX = 8                                   # (a forward used twice before its backward, a few address patterns of the allocator)

    def _weight_grads(self, state, used, dws, weights):
        """In place over ``dws`` (leaf ``used[k]``'s raw gradient): the gradients to ``weight_orig`` with ``state``'s u, v and 1 / sigma,
        in one ``slr_spectral_weight_grad_multi``.  A plan is uploaded only for a set of leaves and addresses not seen before."""
        device = state.inv_sigma.device
        key = (used, tuple(t.data_ptr() for t in dws), tuple(t.data_ptr() for t in weights))
        plan = self._grad_plans.pop(key, None)
        if plan is None:
            while len(self._grad_plans) >= self.GRAD_PLANS_MAX:
                self._grad_plans.pop(next(iter(self._grad_plans)))            # (the oldest: its memory returns stream-ordered)
            plan = _grad_plan(dws, weights, dws, [self.offsets[i][:2] for i in used], list(used), device)
        self._grad_plans[key] = plan                                           # (most recently used last)
        call("slr_spectral_weight_grad_multi", device, plan[0], len(used), plan[2], state.inv_sigma, state.saved_u, state.saved_v)


# --------------------------------------------------------------------------- checkpoints of the reference, unfolded

def _pairs(net):
    """(module, reference key) of every layer of a trainable network with spectral=True, in the reference's key scheme (the one
    ``nets.load_reference_state_dict`` walks): ('conv' | 'linear' | 'bn' | 'unused', module, key)."""
    from . import nets
    out = []
    for i, blk in enumerate(net.blocks):
        if isinstance(blk, nets.PconvResBlock):
            b = f"eblocks.{i}."
            names = (("bn_noise1", "pbn"), ("bn_noise2", "pbn"), "conv_aa", "conv_ab", "conv_b")
        else:
            b = ("eblocks" if isinstance(net, nets.BGDecoder) else "gblocks") + f".{i}."
            names = (("ch_a.0", "bn"), ("ch_a.3", "bn"), "ch_a.2", "ch_a.5", "ch_b.0")
        for bn, (layer, stats) in zip((blk.bn1, blk.bn2), names[:2]):
            out.append(("bn", bn, b + layer + "." + stats))
            out.append(("linear", bn.gain, b + layer + ".gain"))
            out.append(("linear", bn.bias, b + layer + ".bias"))
        for conv, name in zip((blk.conv_aa, blk.conv_ab, blk.conv_b), names[2:]):
            if conv is not None:
                out.append(("conv", conv, b + name))
        if getattr(blk, "conv_b_unused", None) is not None:           # (ResNet_Block_Pconv2 only: ResNet_Block registers no unused ch_b)
            out.append(("unused", blk.conv_b_unused, b + "conv_b"))
    return out


def _entries(net):
    """reference key (without prefix) -> tensor of ``net``."""
    if not getattr(net, "spectral", False):
        raise ValueError("a network built with spectral=True is required (nets.load_reference_state_dict fills the folded ones)")
    out = {}
    for kind, m, key in _pairs(net):
        if kind == "bn":
            out[key + ".stored_mean"], out[key + ".stored_var"] = m.stored_mean, m.stored_var
            out[key + ".accumulation_counter"] = m.accumulation_counter
            continue
        out[key + ".weight_orig"], out[key + ".weight_u"], out[key + ".weight_v"] = m.weight_orig, m.weight_u, m.weight_v
        if kind == "conv" and m.bias is not None:
            out[key + ".bias"] = m.bias
    return out


@torch.no_grad()
def load_spectral_state_dict(net, sd, prefix):
    """Fills a ``spectral=True`` network from a reference state dict WITHOUT folding: ``weight_orig``, ``weight_u`` and ``weight_v`` of
    every convolution and noise linear, the biases, the batch-norm statistics with the reference's ``accumulation_counter``
    (normalization.py:167, 266: carried, it only counts under accumulate_standing) and the ``conv_b`` tensors of the partial-convolution
    blocks that never call it (``UnusedSpectralConv``).  Strict in both directions: every key under ``prefix`` is
    consumed and every tensor of the network is found, with its shape; otherwise KeyError / ValueError and the network is untouched."""
    mine = _entries(net)
    theirs = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    missing = sorted(set(mine) - set(theirs))
    extra = sorted(set(theirs) - set(mine))
    if missing or extra:
        raise KeyError(f"load_spectral_state_dict({prefix!r}): missing {missing[:4]}{'...' if len(missing) > 4 else ''} ({len(missing)}), "
                       f"unexpected {extra[:4]}{'...' if len(extra) > 4 else ''} ({len(extra)})")
    for k, t in mine.items():
        if tuple(theirs[k].shape) != tuple(t.shape):
            raise ValueError(f"load_spectral_state_dict: {prefix + k}: shape {tuple(theirs[k].shape)}, expected {tuple(t.shape)}")
    for k, t in mine.items():
        t.copy_(theirs[k])                               # (in place: the addresses, and with them the plans, stay)
    return net


def reference_state_dict(net, prefix=""):
    """The reference's keys and tensors (detached clones) of a ``spectral=True`` network: what ``load_spectral_state_dict`` reads, and
    the complete key set of the reference's module under ``--norm_G sync:spectral_batch`` (its strict ``load_state_dict`` takes it)."""
    return {prefix + k: t.detach().clone() for k, t in _entries(net).items()}
