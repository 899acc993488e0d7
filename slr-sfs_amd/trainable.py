"""The decoder block whose weights learn.  First its 3x3 convolutions: the plain and the partial 3x3 / stride 1 / pad 1 convolution of the
reference's decoder (models/layers/blocks.py:66-87, models/layers/partialconv2d.py:41-81) as differentiable operators in input, weight and
bias.

Forward: the package's fp32 rung (``nets.fp32_kernels(winograd=False)``: fp32 operands, products and accumulation on the matrix cores, the
arithmetic of ``nn.Conv2d``).  Backward: the gradient to the input is the same forward kernel with flipped, transposed weights; weight and
bias gradients come from ``slr_conv3x3_weight_grad`` / ``slr_conv_grad_scale_bias`` (csrc/conv_grad.hip).  Only what ``needs_input_grad``
asks for is computed.  Nothing synchronises; every result has the same bits from run to run.  There is no fallback: CPU tensors raise, a
missing library raises.

Then the rest of ResNet_Block_Pconv2 in training mode (blocks.py:173-248; csrc/block_grad.hip): the noise-conditioned
(partial) batch-norm with batch statistics + ReLU + mask (``bn_relu_mask_train``, ``TrainableNoiseBN``), the 1x1 skip convolution
(``conv1x1``), differentiable ``avgpool_down`` / ``upsample_up``, and the block itself (``TrainablePconvResBlock``).

Then the generator's networks (the batch-norm's nonzero mask kind in csrc/block_grad.hip, csrc/decoder_grad.hip): the
decoder's first block, whose mask is (x != 0) per element (architectures.py:369) -- ``bn_relu_nonzero_train``,
``partial_conv_factors_counts``, ``partial_conv3x3_counts``,
``TrainablePconvInputBlock`` -- the plain ``TrainableResBlock`` (ResNet_Block, blocks.py:47-87) and the nets made of the two:
``TrainableDecoderPconv2``, ``TrainableEncoderWithZ``, ``TrainableEncoder``, ``TrainableBGDecoder``.

Spectral normalisation as the reference trains with it (--norm_G sync:spectral_batch; DESIGN 3.14, spectral.py, csrc/spectral.hip): the
operators take ``weight_scale`` (the 1 / sigma of this forward, a device scalar folded into the weight preparation) and ``spectral`` (the
saved u and v: the weight gradient is then the one to ``weight_orig``); the layers, blocks and networks take ``spectral=True``.

Not here: BN + ReLU fused into the backward convolution's prologue.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import nets
from . import spectral as _spectral
from ._lib import call, lib, require_device

GRAD_X_B8, GRAD_G_B8 = 1, 2              # include/slr_splat.h: SLR_GRAD_X_B8 / SLR_GRAD_G_B8


def _check_tensors(name, tensors):
    """What every operator checks first of its tensors (None: an absent optional one): types, device, dtype, in this order."""
    for t in tensors:
        if t is not None and not torch.is_tensor(t):
            raise TypeError(f"slr_sfs_amd.{name}: tensors required, got {type(t).__name__}")
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype}")


def _check_contiguous(name, tensors, labels=None):
    """... and last, after their shapes: contiguity and one device."""
    for i, t in enumerate(tensors):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: {labels[i] if labels else 'a tensor'} is not contiguous")
    require_device(*tensors)


def _check(name, x, weight, bias, mask=None, in_b8=False, out_b8=False, k=3, residual=None):
    """Types, device, dtype, shapes and layouts -- before anything touches the device."""
    tensors = (x, weight, bias, mask, residual)
    _check_tensors(name, tensors)
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{name}: input [N,Cin,H,W] with N, Cin, H, W >= 1 required, got {tuple(x.shape)}")
    N, cin, H, W = x.shape
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (cin, k, k) or weight.shape[0] < 1:
        raise ValueError(f"{name}: weight {tuple(weight.shape)}, expected [Cout,{cin},{k},{k}]")
    cout = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"{name}: bias {tuple(bias.shape)}, expected ({cout},)")
    if mask is not None and tuple(mask.shape) != (N, 1, H, W):
        raise ValueError(f"{name}: mask {tuple(mask.shape)}, expected {(N, 1, H, W)}")
    if in_b8 and cin % 8:
        raise ValueError(f"{name}: a channel-blocked input needs Cin % 8 == 0, got {cin}")
    if out_b8 and cout % 8:
        raise ValueError(f"{name}: a channel-blocked output needs Cout % 8 == 0, got {cout}")
    if residual is not None and tuple(residual.shape) != (N, cout, H, W):
        raise ValueError(f"{name}: residual {tuple(residual.shape)}, expected {(N, cout, H, W)}")
    _check_contiguous(name, tensors, ("input", "weight", "bias", "mask", "residual"))


class _Prepared(nets.Conv):
    """``nets.Conv``'s weight preparation and its cache (keyed on the weight's data pointer, version and device) around a weight tensor
    somebody else owns."""

    def __init__(self, weight):
        nn.Module.__init__(self)
        object.__setattr__(self, "weight", weight)      # (not registered: the tensor stays its owner's)
        object.__setattr__(self, "bias", None)
        self.cin, self.k, self.pad = weight.shape[1], weight.shape[2], weight.shape[2] // 2


def _owner_of(weight, owner):
    """The object whose cache holds ``weight``'s prepared buffers: the module, or for the functional form one kept on the tensor itself."""
    if owner is not None:
        return owner
    p = getattr(weight, "_slr_prepared", None)
    if p is None:
        p = weight._slr_prepared = _Prepared(weight)
    return p


def _forward_weights(weight, owner):
    """The fp32 rung's fragment buffer of ``weight``, made again when the weight's version changes (an optimizer step)."""
    with nets.fp32_kernels(winograd=False):
        buf, _, _, arith = _owner_of(weight, owner)._split_weights()
    return buf, arith


def _backward_weights(weight, owner):
    """The same for the backward-data convolution: ``weight.flip(2, 3).transpose(0, 1)`` (as losses.VGG19Features.backward_conv)."""
    def make():
        with torch.no_grad():
            return _Prepared(weight.detach().flip(2, 3).transpose(0, 1).contiguous())
    bconv = nets._cached(_owner_of(weight, owner), "_bwd_conv", make, weight)
    return _forward_weights(bconv.weight, bconv)


def _normalised(name, weight, weight_scale, spectral, sn):
    """The operators' ``weight_scale`` / ``spectral`` arguments, checked, as one ``spectral.Normalised`` (None: no normalisation); ``sn``:
    the one a ``SpectralGroup`` handed to the layer."""
    if sn is not None:
        return sn
    _spectral.check_spectral(name, weight, weight_scale, spectral)
    if weight_scale is None:
        return None
    u, v = spectral if spectral is not None else (None, None)
    return _spectral.Normalised(weight_scale.detach(), None if u is None else u.detach(), None if v is None else v.detach())


def _weights_of(weight, owner, sn, backward=False):
    """(buffer, rung flag) of the forward or the backward-data convolution: today's cached preparation, or with a normalisation the
    buffer of ``weight * scale`` (always the fp32 rung)."""
    if sn is None:
        return _backward_weights(weight, owner) if backward else _forward_weights(weight, owner)
    return sn.buffer(weight, backward), nets.CONV_F32


def _conv(x, buf, arith, bias, cout, layout, residual=None, k=3):
    """The k x k forward kernel (k = 3 or 1; the 1x1 entry point has no residual)."""
    N, cin, H, W = x.shape
    out = x.new_empty(N, cout, H, W)
    if k == 1:
        call("slr_conv1x1_forward", x.device, x, buf, bias, out, N, cin, cout, H, W, 1.0, 1.0, layout | arith)
    else:
        call("slr_conv3x3_forward", x.device, x, buf, bias, residual, out, N, cin, cout, H, W, 1.0, 1.0, None, None, layout | arith)
    return out


def _conv_backward_data(g, weight, owner, sn, in_b8, out_b8, k=3):
    """The gradient to a convolution's input: the forward kernel with the flipped, transposed weight, the layouts swapped."""
    buf, arith = _weights_of(weight, owner, sn, True)
    return _conv(g, buf, arith, None, weight.shape[1], (nets.IN_B8 if out_b8 else 0) | (nets.OUT_B8 if in_b8 else 0), k=k)


def _weight_grad(x, g, cout, want_bias, layout, splits=0, k=3):
    """(dW, db or None).  The 3x3 entry point sums the bias gradient itself; the 1x1 one has no such output: ``_scale_bias`` does it."""
    N, cin, H, W = x.shape
    dw = x.new_empty(cout, cin, k, k)
    ws_bytes = lib().slr_conv1x1_grad_ws_bytes if k == 1 else lib().slr_conv3x3_grad_ws_bytes
    ws = torch.empty(int(ws_bytes(N, cin, cout, H, W, splits)), dtype=torch.uint8, device=x.device)
    if k == 1:
        call("slr_conv1x1_weight_grad", x.device, x, g, dw, N, cin, cout, H, W, splits, layout, ws, ws.numel())
        return dw, (_scale_bias(g, None, None, False, True, layout & GRAD_G_B8)[1] if want_bias else None)
    db = x.new_empty(cout) if want_bias else None
    call("slr_conv3x3_weight_grad", x.device, x, g, dw, db, N, cin, cout, H, W, splits, layout, ws, ws.numel())
    return dw, db


def _scale_bias(g, r, um, want_gr, want_bias, layout=0):
    N, C, H, W = g.shape
    gr = torch.empty_like(g) if want_gr else None
    db = g.new_empty(C) if want_bias else None
    ws = None
    if want_bias:
        ws = torch.empty(int(lib().slr_conv3x3_grad_ws_bytes(N, 0, C, H, W, 0)), dtype=torch.uint8, device=g.device)
    call("slr_conv_grad_scale_bias", g.device, g, r, um, gr, db, N, C, H, W, layout, ws, 0 if ws is None else ws.numel())
    return gr, db


class _Conv(torch.autograd.Function):
    """The plain convolution, 3x3 or 1x1 by the weight's shape."""

    @staticmethod
    def forward(ctx, x, weight, bias, in_b8, out_b8, owner, residual=None, sn=None):
        k = weight.shape[2]
        if k == 1 and residual is not None:
            raise ValueError("conv1x1: no residual (slr_conv1x1_forward has no such argument)")
        buf, arith = _weights_of(weight, owner, sn)
        layout = (nets.IN_B8 if in_b8 else 0) | (nets.OUT_B8 if out_b8 else 0) | (nets.RES_B8 if out_b8 and residual is not None else 0)
        out = _conv(x, buf, arith, bias, weight.shape[0], layout, residual, k)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (in_b8, out_b8, owner, bias is not None)
        ctx.sn = sn
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        in_b8, out_b8, owner, has_bias = ctx.cfg
        g = g.contiguous()
        require_device(g)
        cout, k = weight.shape[0], weight.shape[2]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = None
        if need_x:
            gx = _conv_backward_data(g, weight, owner, ctx.sn, in_b8, out_b8, k)
        glayout = GRAD_G_B8 if out_b8 else 0
        if need_w:
            gw, gb = _weight_grad(x, g, cout, need_b, (GRAD_X_B8 if in_b8 else 0) | glayout, k=k)
            if ctx.sn is not None:
                gw = ctx.sn.weight_grad(gw, weight)
        elif need_b:
            _, gb = _scale_bias(g, None, None, False, True, glayout)
        return gx, gw, gb, None, None, None, (g if ctx.needs_input_grad[6] else None), None    # (out = ... + residual)


def conv3x3(x, weight, bias=None, *, in_b8=False, out_b8=False, residual=None, weight_scale=None, spectral=None, _owner=None, _sn=None):
    """conv2d(x, weight, bias, stride 1, padding 1) for a 3x3 ``weight`` [Cout,Cin,3,3], differentiable in x, weight and bias.

    in_b8 / out_b8: x / the result (and with them their gradients) are channel-blocked, [N,C/8,H,W,8] in memory under the logical shape
    [N,C,H,W] -- the package's activation layout (nets._b8); C % 8 == 0 then.  ``residual`` [N,Cout,H,W] (in the result's layout) is
    added in the kernel's epilogue (the x_a + x_b of ResNet_Block, blocks.py:87) and receives the result's gradient.

    weight_scale: a one-element device tensor; the convolution runs with ``weight * weight_scale`` (the factor is folded into the weight
    preparation: no pass of its own) and the weight gradient is the one to ``weight``, the factor a constant.  spectral=(u, v), with
    ``weight_scale`` = 1 / sigma of the same forward: ``weight`` is the ``weight_orig`` of torch's spectral_norm and its gradient is
    ``spectral_weight_grad``'s, (dW - <dW, W_eff> u v^T) / sigma.  Both None: exactly the operator without them."""
    _check("conv3x3", x, weight, bias, in_b8=in_b8, out_b8=out_b8, residual=residual)
    sn = _normalised("conv3x3", weight, weight_scale, spectral, _sn)
    return _Conv.apply(x, weight, bias, bool(in_b8), bool(out_b8), _owner, residual, sn)


def partial_conv_factors(mask, cin):
    """(r, um) of a 3x3 partial convolution over ``cin`` channels with the channel-uniform ``mask`` [N,1,H,W], as its forward defines them
    (partialconv2d.py:61-72): box = conv(mask, ones) = box3x3(mask) * cin, um = clamp(box, 0, 1), ratio = 9 cin / (box + 1e-8) * um;
    r = ratio * um is the factor between the gradient at the output and the gradient at the raw convolution."""
    box = F.avg_pool2d(mask, 3, stride=1, padding=1, divisor_override=1) * float(cin)
    um = torch.clamp(box, 0, 1)
    ratio = float(cin * 9) / (box + 1e-8) * um
    return ratio * um, um


def _partial_conv_backward(ctx, g, xm, r, um, weight):
    """The backward of both partial convolutions, whose inputs are (xm, mask or msum, weight, bias, owner, residual, ...): the gradient at
    the raw convolution gr = g * r and the bias gradient sum g * um (``_scale_bias``), then backward-data and weight gradient of gr."""
    owner, (in_b8, out_b8) = ctx.owner, ctx.layouts
    g = g.contiguous()
    require_device(g)
    need_x, _, need_w, need_b = ctx.needs_input_grad[:4]
    gx = gw = gb = None
    glayout = GRAD_G_B8 if out_b8 else 0
    if need_x or need_w or need_b:
        gr, gb = _scale_bias(g, r, um, need_x or need_w, need_b, glayout)
        if need_x:
            gx = _conv_backward_data(gr, weight, owner, ctx.sn, in_b8, out_b8)
        if need_w:
            gw, _ = _weight_grad(xm, gr, weight.shape[0], False, (GRAD_X_B8 if in_b8 else 0) | glayout)
            if ctx.sn is not None:
                gw = ctx.sn.weight_grad(gw, weight)
    return gx, None, gw, gb, None, (g if ctx.needs_input_grad[5] else None), None, None, None    # (out = ... + residual)


class _PartialConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xm, mask, weight, bias, owner, residual=None, in_b8=False, out_b8=False, sn=None):
        N, cin, H, W = xm.shape
        cout = weight.shape[0]
        buf, arith = _weights_of(weight, owner, sn)
        ctx.sn = sn
        out, um = xm.new_empty(N, cout, H, W), xm.new_empty(N, 1, H, W)
        layout = (nets.IN_B8 if in_b8 else 0) | (nets.OUT_B8 if out_b8 else 0) | (nets.RES_B8 if out_b8 and residual is not None else 0)
        call("slr_pconv3x3_forward", xm.device, xm, None, None, mask, buf, 1.0, 1.0, bias, residual, None, None, out, um,
             N, cin, cout, H, W, layout | arith)
        ctx.save_for_backward(xm, mask, weight)
        ctx.owner, ctx.layouts = owner, (in_b8, out_b8)
        ctx.mark_non_differentiable(um)
        return out, um

    @staticmethod
    def backward(ctx, g, _g_um):
        xm, mask, weight = ctx.saved_tensors
        r, um = partial_conv_factors(mask, weight.shape[1]) if any(ctx.needs_input_grad[:4]) else (None, None)
        return _partial_conv_backward(ctx, g, xm, r, um, weight)


def partial_conv3x3(xm, mask, weight, bias, *, residual=None, in_b8=False, out_b8=False, weight_scale=None, spectral=None, _owner=None,
                    _sn=None):
    """``nets.PartialConv.forward(xm, mask, pre_bn=None)``: PartialConv2d(multi_channel=True, return_mask=True) (partialconv2d.py:41-81)
    of the already activated and masked ``xm`` [N,Cin,H,W] with the channel-uniform ``mask`` [N,1,H,W]; returns (out, update_mask).
    Differentiable in xm, weight and bias; mask and update_mask carry no gradient.  ``residual`` [N,Cout,H,W] (in the result's layout) is
    added in the kernel's epilogue (blocks.py:248) and receives the result's gradient.  in_b8 / out_b8, weight_scale / spectral as
    ``conv3x3``."""
    if bias is None:
        raise ValueError("partial_conv3x3: a bias is required (PartialConv2d adds it inside the mask ratio)")
    _check("partial_conv3x3", xm, weight, bias, mask=mask, in_b8=in_b8, out_b8=out_b8, residual=residual)
    sn = _normalised("partial_conv3x3", weight, weight_scale, spectral, _sn)
    return _PartialConv3x3.apply(xm, mask.detach(), weight, bias, _owner, residual, bool(in_b8), bool(out_b8), sn)


def _learn(conv, spectral):
    """The parameters of a ``nets.Conv`` learn; spectral=True: as torch's spectral_norm leaves the layer -- the parameter ``weight_orig``,
    the buffers ``weight_u`` / ``weight_v`` (normalised randn), no ``weight``."""
    conv.spectral = bool(spectral)
    conv.weight.requires_grad_(True)
    if conv.bias is not None:
        conv.bias.requires_grad_(True)
    if spectral:
        _spectral.make_spectral(conv)


def _w(conv):
    return conv.weight_orig if conv.spectral else conv.weight


def _taken(conv):
    """(weight, normalisation) of this forward: ``weight_orig`` with what the layer's ``SpectralGroup`` took for it, or (weight, None)."""
    return _spectral.taken(conv) if conv.spectral else (conv.weight, None)


class TrainableConv3x3(nets.Conv):
    """``nets.Conv(cin, cout, 3)`` whose parameters learn: same state-dict keys (``weight``, ``bias``), so what
    ``nets.load_reference_state_dict`` reads for a ``nets.Conv`` drops in."""

    def __init__(self, cin, cout, bias=True, spectral=False):
        super().__init__(cin, cout, 3, bias)
        _learn(self, spectral)

    def forward(self, x, in_b8=False, out_b8=False, residual=None):
        w, sn = _taken(self)
        return conv3x3(x, w, self.bias, in_b8=in_b8, out_b8=out_b8, residual=residual, _owner=self, _sn=sn)


class TrainablePartialConv3x3(nets.PartialConv):
    """``nets.PartialConv(cin, cout, 3)`` whose parameters learn; forward(xm, mask) -> (out, update_mask) as ``partial_conv3x3``."""

    def __init__(self, cin, cout, spectral=False):
        super().__init__(cin, cout, 3, True)
        _learn(self, spectral)

    def forward(self, xm, mask, residual=None, in_b8=False, out_b8=False):
        w, sn = _taken(self)
        return partial_conv3x3(xm, mask, w, self.bias, residual=residual, in_b8=in_b8, out_b8=out_b8, _owner=self, _sn=sn)


# --------------------------------------------------------------------------- the rest of the block (csrc/block_grad.hip)

def _check_planes(name, x, b8, mask=None, tables=(), like=()):
    """The same checks for the operators on [N,C,H,W] planes: ``tables`` are [N,C], ``like`` tensors of x's shape."""
    tensors = (x, mask, *tables, *like)
    _check_tensors(name, tensors)
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{name}: input [N,C,H,W] with N, C, H, W >= 1 required, got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if mask is not None and tuple(mask.shape) != (N, 1, H, W):
        raise ValueError(f"{name}: mask {tuple(mask.shape)}, expected {(N, 1, H, W)}")
    for t in tables:
        if t is not None and tuple(t.shape) != (N, C):
            raise ValueError(f"{name}: gain / bias {tuple(t.shape)}, expected {(N, C)}")
    for t in like:
        if t is not None and t.shape != x.shape:
            raise ValueError(f"{name}: {tuple(t.shape)}, expected {tuple(x.shape)}")
    if b8 and C % 8:
        raise ValueError(f"{name}: a channel-blocked tensor needs C % 8 == 0, got {C}")
    if N * C > 65535:
        raise ValueError(f"{name}: N * C <= 65535 required, got {N * C}")
    _check_contiguous(name, tensors)


# entry points of the two mask kinds (csrc/block_grad.hip): workspace size, statistics, forward, backward
_BN_PLANE = ("slr_bn_train_ws_bytes", "slr_bn_batch_stats", "slr_bn_relu_mask_train", "slr_bn_relu_mask_backward")
_BN_NONZERO = ("slr_bn_nonzero_ws_bytes", "slr_bn_nonzero_stats", "slr_bn_relu_nonzero_train", "slr_bn_relu_nonzero_backward")


class _BnReluTrain(torch.autograd.Function):
    """(a, mean, var[, msum][, x]).  ``nonzero``: the mask is k = [x != 0], recomputed from x by every kernel (``mask`` is None then); the
    statistics' count is one per channel, and msum = sum_c k comes back for the partial convolution behind.  With ``fork`` the input comes
    back as the last output, whose gradient the backward adds to dx in its elementwise pass (the block input feeds bn1 and the skip
    branch)."""

    @staticmethod
    def forward(ctx, x, mask, gain, bias, mean, var, eps, b8, fork, nonzero):
        N, C, H, W = x.shape
        ws_bytes, stats, train, _ = _BN_NONZERO if nonzero else _BN_PLANE
        m = () if nonzero else (mask,)                   # (the plane entry points take the mask, in the places below)
        stored = mean is not None
        count = None
        if not stored:
            mean, var, count = x.new_empty(C), x.new_empty(C), x.new_empty(C if nonzero else 1)
            ws = torch.empty(int(getattr(lib(), ws_bytes)(N, C, H, W)), dtype=torch.uint8, device=x.device)
            call(stats, x.device, x, *m, eps, mean, var, count, N, C, H, W, int(b8), ws, ws.numel())
        scale, shift = x.new_empty(N, C), x.new_empty(N, C)
        call("slr_bn_train_tables", x.device, mean, var, gain, bias, eps, scale, shift, N, C)
        a = torch.empty_like(x)
        call(train, x.device, x, scale, shift, *m, a, N, C, H, W, int(b8))
        ctx.save_for_backward(x, mask, gain, scale, shift, mean, var, count)
        ctx.cfg = (eps, b8, stored, bias is not None, fork, nonzero)
        ctx.set_materialize_grads(False)
        out = (a, None, None) if stored else (a, mean, var)
        if nonzero:
            msum = x.new_empty(N, 1, H, W)
            call("slr_nonzero_count_plane", x.device, x, msum, N, C, H, W, int(b8))
            out += (msum,)
        ctx.mark_non_differentiable(*(t for t in out[1:] if t is not None))       # (one call: a second one replaces the first)
        return out + (x,) if fork else out

    @staticmethod
    def backward(ctx, ga, *grads):
        x, mask, gain, scale, shift, mean, var, count = ctx.saved_tensors
        eps, b8, stored, has_bias, fork, nonzero = ctx.cfg
        ws_bytes, _, _, backward = _BN_NONZERO if nonzero else _BN_PLANE
        gskip = grads[-1] if fork else None              # (the gradients of mean, var and msum are not used)
        N, C, H, W = x.shape
        need_x, need_g, need_b = ctx.needs_input_grad[0], gain is not None and ctx.needs_input_grad[2], has_bias and ctx.needs_input_grad[3]
        none = (None,) * 9
        if ga is None:                                   # only the skip branch was used
            return ((gskip if need_x else None),) + none
        ga = ga.contiguous()
        require_device(ga)
        addend = None
        if need_x and gskip is not None:
            addend = gskip.contiguous()
            require_device(addend)
        dx = torch.empty_like(x) if need_x else None
        dgain = x.new_empty(N, C) if need_g else None
        dbias = x.new_empty(N, C) if need_b else None
        if dx is None and dgain is None and dbias is None:
            return (None,) + none
        ws = None
        if not stored or need_g or need_b:
            ws = torch.empty(int(getattr(lib(), ws_bytes)(N, C, H, W)), dtype=torch.uint8, device=x.device)
        call(backward, x.device, x, ga, *(() if nonzero else (mask,)), scale, shift, mean, var, gain, count, eps, addend, dx, dgain, dbias,
             int(stored), N, C, H, W, int(b8), ws, 0 if ws is None else ws.numel())
        return (dx, None, dgain, dbias) + none[:6]


def _bn_relu_train(name, x, mask, gain, bias, mean, var, eps, b8, fork, nonzero):
    """The checks and the call both mask kinds share; with stored statistics the caller's own mean and var come back."""
    _check_planes(name, x, b8, mask, (gain, bias))
    if (mean is None) != (var is None):
        raise ValueError(f"{name}: mean and var go together")
    if mean is not None:
        for t in (mean, var):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (x.shape[1],) or not t.is_contiguous():
                raise ValueError(f"{name}: mean / var: contiguous float32 device tensors ({x.shape[1]},) required")
        mean, var = mean.detach(), var.detach()
    out = _BnReluTrain.apply(x, None if mask is None else mask.detach(), gain, bias, mean, var, float(eps), bool(b8), bool(fork), nonzero)
    if mean is not None:
        out = (out[0], mean, var) + tuple(out[3:])
    return out


def bn_relu_mask_train(x, mask, gain, bias, *, mean=None, var=None, eps=1e-5, b8=False, fork=False):
    """relu(bn(x)) * mask of the block in training mode (blocks.py:225-231 with normalization.py:276-354 and partialconv2d.py:69):
    scale = rsqrt(var + eps) * gain, shift = mean * scale - bias, a = relu(x * scale - shift) * mask, with the batch statistics
    mean = sum x / cnt, var = sum x^2 / cnt - mean^2 over ALL elements of a channel and cnt = N H W (``mask`` None: manual_bn) or
    sum(mask) + eps (``mask`` [N,1,H,W]: partial_manual_bn).  ``gain`` / ``bias``: [N,C] per-sample tables, or None = 1 / 0.  Passing
    ``mean`` and ``var`` [C] selects stored statistics (eval mode).  Returns (a, mean, var); differentiable in x, gain and bias -- the
    gradient to x includes the one through the batch statistics.  b8: x and a are channel-blocked.
    fork=True returns (a, mean, var, x): x again as an output of the same node, for a second consumer of x (the block's skip branch).  The
    gradient arriving at that output is added to dx inside the backward's elementwise pass (the entry point's ``addend``) instead of
    in a pass of its own by autograd."""
    return _bn_relu_train("bn_relu_mask_train", x, mask, gain, bias, mean, var, eps, b8, fork, False)


def conv1x1(x, weight, bias=None, *, in_b8=False, out_b8=False, weight_scale=None, spectral=None, _owner=None, _sn=None):
    """conv2d(x, weight, bias) for a 1x1 ``weight`` [Cout,Cin,1,1] (the block's skip branch, blocks.py:192-193, 243-247) on the fp32 rung,
    differentiable in x, weight and bias; in_b8 / out_b8, weight_scale / spectral as ``conv3x3``."""
    _check("conv1x1", x, weight, bias, in_b8=in_b8, out_b8=out_b8, k=1)
    sn = _normalised("conv1x1", weight, weight_scale, spectral, _sn)
    return _Conv.apply(x, weight, bias, bool(in_b8), bool(out_b8), _owner, None, sn)


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, up, b8):
        N, C, H, W = x.shape
        out = x.new_empty(N, C, 2 * H, 2 * W) if up else x.new_empty(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
        call("slr_upsample_bilinear2x" if up else "slr_avgpool3x3s2", x.device, x, out, N, C, H, W, int(b8))
        ctx.cfg = (tuple(x.shape), up, b8)
        return out

    @staticmethod
    def backward(ctx, g):
        (N, C, H, W), up, b8 = ctx.cfg
        g = g.contiguous()
        require_device(g)
        gin = g.new_empty(N, C, H, W)
        call("slr_upsample_bilinear2x_backward" if up else "slr_avgpool3x3s2_backward", g.device, g, gin, N, C, H, W, int(b8))
        return gin, None, None


def avgpool_down(x, b8=False):
    """nn.AvgPool2d(3, stride=2, padding=1) (blocks.py:196-199), differentiable; b8: x and the result are channel-blocked."""
    _check_planes("avgpool_down", x, b8)
    return _Resample.apply(x, False, bool(b8))


def upsample_up(x, b8=False):
    """nn.Upsample(scale_factor=2, mode='bilinear') (blocks.py:200-203), differentiable; b8: x and the result are channel-blocked."""
    _check_planes("upsample_up", x, b8)
    return _Resample.apply(x, True, bool(b8))


class TrainableConv1x1(nets.Conv):
    """``nets.Conv(cin, cout, 1)`` whose parameters learn (the block's ``conv_b``)."""

    def __init__(self, cin, cout, bias=False, spectral=False):
        super().__init__(cin, cout, 1, bias)
        _learn(self, spectral)

    def forward(self, x, in_b8=False, out_b8=False):
        w, sn = _taken(self)
        return conv1x1(x, w, self.bias, in_b8=in_b8, out_b8=out_b8, _owner=self, _sn=sn)


class TrainableNoiseBN(nn.Module):
    """(Partial)LinearNoiseLayer + ReLU + mask (normalization.py:19-90, 157-354): ``nets.AffineBN``'s buffers ``stored_mean`` /
    ``stored_var`` plus the two bias-free linear maps ``gain`` and ``bias`` from the noise [N,noise_sz] (torch ops: [N,20] x [20,C] is
    not tensor-sized).  Training: batch statistics, the stored ones updated with momentum 0.1; eval: stored statistics, zero noise."""

    def __init__(self, ch, noise_sz=20, eps=1e-5, momentum=0.1, spectral=False):
        super().__init__()
        self.eps, self.momentum, self.noise_sz, self.spectral = eps, momentum, noise_sz, bool(spectral)
        self.register_buffer("stored_mean", torch.zeros(ch))
        self.register_buffer("stored_var", torch.ones(ch))
        if spectral:                                     # keys gain.weight_orig / gain.weight_u / gain.weight_v, as the reference's
            self.register_buffer("accumulation_counter", torch.zeros(1))      # normalization.py:167, 266: in its state dicts; carried
            self.gain, self.bias = _spectral.SpectralLinear(noise_sz, ch), _spectral.SpectralLinear(noise_sz, ch)
        else:
            self.gain, self.bias = nn.Linear(noise_sz, ch, bias=False), nn.Linear(noise_sz, ch, bias=False)

    def forward(self, x, mask, noise=None, b8=False, fork=False, nonzero=False):
        """relu(bn(x)) * mask (``mask`` None: no mask, the plain BN of the encoder blocks).  ``noise`` [N,noise_sz]; None draws
        torch.randn in training mode and means zeros in eval mode.  Returns ``bn_relu_mask_train``'s tuple; b8 and fork as there.
        nonzero=True (``mask`` None): the per-element mask x != 0 of the decoder's first block, ``bn_relu_nonzero_train``'s tuple."""
        if nonzero and mask is not None:
            raise ValueError("TrainableNoiseBN: nonzero=True derives the mask from x; pass mask=None")
        if self.spectral:
            _spectral.begin(self)
        if noise is None:
            noise = (torch.randn if self.training else torch.zeros)(x.shape[0], self.noise_sz, device=x.device, dtype=x.dtype)
        gain, bias = (1.0 + self.gain(noise)).contiguous(), self.bias(noise).contiguous()
        bn = (lambda **kw: bn_relu_nonzero_train(x, gain, bias, **kw)) if nonzero else (lambda **kw: bn_relu_mask_train(x, mask, gain, bias, **kw))
        if not self.training:
            return bn(mean=self.stored_mean, var=self.stored_var, eps=self.eps, b8=b8, fork=fork)
        out = bn(eps=self.eps, b8=b8, fork=fork)
        with torch.no_grad():                            # normalization.py:287-300
            self.stored_mean.mul_(1.0 - self.momentum).add_(out[1], alpha=self.momentum)
            self.stored_var.mul_(1.0 - self.momentum).add_(out[2], alpha=self.momentum)
        return out


def _block_forward(block, b8_in, noise, first):
    """What the three blocks' forwards share -> (y, update mask or None, b8_out).  ``first(noise1, b8)`` -> (a, mask or None, x again): the
    block's own bn1 + conv_aa, bn1 called with fork=True.  Then bn2 -> conv_ab + conv_b(x) (or + x) in its epilogue -> one resampling of the
    sum (both resamplers are linear, as in ``nets.PconvResBlock``).  A mask selects the partial form of bn2 and conv_ab."""
    if block.spectral:
        _spectral.begin(block)
    cout = _w(block.conv_aa).shape[0]
    b8 = cout % 8 == 0 if block.conv_b is not None else bool(b8_in)
    n1, n2 = noise if noise is not None else (None, None)
    a, m, xs = first(n1, b8)
    a = block.bn2(a, m, n2, b8=b8)[0]                                                # blocks.py:233-238 / 73-75
    skip = block.conv_b(xs, in_b8=b8_in, out_b8=b8) if block.conv_b is not None else xs      # :243-247 / 78-81
    if m is None:
        a = block.conv_ab(a, in_b8=b8, out_b8=b8, residual=skip)                     # :87
    else:
        a, m = block.conv_ab(a, m, residual=skip, in_b8=b8, out_b8=b8)               # :239, 248
    if block.kind == "Up":
        a = upsample_up(a, b8)
    elif block.kind:
        a = avgpool_down(a, b8)
    return a, m, b8


class TrainablePconvResBlock(nets.PconvResBlock):
    """``nets.PconvResBlock`` (ResNet_Block_Pconv2 with pconv_pbn_woresbias, blocks.py:173-248) as one differentiable unit in training or
    eval mode: same sub-module names and state-dict keys (``nets.load_reference_state_dict`` fills it), the BNs with their noise weights
    ``bn1.gain.weight`` ... as extra keys."""

    def __init__(self, cin, cout, resample=None, spectral=False):
        super().__init__(cin, cout, resample)
        self.spectral = sn = bool(spectral)
        self.bn1, self.bn2 = TrainableNoiseBN(cin, spectral=sn), TrainableNoiseBN(cout, spectral=sn)
        self.conv_aa, self.conv_ab = TrainablePartialConv3x3(cin, cout, spectral=sn), TrainablePartialConv3x3(cout, cout, spectral=sn)
        self.conv_b = TrainableConv1x1(cin, cout, spectral=sn) if self.conv_b is not None else None
        if sn and self.conv_b is None:                   # the reference builds conv_b in every block (blocks.py:192-195): keep its tensors
            self.conv_b_unused = _spectral.UnusedSpectralConv(cin, cout)
        self.kind = resample

    def forward(self, x, mask, b8_in=False, noise=None):
        """-> (y, update_mask, b8_out).  ``mask`` [N,1,H,W] channel-uniform; ``b8_in`` / ``b8_out``: x / y are channel-blocked;
        ``noise`` None or the pair (noise1, noise2) of the two BNs.  bn1 -> conv_aa -> bn2 -> conv_ab + conv_b(x) (or + x) in its epilogue ->
        one resampling of the sum (both resamplers are linear, as in ``nets.PconvResBlock``) -> the mask resampled."""
        if mask is None:
            raise ValueError("TrainablePconvResBlock: an explicit mask [N,1,H,W] is required (the per-element mask x != 0 is TrainablePconvInputBlock's)")
        _check_planes("TrainablePconvResBlock", x, b8_in, mask)

        def first(n1, b8):                               # blocks.py:225-231
            a, _, _, xs = self.bn1(x, mask, n1, b8=b8_in, fork=True)
            return self.conv_aa(a, mask, in_b8=b8_in, out_b8=b8) + (xs,)
        a, m, b8 = _block_forward(self, b8_in, noise, first)
        return a, self.resample_mask(m), b8


# --------------------------------------------------------------------------- the decoder's first block (csrc/decoder_grad.hip)

def bn_relu_nonzero_train(x, gain, bias, *, mean=None, var=None, eps=1e-5, b8=False, fork=False):
    """``bn_relu_mask_train`` with the per-element mask k = (x != 0) of the decoder's first block (architectures.py:369; the mask is never
    materialised): cnt[c] = sum k + eps, mean = sum x / cnt, var = sum x^2 / cnt - mean^2 per channel (normalization.py:319-335 with a
    [N,C,H,W] mask), a = relu(x * scale - shift) * k.  Returns (a, mean, var, msum[, x]) with msum [N,1,H,W] = sum_c k, what the partial
    convolution behind it needs (``partial_conv3x3_counts``).  Differentiable in x, gain and bias; the gradient through the statistics
    reaches the zero elements of x too, as the reference's autograd gives it.  mean / var, b8 and fork as ``bn_relu_mask_train``."""
    return _bn_relu_train("bn_relu_nonzero_train", x, None, gain, bias, mean, var, eps, b8, fork, True)


def _factors_counts(msum, cin):
    box = F.avg_pool2d(msum, 3, stride=1, padding=1, divisor_override=1)
    um = torch.clamp(box, 0, 1)
    return float(cin * 9) / (box + 1e-8) * um, um


def partial_conv_factors_counts(msum, cin):
    """``partial_conv_factors`` for a per-element mask given as its count plane ``msum`` [N,1,H,W] = sum_c mask (partialconv2d.py:61-72
    with a [N,Cin,H,W] mask): box = conv(mask, ones) = box3x3(msum), um = clamp(box, 0, 1), ratio = 9 cin / (box + 1e-8) * um; returns
    (r, um), r = ratio * um."""
    _check_planes("partial_conv_factors_counts", msum, False)
    if msum.shape[1] != 1:
        raise ValueError(f"partial_conv_factors_counts: msum [N,1,H,W] required, got {tuple(msum.shape)}")
    ratio, um = _factors_counts(msum, cin)
    return ratio * um, um


class _PartialConv3x3Counts(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xm, msum, weight, bias, owner, residual=None, in_b8=False, out_b8=False, sn=None):
        N, cin, H, W = xm.shape
        cout = weight.shape[0]
        buf, arith = _weights_of(weight, owner, sn)
        ctx.sn = sn
        ratio, um = _factors_counts(msum, cin)
        out = _conv(xm, buf, arith, None, cout, (nets.IN_B8 if in_b8 else 0) | (nets.OUT_B8 if out_b8 else 0))
        call("slr_pconv_train_epilogue", xm.device, out, ratio, um, bias, residual, out, N, cout, H, W, int(out_b8))
        ctx.save_for_backward(xm, ratio, um, weight)     # (um is 0 or 1: ratio * um has ratio's bits, it is r)
        ctx.owner, ctx.layouts = owner, (in_b8, out_b8)
        ctx.mark_non_differentiable(um)
        return out, um

    @staticmethod
    def backward(ctx, g, _g_um):
        return _partial_conv_backward(ctx, g, *ctx.saved_tensors)


def partial_conv3x3_counts(xm, msum, weight, bias, *, residual=None, in_b8=False, out_b8=False, weight_scale=None, spectral=None,
                           _owner=None, _sn=None):
    """``partial_conv3x3`` for a per-element mask given as its count plane: ``xm`` [N,Cin,H,W] already activated and masked, ``msum``
    [N,1,H,W] = sum_c mask (``bn_relu_nonzero_train``'s).  A bias-free convolution on the fp32 rung, then
    out = (raw * ratio + bias) * um (+ residual) with the factors of ``partial_conv_factors_counts``; returns (out, update_mask).
    Differentiable in xm, weight, bias and residual; weight_scale / spectral as ``conv3x3``."""
    if bias is None:
        raise ValueError("partial_conv3x3_counts: a bias is required (PartialConv2d adds it inside the mask ratio)")
    _check("partial_conv3x3_counts", xm, weight, bias, mask=msum, in_b8=in_b8, out_b8=out_b8, residual=residual)
    sn = _normalised("partial_conv3x3_counts", weight, weight_scale, spectral, _sn)
    return _PartialConv3x3Counts.apply(xm, msum.detach(), weight, bias, _owner, residual, bool(in_b8), bool(out_b8), sn)


class TrainablePconvInputBlock(TrainablePconvResBlock):
    """The decoder's first block: ``TrainablePconvResBlock`` called with the per-element mask (x != 0) (architectures.py:369).  Same
    sub-modules and state-dict keys as its parent."""

    def forward(self, x, b8_in=False, noise=None):
        """-> (y, update_mask, b8_out); arguments as the parent's, without the mask."""
        _check_planes("TrainablePconvInputBlock", x, b8_in)

        def first(n1, b8):                               # blocks.py:225-231 -- the mask is channel-uniform after conv_aa
            a, _, _, msum, xs = self.bn1(x, None, n1, b8=b8_in, fork=True, nonzero=True)
            w, sn = _taken(self.conv_aa)
            return partial_conv3x3_counts(a, msum, w, self.conv_aa.bias, in_b8=b8_in, out_b8=b8, _owner=self.conv_aa, _sn=sn) + (xs,)
        a, m, b8 = _block_forward(self, b8_in, noise, first)
        return a, self.resample_mask(m), b8


# --------------------------------------------------------------------------- the plain block and the networks

class TrainableResBlock(nets.ResBlock):
    """``nets.ResBlock`` (ResNet_Block, blocks.py:47-87) as one differentiable unit in training or eval mode: the noise-conditioned
    batch-norm without a mask (manual_bn), two 3x3 convolutions, the 1x1 skip convolution with its bias.  Same sub-module names and
    state-dict keys, the BNs' noise layers as extra keys."""

    def __init__(self, cin, cout, resample=None, spectral=False):
        super().__init__(cin, cout, resample)
        self.spectral = sn = bool(spectral)
        self.bn1, self.bn2 = TrainableNoiseBN(cin, spectral=sn), TrainableNoiseBN(cout, spectral=sn)
        self.conv_aa, self.conv_ab = TrainableConv3x3(cin, cout, spectral=sn), TrainableConv3x3(cout, cout, spectral=sn)
        self.conv_b = TrainableConv1x1(cin, cout, bias=True, spectral=sn) if self.conv_b is not None else None
        self.kind = resample

    def forward(self, x, b8_in=False, noise=None):
        """-> (y, b8_out).  bn1 -> conv_aa -> bn2 -> conv_ab + conv_b(x) (or + x) in its epilogue -> one resampling of the sum."""
        _check_planes("TrainableResBlock", x, b8_in)

        def first(n1, b8):                               # blocks.py:69-72
            a, _, _, xs = self.bn1(x, None, n1, b8=b8_in, fork=True)
            return self.conv_aa(a, in_b8=b8_in, out_b8=b8), None, xs
        a, _, b8 = _block_forward(self, b8_in, noise, first)
        return a, b8


def _net_plan(name, first, inner, last, widths, updown, default_updown):
    widths = list(inner if widths is None else widths)
    updown = list(default_updown if updown is None else updown)
    if len(updown) != len(widths) + 1:
        raise ValueError(f"{name}: {len(widths)} inner widths need {len(widths) + 1} resampling entries, got {len(updown)}")
    if any(u is not None and u is not False and u not in ("Down", "Up") for u in updown):
        raise ValueError(f"{name}: updown entries are None / False, 'Down' or 'Up', got {updown}")
    if any(not isinstance(c, int) or c < 1 for c in [first, last] + widths):
        raise ValueError(f"{name}: channel counts are positive integers")
    if last % 8 == 0:
        raise ValueError(f"{name}: the net ends in NCHW; its last channel count must not be a multiple of 8, got {last}")
    return [first] + widths + [last], [u or None for u in updown]


def _noise_of(noise, n):
    if noise is None:
        return [None] * n
    if len(noise) != n:
        raise ValueError(f"noise: one (noise1, noise2) pair per block required, got {len(noise)} for {n} blocks")
    return list(noise)


class _TrainableResNet:
    """forward of the nets made of ``TrainableResBlock``s: the blocks in order, NCHW at the end."""

    def _run(self, x, noise):
        if self.spectral:                                # sigma of every tensor and every prepared buffer: at most four launches for the network
            _spectral.begin(self, force=True)
        b8 = False
        for blk, nz in zip(self.blocks, _noise_of(noise, len(self.blocks))):
            x, b8 = blk(x, b8, noise=nz)
        assert not b8                                    # the few-channel end is NCHW
        return x


class TrainableEncoderWithZ(_TrainableResNet, nets.EncoderWithZ):
    """``nets.EncoderWithZ`` (ResNetEncoder_with_Z, architectures.py:155-197) whose weights learn.  widths: the seven inner widths
    (default nets._ENC[1:]); updown: the eight blocks' resampling (default none)."""

    def __init__(self, cin=3, feat=64, *, widths=None, updown=None, spectral=False):
        nn.Module.__init__(self)
        self.spectral = bool(spectral)
        n = len(nets._ENC[1:] if widths is None else widths) + 1
        ch, ud = _net_plan("TrainableEncoderWithZ", cin, nets._ENC[1:], feat + 1, widths, updown, [None] * n)
        self.blocks = nn.ModuleList(TrainableResBlock(ch[i], ch[i + 1], ud[i], spectral) for i in range(len(ud)))

    def forward(self, x, noise=None):
        x = self._run(x, noise)
        return x[:, :-1].contiguous(), x[:, -1:].contiguous()          # :195-197


class TrainableEncoder(_TrainableResNet, nets.Encoder):
    """``nets.Encoder`` (ResNetEncoder, architectures.py:121-153) whose weights learn; widths / updown as ``TrainableEncoderWithZ``."""

    def __init__(self, cin=3, cout=2, *, widths=None, updown=None, spectral=False):
        nn.Module.__init__(self)
        self.spectral = bool(spectral)
        n = len(nets._ENC[1:] if widths is None else widths) + 1
        ch, ud = _net_plan("TrainableEncoder", cin, nets._ENC[1:], cout, widths, updown, [None] * n)
        self.blocks = nn.ModuleList(TrainableResBlock(ch[i], ch[i + 1], ud[i], spectral) for i in range(len(ud)))

    def forward(self, x, noise=None):
        return self._run(x, noise)


class TrainableBGDecoder(_TrainableResNet, nets.BGDecoder):
    """``nets.BGDecoder`` (ResNetBGDecoder, architectures.py:233-260) whose weights learn.  widths: the inner widths (default nets._DEC);
    updown: the blocks' resampling (default nets._UPDOWN)."""

    def __init__(self, cin=3, cout=3, *, widths=None, updown=None, spectral=False):
        nn.Module.__init__(self)
        self.spectral = bool(spectral)
        ch, ud = _net_plan("TrainableBGDecoder", cin, nets._DEC, cout, widths, updown, nets._UPDOWN)
        self.blocks = nn.ModuleList(TrainableResBlock(ch[i], ch[i + 1], ud[i], spectral) for i in range(len(ud)))

    def forward(self, x, noise=None):
        return self._run(x, noise)


class TrainableDecoderPconv2(nets.DecoderPconv2):
    """``nets.DecoderPconv2`` (ResNetDecoderPconv2, architectures.py:345-375) whose weights learn: block 0 is a
    ``TrainablePconvInputBlock`` (mask = x != 0, :369), the others ``TrainablePconvResBlock``s.  widths / updown as ``TrainableBGDecoder``."""

    def __init__(self, cin=64, cout=3, *, widths=None, updown=None, spectral=False):
        nn.Module.__init__(self)
        self.spectral = bool(spectral)
        ch, ud = _net_plan("TrainableDecoderPconv2", cin, nets._DEC, cout, widths, updown, nets._UPDOWN)
        self.blocks = nn.ModuleList((TrainablePconvResBlock if i else TrainablePconvInputBlock)(ch[i], ch[i + 1], ud[i], spectral)
                                    for i in range(len(ud)))

    def forward(self, x, noise=None):
        if self.spectral:
            _spectral.begin(self, force=True)
        noise = _noise_of(noise, len(self.blocks))
        x, mask, b8 = self.blocks[0](x, False, noise=noise[0])
        for blk, nz in zip(self.blocks[1:], noise[1:]):
            x, mask, b8 = blk(x, mask, b8, noise=nz)
        assert not b8                                    # the 1- / 3-channel end is NCHW
        return x
