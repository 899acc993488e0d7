"""3x3 convolutions whose weights learn: the plain and the partial 3x3 / stride 1 / pad 1 convolution of the reference's decoder
(models/layers/blocks.py:66-87, models/layers/partialconv2d.py:41-81) as differentiable operators in input, weight and bias.

Forward: the package's fp32 rung (``nets.fp32_kernels(winograd=False)``: fp32 operands, products and accumulation on the matrix cores, the
arithmetic of ``nn.Conv2d``).  Backward: the gradient to the input is the same forward kernel with flipped, transposed weights; weight and
bias gradients come from ``slr_conv3x3_weight_grad`` / ``slr_conv_grad_scale_bias`` (csrc/conv_grad.hip).  Only what ``needs_input_grad``
asks for is computed.  Nothing synchronises; every result has the same bits from run to run.  There is no fallback: CPU tensors raise, a
missing library raises.

Not here (compositions on top of this primitive): batch-statistics BN, spectral normalisation, the 1x1 skip branch, the
backward of pooling / up-sampling, and BN + ReLU fused into the backward's prologue.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import nets
from ._lib import call, lib, require_device

GRAD_X_B8, GRAD_G_B8 = 1, 2              # include/slr_splat.h: SLR_GRAD_X_B8 / SLR_GRAD_G_B8


def _check(name, x, weight, bias, mask=None, in_b8=False, out_b8=False):
    """Types, device, dtype, shapes and layouts -- before anything touches the device."""
    tensors = (x, weight, bias, mask)
    for t in tensors:
        if t is not None and not torch.is_tensor(t):
            raise TypeError(f"slr_sfs_amd.{name}: tensors required, got {type(t).__name__}")
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype}")
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{name}: input [N,Cin,H,W] with N, Cin, H, W >= 1 required, got {tuple(x.shape)}")
    N, cin, H, W = x.shape
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (cin, 3, 3) or weight.shape[0] < 1:
        raise ValueError(f"{name}: weight {tuple(weight.shape)}, expected [Cout,{cin},3,3]")
    cout = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"{name}: bias {tuple(bias.shape)}, expected ({cout},)")
    if mask is not None and tuple(mask.shape) != (N, 1, H, W):
        raise ValueError(f"{name}: mask {tuple(mask.shape)}, expected {(N, 1, H, W)}")
    if in_b8 and cin % 8:
        raise ValueError(f"{name}: a channel-blocked input needs Cin % 8 == 0, got {cin}")
    if out_b8 and cout % 8:
        raise ValueError(f"{name}: a channel-blocked output needs Cout % 8 == 0, got {cout}")
    for label, t in (("input", x), ("weight", weight), ("bias", bias), ("mask", mask)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: {label} is not contiguous")
    require_device(*tensors)


class _Prepared(nets.Conv):
    """``nets.Conv``'s weight preparation and its cache (keyed on the weight's data pointer, version and device) around a weight tensor
    somebody else owns."""

    def __init__(self, weight):
        nn.Module.__init__(self)
        object.__setattr__(self, "weight", weight)      # (not registered: the tensor stays its owner's)
        object.__setattr__(self, "bias", None)
        self.cin, self.k, self.pad = weight.shape[1], 3, 1


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


def _conv(x, buf, arith, bias, cout, layout):
    N, cin, H, W = x.shape
    out = x.new_empty(N, cout, H, W)
    call("slr_conv3x3_forward", x.device, x, buf, bias, None, out, N, cin, cout, H, W, 1.0, 1.0, None, None, layout | arith)
    return out


def _grad_ws(x, cout, splits=0):
    N, cin, H, W = x.shape
    nbytes = int(lib().slr_conv3x3_grad_ws_bytes(N, cin, cout, H, W, splits))
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device)


def _weight_grad(x, g, cout, want_bias, layout, splits=0):
    N, cin, H, W = x.shape
    dw = x.new_empty(cout, cin, 3, 3)
    db = x.new_empty(cout) if want_bias else None
    ws = _grad_ws(x, cout, splits)
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


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, in_b8, out_b8, owner):
        buf, arith = _forward_weights(weight, owner)
        layout = (nets.IN_B8 if in_b8 else 0) | (nets.OUT_B8 if out_b8 else 0)
        out = _conv(x, buf, arith, bias, weight.shape[0], layout)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (in_b8, out_b8, owner, bias is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        in_b8, out_b8, owner, has_bias = ctx.cfg
        g = g.contiguous()
        require_device(g)
        cout, cin = weight.shape[:2]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = None
        if need_x:
            buf, arith = _backward_weights(weight, owner)
            gx = _conv(g, buf, arith, None, cin, (nets.IN_B8 if out_b8 else 0) | (nets.OUT_B8 if in_b8 else 0))
        glayout = GRAD_G_B8 if out_b8 else 0
        if need_w:
            gw, gb = _weight_grad(x, g, cout, need_b, (GRAD_X_B8 if in_b8 else 0) | glayout)
        elif need_b:
            _, gb = _scale_bias(g, None, None, False, True, glayout)
        return gx, gw, gb, None, None, None


def conv3x3(x, weight, bias=None, *, in_b8=False, out_b8=False, _owner=None):
    """conv2d(x, weight, bias, stride 1, padding 1) for a 3x3 ``weight`` [Cout,Cin,3,3], differentiable in x, weight and bias.

    in_b8 / out_b8: x / the result (and with them their gradients) are channel-blocked, [N,C/8,H,W,8] in memory under the logical shape
    [N,C,H,W] -- the package's activation layout (nets._b8); C % 8 == 0 then."""
    _check("conv3x3", x, weight, bias, in_b8=in_b8, out_b8=out_b8)
    return _Conv3x3.apply(x, weight, bias, bool(in_b8), bool(out_b8), _owner)


def partial_conv_factors(mask, cin):
    """(r, um) of a 3x3 partial convolution over ``cin`` channels with the channel-uniform ``mask`` [N,1,H,W], as its forward defines them
    (partialconv2d.py:61-72): box = conv(mask, ones) = box3x3(mask) * cin, um = clamp(box, 0, 1), ratio = 9 cin / (box + 1e-8) * um;
    r = ratio * um is the factor between the gradient at the output and the gradient at the raw convolution."""
    box = F.avg_pool2d(mask, 3, stride=1, padding=1, divisor_override=1) * float(cin)
    um = torch.clamp(box, 0, 1)
    ratio = float(cin * 9) / (box + 1e-8) * um
    return ratio * um, um


class _PartialConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xm, mask, weight, bias, owner):
        N, cin, H, W = xm.shape
        cout = weight.shape[0]
        buf, arith = _forward_weights(weight, owner)
        out, um = xm.new_empty(N, cout, H, W), xm.new_empty(N, 1, H, W)
        call("slr_pconv3x3_forward", xm.device, xm, None, None, mask, buf, 1.0, 1.0, bias, None, None, None, out, um,
             N, cin, cout, H, W, arith)
        ctx.save_for_backward(xm, mask, weight)
        ctx.owner = owner
        ctx.mark_non_differentiable(um)
        return out, um

    @staticmethod
    def backward(ctx, g, _g_um):
        xm, mask, weight = ctx.saved_tensors
        owner = ctx.owner
        g = g.contiguous()
        require_device(g)
        cout, cin = weight.shape[:2]
        need_x, _, need_w, need_b = ctx.needs_input_grad[:4]
        gx = gw = gb = None
        if need_x or need_w or need_b:
            r, um = partial_conv_factors(mask, cin)
            gr, gb = _scale_bias(g, r, um, need_x or need_w, need_b)
            if need_x:
                buf, arith = _backward_weights(weight, owner)
                gx = _conv(gr, buf, arith, None, cin, 0)
            if need_w:
                gw, _ = _weight_grad(xm, gr, cout, False, 0)
        return gx, None, gw, gb, None


def partial_conv3x3(xm, mask, weight, bias, *, _owner=None):
    """``nets.PartialConv.forward(xm, mask, pre_bn=None)``: PartialConv2d(multi_channel=True, return_mask=True) (partialconv2d.py:41-81)
    of the already activated and masked ``xm`` [N,Cin,H,W] with the channel-uniform ``mask`` [N,1,H,W]; returns (out, update_mask).
    Differentiable in xm, weight and bias; mask and update_mask carry no gradient.  NCHW tensors."""
    if bias is None:
        raise ValueError("partial_conv3x3: a bias is required (PartialConv2d adds it inside the mask ratio)")
    _check("partial_conv3x3", xm, weight, bias, mask=mask)
    return _PartialConv3x3.apply(xm, mask.detach(), weight, bias, _owner)


class TrainableConv3x3(nets.Conv):
    """``nets.Conv(cin, cout, 3)`` whose parameters learn: same state-dict keys (``weight``, ``bias``), so what
    ``nets.load_reference_state_dict`` reads for a ``nets.Conv`` drops in."""

    def __init__(self, cin, cout, bias=True):
        super().__init__(cin, cout, 3, bias)
        self.weight.requires_grad_(True)
        if self.bias is not None:
            self.bias.requires_grad_(True)

    def forward(self, x, in_b8=False, out_b8=False):
        return conv3x3(x, self.weight, self.bias, in_b8=in_b8, out_b8=out_b8, _owner=self)


class TrainablePartialConv3x3(nets.PartialConv):
    """``nets.PartialConv(cin, cout, 3)`` whose parameters learn; forward(xm, mask) -> (out, update_mask) as ``partial_conv3x3``."""

    def __init__(self, cin, cout):
        super().__init__(cin, cout, 3, True)
        self.weight.requires_grad_(True)
        self.bias.requires_grad_(True)

    def forward(self, xm, mask):
        return partial_conv3x3(xm, mask, self.weight, self.bias, _owner=self)
