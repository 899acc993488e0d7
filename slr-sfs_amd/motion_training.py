"""The operators that train the SPADE motion U-Net (the reference's train_motion_unet.py with --model_type SPADE_unet_mask_motion:
models/networks/architectures.py:602-743, models/networks/networks.py:422-463, models/losses/synthesis.py:11-58, 142-160), differentiable,
on csrc/motion_grad.hip, csrc/conv4x4.hip and csrc/disc.hip (ABI 23):

  conv4x4s2               Conv2d(Cin, Cout, 4, stride 2, padding 1) with the LeakyReLU in front of it, weight_scale / spectral as conv3x3
  instnorm_spade_train    instance norm + SPADE modulation, gradient to x and to gamma | beta
  upsample2x_concat_train the decoder's mixed bilinear / nearest x2 up-sampling + concatenation (+ ReLU), gradient to both sources
  motion_losses           EndPointError, MotionL1 and the PSNR's squared error in one pass, gradient to the prediction

Every operator is an autograd Function whose backward runs once; argument checks run before the device is touched; CPU tensors raise
NotImplementedError; there is no torch fallback.  Nothing synchronises host and device and every result has the same bits from run to
run.  DESIGN 3.17.

On top of them: TrainableSPADEIN and TrainableSPADEUnet4MaskMotion (the network in train() and eval() mode, state dicts in the reference's
unfolded keys), MotionLoss (the reference's dictionary of weighted terms) and MotionTrainingModel (the reference's
SPADEUnetMaskMotion.forward(batch)).

Not here: Unet4Motion with training-mode BatchNorm, a MotionTrainer (base_model_motion.BaseModel), --train_motion inside TrainingModel
(still refused), the online-hint dataset.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import spectral as _spectral
from ._lib import call, lib, require_device
from .nets import RELU_AFTER, RELU_BEFORE, RELU_NONE, _MOTION_DEC_NORM, _MOTION_ENC_NORM, _check_motion_grid, resize_segmap
from .trainable import TrainableConv3x3, conv3x3

__all__ = ["conv4x4s2", "instnorm_spade_train", "upsample2x_concat_train", "motion_losses", "MotionLoss", "TrainableSPADEIN",
           "TrainableSPADEUnet4MaskMotion", "MotionTrainingModel", "RELU_NONE", "RELU_BEFORE", "RELU_AFTER"]


def _bytes(n, like):
    return torch.empty(int(n), dtype=torch.uint8, device=like.device)


def _check(name, tensors, optional=()):
    """tensors: {argument name: tensor}; those named in ``optional`` may be None.  Type, device, dtype and contiguity -- before anything
    touches the device."""
    for what, t in tensors.items():
        if not torch.is_tensor(t) and not (t is None and what in optional):
            raise TypeError(f"slr_sfs_amd.{name}: {what}: a tensor is required, got {type(t).__name__}")
    for what, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
    first = None
    for what, t in tensors.items():
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise TypeError(f"slr_sfs_amd: float32 tensors required, got {t.dtype} ({name}: {what})")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} is not contiguous")
        if first is None:
            first = t
        elif t.device != first.device:
            raise ValueError(f"{name}: {what} lives on {t.device}, not on {first.device}")


# ---------------------------------------------------------------------------------------------- the encoder convolution

def _prepared(weight, scale, backward):
    """The MFMA fragments of ``weight`` [Cout,Cin,4,4] times the device scalar ``scale`` (or 1).  backward: the parity-class fragments of
    the stride-2 data gradient, which the padding-1 kernel reads with the class bits flipped (csrc/conv4x4.hip, C4_ENCB2)."""
    cout, cin = weight.shape[:2]
    buf = _bytes(lib().slr_conv4x4_weight_bytes(cout, cin, backward), weight)
    call("slr_conv4x4_f32_weights", weight.device, weight, scale, buf, cout, cin, 2, backward)
    return buf


class _Conv4x4s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, scale, u, v, leaky, splits):
        N, cin, H, W = x.shape
        cout = weight.shape[0]
        out = x.new_empty(N, cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1)
        call("slr_conv4x4s2_forward", x.device, x, _prepared(weight, scale, 0), bias, None, None, out, N, cin, cout, H, W,
             int(leaky is not None), float(leaky or 0.0))
        ctx.save_for_backward(x, weight, scale, u, v)
        ctx.cfg = (leaky, bias is not None, splits)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight, scale, u, v = ctx.saved_tensors
        leaky, has_bias, splits = ctx.cfg
        g = g.contiguous()
        require_device(g)
        N, cin, H, W = x.shape
        cout = weight.shape[0]
        slope = float(leaky or 0.0)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = None
        if need_x:
            gx = torch.empty_like(x)
            call("slr_conv4x4s2_backward_data", x.device, g, x if leaky is not None else None, _prepared(weight, scale, 1), gx, N, cin, cout,
                 H, W, slope)
        if need_w or need_b:
            dw = torch.empty_like(weight)                # the gradient at the effective weight, weight * scale
            gb = x.new_empty(cout) if need_b else None
            ws = _bytes(lib().slr_conv4x4s2_grad_ws_bytes(N, cin, cout, H, W, splits), x)
            call("slr_conv4x4s2_weight_grad", x.device, x, g, dw, gb, N, cin, cout, H, W, int(leaky is not None), slope, splits, ws, ws.numel())
            if need_w:
                if scale is None:
                    gw = dw
                elif u is None:
                    gw = dw * scale
                else:
                    gw = _spectral._weight_grad(dw, weight, u, v, scale)
        return gx, gw, gb, None, None, None, None, None


def conv4x4s2(x, weight, bias=None, *, leaky=None, weight_scale=None, spectral=None, _splits=0):
    """conv2d(pre(x), weight * weight_scale, bias, stride 2, padding 1) for a 4x4 ``weight`` [Cout,Cin,4,4]: the encoder convolution of
    the motion U-Nets.  ``leaky``: the slope of the LeakyReLU in FRONT of the convolution (pre = leaky_relu(., leaky); None: identity, as
    for conv1).  ``weight_scale`` / ``spectral=(u, v)`` mean what they mean on ``conv3x3``: a one-element device tensor folded into the
    weight preparation, a constant of the gradient; with ``spectral`` the weight is torch's ``weight_orig`` and its gradient
    ``spectral_weight_grad``'s.  x [N,Cin,H,W] with H, W >= 2 (odd sizes included) -> [N,Cout,(H-2)//2+1,(W-2)//2+1].  Differentiable in
    x, weight and bias; a gradient whose input does not require it is not computed."""
    _check("conv4x4s2", {"x": x, "weight": weight, "bias": bias}, optional=("bias",))
    if x.dim() != 4 or min(x.shape) < 1 or x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError(f"conv4x4s2: input [N,C,H,W] with H, W >= 2 required, got {tuple(x.shape)}")
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 4, 4):
        raise ValueError(f"conv4x4s2: weight {tuple(weight.shape)}, expected [Cout,{x.shape[1]},4,4]")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv4x4s2: bias {tuple(bias.shape)}, expected ({weight.shape[0]},)")
    if leaky is not None and not (isinstance(leaky, (int, float)) and not isinstance(leaky, bool) and 0.0 <= float(leaky) < 1.0):
        raise ValueError(f"conv4x4s2: leaky is the slope of the LeakyReLU in front (a number in [0, 1)) or None, got {leaky!r}")
    _spectral.check_spectral("conv4x4s2", weight, weight_scale, spectral)
    u, v = spectral if spectral is not None else (None, None)
    det = lambda t: None if t is None else t.detach()     # noqa: E731
    return _Conv4x4s2.apply(x, weight, bias, det(weight_scale), det(u), det(v), None if leaky is None else float(leaky), int(_splits))


# ---------------------------------------------------------------------------------------------- SPADE instance norm

class _InstNormSpade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma_beta, eps):
        N, C, H, W = x.shape
        out, mean, rstd = torch.empty_like(x), x.new_empty(N * C), x.new_empty(N * C)
        call("slr_instnorm_spade_train_forward", x.device, x, gamma_beta, out, mean, rstd, N, C, H, W, eps)
        ctx.save_for_backward(x, gamma_beta, mean, rstd)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, gamma_beta, mean, rstd = ctx.saved_tensors
        g = g.contiguous()
        require_device(g)
        gx, dgb = torch.empty_like(x), torch.empty_like(gamma_beta)
        call("slr_instnorm_spade_backward", x.device, x, gamma_beta, g, mean, rstd, gx, dgb, *x.shape)
        return gx, dgb, None


def instnorm_spade_train(x, gamma_beta, eps=1e-5):
    """SPADE with InstanceNorm2d (networks.py:441-463): instance_norm(x, eps) * (1 + gamma) + beta with gamma_beta = cat(gamma, beta)
    [N,2C,H,W], planes of at least 2 x 2.  The forward is the inference kernel's code (bit-equal to ``nets.instnorm_spade``) and keeps the
    planes' mean and rstd; differentiable in x and gamma_beta."""
    _check("instnorm_spade_train", {"x": x, "gamma_beta": gamma_beta})
    if x.dim() != 4 or min(x.shape) < 1 or x.shape[2] * x.shape[3] < 4:
        raise ValueError(f"instnorm_spade_train: x [N,C,H,W] with planes of at least 2 x 2 required, got {tuple(x.shape)}")
    N, C, H, W = x.shape
    if tuple(gamma_beta.shape) != (N, 2 * C, H, W):
        raise ValueError(f"instnorm_spade_train: gamma_beta {tuple(gamma_beta.shape)}, expected {(N, 2 * C, H, W)}")
    return _InstNormSpade.apply(x, gamma_beta, float(eps))


# ---------------------------------------------------------------------------------------------- up-sampling + concatenation

class _Upsample2xConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, nearest_channel, relu):
        N, Ca, H, W = a.shape
        Cb = 0 if b is None else b.shape[1]
        out = a.new_empty(N, Ca + Cb, 2 * H, 2 * W)
        call("slr_upsample2x_concat", a.device, a, Ca, b, Cb, out, N, H, W, nearest_channel, relu)
        # RELU_BEFORE gates by the sources, RELU_AFTER by the result (which the next convolution keeps as its input anyway)
        ctx.save_for_backward(a if relu == RELU_BEFORE else None, b if relu == RELU_BEFORE else None, out if relu == RELU_AFTER else None)
        ctx.cfg = (tuple(a.shape), Cb, nearest_channel, relu)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, out = ctx.saved_tensors
        (N, Ca, H, W), Cb, nearest_channel, relu = ctx.cfg
        g = g.contiguous()
        require_device(g)
        ga = g.new_empty(N, Ca, H, W)
        gb = g.new_empty(N, Cb, H, W) if Cb else None
        call("slr_upsample2x_concat_backward", g.device, g, out, a, Ca, b, Cb, ga, gb, N, H, W, nearest_channel, relu)
        return ga, gb, None, None


def upsample2x_concat_train(a, b=None, nearest_channel=-1, relu=RELU_NONE):
    """``nets.upsample2x_concat``, differentiable in a and b: cat(up(a), up(b)) [N,Ca+Cb,2H,2W] with up the bilinear x2 up-sampling
    (align_corners=False) except channel ``nearest_channel`` of EACH source, which is nearest; RELU_BEFORE: up(relu(.)), RELU_AFTER:
    relu(cat(.)); relu'(0) = 0."""
    _check("upsample2x_concat_train", {"a": a, "b": b}, optional=("b",))
    if relu not in (RELU_NONE, RELU_BEFORE, RELU_AFTER):
        raise ValueError(f"upsample2x_concat_train: relu is RELU_NONE, RELU_BEFORE or RELU_AFTER, got {relu!r}")
    if a.dim() != 4 or min(a.shape) < 1:
        raise ValueError(f"upsample2x_concat_train: a [N,Ca,H,W] required, got {tuple(a.shape)}")
    if b is not None and (b.dim() != 4 or b.shape[1] < 1 or (b.shape[0],) + tuple(b.shape[2:]) != (a.shape[0],) + tuple(a.shape[2:])):
        raise ValueError(f"upsample2x_concat_train: b {tuple(b.shape)} does not go with a {tuple(a.shape)}")
    if not isinstance(nearest_channel, int) or isinstance(nearest_channel, bool) or nearest_channel < -1:
        raise ValueError(f"upsample2x_concat_train: nearest_channel is a channel index or -1, got {nearest_channel!r}")
    return _Upsample2xConcat.apply(a, b, int(nearest_channel), int(relu))


# ---------------------------------------------------------------------------------------------- the motion losses

class _MotionLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        N, _, H, W = pred.shape
        sums = torch.empty(N, 3, dtype=torch.float64, device=pred.device)
        ws = _bytes(lib().slr_motion_loss_ws_bytes(N, H, W), pred)
        call("slr_motion_loss", pred.device, pred, gt, sums, N, H, W, ws, ws.numel())
        total = sums.sum(0)                              # (N doubles per term, torch's fixed order)
        epe = (total[0] / (N * H * W)).float()
        l1 = (total[1] / (2 * N * H * W)).float()
        mse = (sums[:, 2] / (H * W)).float()
        ctx.save_for_backward(pred, gt)
        ctx.mark_non_differentiable(mse)
        return epe, l1, mse

    @staticmethod
    @once_differentiable
    def backward(ctx, g_epe, g_l1, _g_mse):
        pred, gt = ctx.saved_tensors
        N, _, H, W = pred.shape
        gpred = torch.empty_like(pred)
        call("slr_motion_loss_grad", pred.device, pred, gt, g_epe.contiguous(), g_l1.contiguous(), gpred, N, H, W)
        return gpred, None


def motion_losses(pred, gt):
    """One pass over pred, gt [N,2,H,W]: ``(EndPointError, MotionL1, mse_err)`` -- mean over pixels of |pred - gt|_2 (synthesis.py:147-160),
    nn.L1Loss (:142-145) as 0-d tensors, and (pred - gt)^2 summed over the channels, averaged per image [N] (the PSNR's mse_err, :119).
    Differentiable in pred through the first two; the EndPointError's gradient is exactly 0 where pred == gt (torch's norm backward)."""
    _check("motion_losses", {"pred": pred, "gt": gt})
    if pred.dim() != 4 or pred.shape[1] != 2 or min(pred.shape) < 1:
        raise ValueError(f"motion_losses: pred [N,2,H,W] required, got {tuple(pred.shape)}")
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"motion_losses: gt {tuple(gt.shape)}, expected {tuple(pred.shape)}")
    return _MotionLosses.apply(pred, gt.detach())


class MotionLoss(nn.Module):
    """MotionLoss (synthesis.py:11-58): ``opts.motion_losses`` is a list of "<lambda>_<name>" with the names MotionL1 and EndPointError.
    forward(pred, gt) returns the reference's dictionary: every named term unscaled and ``Total Loss`` = the sum of EVERY term times its
    lambda, the first included (SynthesisLoss leaves its first term unscaled; MotionLoss does not), in the reference's key order (each
    term's own keys in front of what was there).  ``mse_err`` of the same pass is kept in ``last_mse_err`` for the PSNR."""

    NAMES = ("MotionL1", "EndPointError")

    def __init__(self, opts):
        super().__init__()
        entries = list(opts.motion_losses if hasattr(opts, "motion_losses") else opts["motion_losses"])
        if not entries:
            raise ValueError("MotionLoss: motion_losses is empty")
        self.lambdas, self.loss_names = [], []
        for e in entries:
            parts = str(e).split("_")
            if len(parts) != 2:
                raise ValueError(f"MotionLoss: entry {e!r} is not '<lambda>_<name>'")
            if parts[1] not in self.NAMES:
                raise NotImplementedError(f"MotionLoss: --motion_losses {parts[1]} (MotionL1 and EndPointError are built)")
            self.lambdas.append(float(parts[0]))
            self.loss_names.append(parts[1])
        self.last_mse_err = None

    def forward(self, pred_motion, gt_motion, image=None, mask=None):
        epe, l1, mse = motion_losses(pred_motion, gt_motion)
        self.last_mse_err = mse
        loss_dir = {}
        for lam, name in zip(self.lambdas, self.loss_names):
            err = epe if name == "EndPointError" else l1
            term = {name: err, "Total Loss": err}
            loss_dir["Total Loss"] = loss_dir["Total Loss"] + err * lam if "Total Loss" in loss_dir else err * lam
            loss_dir = dict(term, **loss_dir)            # (what is there overrides the term's own entries)
        return loss_dir


# ---------------------------------------------------------------------------------------------- the network

class _SpectralConv(nn.Module):
    """spectral_norm(nn.Conv2d(cin, cout, k)) as torch leaves it: the parameters ``weight_orig`` and ``bias``, the buffers ``weight_u``
    [cout] and ``weight_v`` [cin k k] (normalised randn).  The network computes 1 / sigma for all its layers at once and hands it in."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.k = k
        self.weight_orig = nn.Parameter(torch.empty(cout, cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.normal_(self.weight_orig, std=math.sqrt(1.0 / (cin * k * k)))
        self.register_buffer("weight_u", F.normalize(torch.randn(cout), dim=0, eps=_spectral.EPS))
        self.register_buffer("weight_v", F.normalize(torch.randn(cin * k * k), dim=0, eps=_spectral.EPS))

    def forward(self, x, sn, leaky=None):
        scale, u, v = sn
        if self.k == 4:
            return conv4x4s2(x, self.weight_orig, self.bias, leaky=leaky, weight_scale=scale, spectral=(u, v))
        return conv3x3(x, self.weight_orig, self.bias, weight_scale=scale, spectral=(u, v))


class TrainableSPADEIN(nn.Module):
    """SPADE(nn.InstanceNorm2d, C, 6) (networks.py:422-463) whose parameters learn: ``mlp_shared`` 6 -> 128 and ``mlp_gb`` 128 -> 2C
    (mlp_gamma's weights, then mlp_beta's: one convolution, as in ``nets.SPADEIN``), plain 3x3 convolutions on ``conv3x3``; the ReLU
    between them is torch's; ``seg`` is the segmap already resized to x's size.  InstanceNorm2d has no state: train() and eval() agree."""

    def __init__(self, C, label_nc=6, nhidden=128):
        super().__init__()
        self.C = C
        self.mlp_shared = TrainableConv3x3(label_nc, nhidden)
        self.mlp_gb = TrainableConv3x3(nhidden, 2 * C)

    def forward(self, x, seg):
        actv = torch.relu(self.mlp_shared(seg))
        return instnorm_spade_train(x, self.mlp_gb(actv))


class TrainableSPADEUnet4MaskMotion(nn.Module):
    """SPADEUnet4MaskMotion (architectures.py:602-743) under --norm_G sync:spectral_batch --motion_norm_G sync:spectral_instance, in
    train() and eval() mode, differentiable in every parameter: conv1..conv8 (4x4 / stride 2 / padding 1, LeakyReLU(0.2) in front of
    conv2..conv8) and dconv1..dconv8 (3x3) carry ``weight_orig`` / ``weight_u`` / ``weight_v`` / ``bias``; SPADE(InstanceNorm2d) after
    conv2..conv7 and dconv1..dconv7 on the network input resized to each level (mask nearest); every x2 up-sampling bilinear except channel
    3 (nearest), ReLU after up-sampling + concatenation except for e8 (ReLU first).  H, W multiples of 256.

    1 / sigma of the 16 spectral layers comes from ONE ``spectral.spectral_sigma`` call per forward (one power iteration in train(), none
    in eval()) for the matrices within its limit of ``spectral.MAX_DIM`` columns -- all 16 up to nf = 21; at nf = 32 conv5..conv8 and
    dconv2..dconv5 (4096 and 4608 columns) take the per-layer power iteration of ``adversarial.spectral_weight``'s expressions instead.
    The sum of the two gradients reaching each e_i (its SPADE successor and its skip) is torch autograd's add."""

    def __init__(self, cin=6, cout=2, nf=32):
        super().__init__()
        if cin != 6:
            raise ValueError(f"TrainableSPADEUnet4MaskMotion: the SPADE segmap is the 6-channel input (RGB, mask, hint); got {cin} channels")
        self.cin = cin
        enc = [cin, nf, nf * 2, nf * 4, nf * 8, nf * 8, nf * 8, nf * 8, nf * 8]
        for i in range(1, 9):
            setattr(self, f"conv{i}", _SpectralConv(enc[i - 1], enc[i], 4))
        dec = [(nf * 8, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 4), (nf * 8, nf * 2),
               (nf * 4, nf), (nf * 2, cout)]
        for k, (ci, co) in enumerate(dec, 1):
            setattr(self, f"dconv{k}", _SpectralConv(ci, co, 3))
        for i, s in _MOTION_ENC_NORM.items():
            setattr(self, f"spade_layer{s}", TrainableSPADEIN(enc[i]))
        for k, s in _MOTION_DEC_NORM.items():
            setattr(self, f"spade_layer{s}", TrainableSPADEIN(dec[k - 1][1]))

    def _spectral_layers(self):
        return [getattr(self, f"conv{i}") for i in range(1, 9)] + [getattr(self, f"dconv{i}") for i in range(1, 9)]

    def _sigmas(self):
        """{layer: (1 / sigma [1], u, v)} of this forward; u and v are the copies its backward uses (the buffers may move again)."""
        layers = self._spectral_layers()
        small = [m for m in layers if m.weight_v.numel() <= _spectral.MAX_DIM and m.weight_u.numel() <= _spectral.MAX_DIM]
        out = {}
        if small:
            inv, su, sv, offs = _spectral.spectral_sigma([m.weight_orig.detach() for m in small], [m.weight_u for m in small],
                                                         [m.weight_v for m in small], training=self.training)
            for j, (m, (uo, vo)) in enumerate(zip(small, offs)):
                out[m] = (inv[j:j + 1], su[uo:uo + m.weight_u.numel()], sv[vo:vo + m.weight_v.numel()])
        for m in layers:
            if m in out:
                continue
            wm, u, v = m.weight_orig.detach().reshape(m.weight_orig.shape[0], -1), m.weight_u, m.weight_v
            with torch.no_grad():
                if self.training:                        # (products and torch's own sums: a fixed order of addition)
                    F.normalize((wm * u.unsqueeze(1)).sum(0), dim=0, eps=_spectral.EPS, out=v)
                    F.normalize((wm * v).sum(1), dim=0, eps=_spectral.EPS, out=u)
                u, v = u.clone(), v.clone()
                out[m] = ((1.0 / (u * (wm * v).sum(1)).sum()).reshape(1), u, v)
        return out

    def forward(self, x):
        _check("TrainableSPADEUnet4MaskMotion", {"input": x})
        _check_motion_grid(x)
        if x.dim() != 4 or x.shape[1] != self.cin:
            raise ValueError(f"TrainableSPADEUnet4MaskMotion: input [N, {self.cin}, H, W] expected, got {tuple(x.shape)}")
        sn = self._sigmas()
        with torch.no_grad():
            seg = {k: resize_segmap(x, k) for k in range(1, 8)}            # once per forward, every level; input only: no gradient
        e = [self.conv1(x, sn[self.conv1])]
        for i in range(2, 8):
            conv = getattr(self, f"conv{i}")
            e.append(getattr(self, f"spade_layer{_MOTION_ENC_NORM[i]}")(conv(e[-1], sn[conv], leaky=0.2), seg[i]))
        e.append(self.conv8(e[-1], sn[self.conv8], leaky=0.2))
        d = upsample2x_concat_train(e[7], None, 3, RELU_BEFORE)             # relu(e8), then the mixed up-sampling
        for k in range(1, 8):
            dconv = getattr(self, f"dconv{k}")
            d_ = getattr(self, f"spade_layer{_MOTION_DEC_NORM[k]}")(dconv(d, sn[dconv]), seg[8 - k])
            d = upsample2x_concat_train(d_, e[7 - k], 3, RELU_AFTER)
        return self.dconv8(d, sn[self.dconv8])

    # ---- state dicts in the reference's (unfolded) keys

    def _reference_entries(self):
        """[(reference key, tensor of this module, row slice or None)] -- mlp_gamma / mlp_beta are the halves of mlp_gb."""
        ent = []
        for name in [f"conv{i}" for i in range(1, 9)] + [f"dconv{i}" for i in range(1, 9)]:
            m = getattr(self, name)
            ent += [(f"{name}.bias", m.bias, None), (f"{name}.weight_orig", m.weight_orig, None), (f"{name}.weight_u", m.weight_u, None),
                    (f"{name}.weight_v", m.weight_v, None)]
        for s in list(_MOTION_ENC_NORM.values()) + list(_MOTION_DEC_NORM.values()):
            sp = getattr(self, f"spade_layer{s}")
            C = sp.C
            for leaf, t in (("weight", "weight"), ("bias", "bias")):
                ent.append((f"spade_layer{s}.mlp_shared.0.{leaf}", getattr(sp.mlp_shared, t), None))
                ent.append((f"spade_layer{s}.mlp_gamma.{leaf}", getattr(sp.mlp_gb, t), slice(0, C)))
                ent.append((f"spade_layer{s}.mlp_beta.{leaf}", getattr(sp.mlp_gb, t), slice(C, 2 * C)))
        return ent

    def reference_state_dict(self, prefix=""):
        """The state dict of the reference's SPADEUnet4MaskMotion under ``prefix`` (copies): what ``nets.load_motion_state_dict`` and the
        reference's own ``load_state_dict`` read."""
        return {prefix + k: (t if sl is None else t[sl]).detach().clone() for k, t, sl in self._reference_entries()}

    @torch.no_grad()
    def load_reference_state_dict(self, sd, prefix=""):
        """Fill the network from the reference's state dict under ``prefix``.  Strict in both directions -- every key under the prefix is
        consumed, every tensor of the network found, every shape equal -- and all of it is checked before anything is copied."""
        sub = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        if not sub:
            raise KeyError(f"no key of the state dict starts with {prefix!r}")
        ent = self._reference_entries()
        missing = sorted(k for k, _, _ in ent if k not in sub)
        if missing:
            raise KeyError(f"TrainableSPADEUnet4MaskMotion: {len(missing)} key(s) missing under {prefix!r}: {missing[:6]}")
        left = sorted(set(sub) - {k for k, _, _ in ent})
        if left:
            raise KeyError(f"TrainableSPADEUnet4MaskMotion: {len(left)} key(s) under {prefix!r} not consumed (another norm / architecture?): "
                           f"{left[:6]}")
        for k, t, sl in ent:
            want = tuple((t if sl is None else t[sl]).shape)
            if not torch.is_tensor(sub[k]) or tuple(sub[k].shape) != want:
                raise ValueError(f"{prefix}{k}: {tuple(getattr(sub[k], 'shape', ()))}, the network expects {want}")
        for k, t, sl in ent:
            (t if sl is None else t[sl]).copy_(sub[k])
        return self


class MotionTrainingModel(nn.Module):
    """SPADEUnetMaskMotion (models/unet_motion.py:111-191) for training: ``forward(batch)`` returns ``(loss_dict, pred_dict)``.

    batch: ``images`` [[B,3,W,W], ...], ``motions`` [B,2,W,W] (or flat), ``hints`` [B,2,W,W] (or flat), on the device.  The moving-region
    mask is 1 where the speed |motion|_2 reaches 0.1 x its per-sample mean; the network sees cat(image, mask, hint); the losses are taken on
    pred * div_flow (MotionLoss), ``PSNR_motion`` from the same pass; pred_dict holds PredMotion (before div_flow, as the reference's),
    GTMotion, InputImg, MovingMask, HintMotion.  ``forward_flow(image, gt_mask, gt_hint)`` returns {"PredMotion": pred * div_flow}.
    The mask and the PSNR's logarithm are a few torch operators on [B,1,W,W] and [B] tensors.

    Options this class does not take raise NotImplementedError naming the flag."""

    def __init__(self, opts, nf=32):
        super().__init__()
        get = lambda k, d=None: getattr(opts, k, d) if not isinstance(opts, dict) else opts.get(k, d)   # noqa: E731
        if not get("use_mask_as_motion_input", False):
            raise NotImplementedError("MotionTrainingModel: --use_mask_as_motion_input is required (the SPADE segmap is image, mask, hint)")
        if not get("use_hint_as_motion_input", False):
            raise NotImplementedError("MotionTrainingModel: --use_hint_as_motion_input is required (the SPADE segmap is image, mask, hint)")
        norm = get("motion_norm_G", "sync:spectral_instance")
        if ":" not in norm or norm.split(":")[1] != "spectral_instance":
            raise NotImplementedError(f"MotionTrainingModel: --motion_norm_G {norm} (sync:spectral_instance is built)")
        self.div_flow = float(get("div_flow", 20.0))
        self.W = int(get("W", 256))
        self.motionH, self.motionW = int(get("motionH", self.W)), int(get("motionW", self.W))
        self.motion_predictor = TrainableSPADEUnet4MaskMotion(6, 2, nf)
        self.loss_function = MotionLoss(opts)

    def forward(self, batch):
        image, gt_motion = batch["images"][0], batch["motions"]
        bs = image.shape[0]
        if gt_motion.dim() <= 3:
            gt_motion = gt_motion.view(bs, -1, self.motionH, self.motionW)
        if gt_motion.shape[1] == 3:
            raise NotImplementedError("MotionTrainingModel: 3-channel (u, v, m) motion (uvm) is not built; [B,2,H,W] motions are")
        _check("MotionTrainingModel", {"images[0]": image, "motions": gt_motion, "hints": batch["hints"]})
        with torch.no_grad():
            speed = (gt_motion[:, 0:1] ** 2 + gt_motion[:, 1:2] ** 2).sqrt().view(bs, 1, self.W, self.W)
            moving_region_mask = 1.0 - (speed < speed.mean([1, 2, 3], True) * 0.1).float()
        hint = batch["hints"].view(bs, 2, moving_region_mask.shape[2], moving_region_mask.shape[3])
        pred_motion = self.motion_predictor(torch.cat([image, moving_region_mask, hint], 1))
        loss = self.loss_function(pred_motion * self.div_flow, gt_motion.contiguous(), image)
        loss["PSNR_motion"] = (10 * (1 / self.loss_function.last_mse_err).log10()).mean()
        return loss, {"PredMotion": pred_motion, "GTMotion": gt_motion, "InputImg": image, "MovingMask": moving_region_mask,
                      "HintMotion": hint}

    def forward_flow(self, image, gt_mask=None, gt_hint=None):
        if gt_mask is None or gt_hint is None:
            raise NotImplementedError("MotionTrainingModel.forward_flow: the mask and the hint are required (--use_mask_as_motion_input "
                                      "--use_hint_as_motion_input)")
        return {"PredMotion": self.motion_predictor(torch.cat([image, gt_mask, gt_hint], 1)) * self.div_flow}
