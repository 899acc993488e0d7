"""The adversarial loss of the reference's trainer (models/base_model.py:15-30, 118-151: --discriminator_losses pix2pixHD --gan_mode hinge
--norm_D spectralinstance): the multiscale PatchGAN discriminator (models/networks/discriminators.py), its hinge and feature-matching
losses (models/losses/gan_loss.py) and both training steps, differentiable in the fake image and in every parameter.

The 4x4 convolutions and the instance norm + LeakyReLU run on csrc/disc.hip in both directions (``conv4x4``, ``instnorm_lrelu``); the
feature-matching L1 terms on ``slr_l1_loss_grad``.  The 3-channel counted average pool between the two scales, the power iteration and
sigma of the spectral normalisation, the hinge means on the final maps and the adds of the loss terms are torch operators on tensors of
under 1 MB.  Nothing synchronises host and device; every result has the same bits from run to run.  There is no fallback: CPU tensors
raise, a missing library raises.  DESIGN 3.12.

Not here: AlphaDiscriminatorLoss, the pix2pixHDorigin variant, --norm_D other than spectralinstance, the optimiser.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from ._lib import call, lib, require_device
from .losses import l1_loss

SLOPE = 0.2


def _bytes(n, like):
    return torch.empty(int(n), dtype=torch.uint8, device=like.device)


def _prepared(weight, scale, stride, backward):
    """The MFMA fragment buffer of ``weight`` [Cout,Cin,4,4], every weight times the device scalar ``scale`` (or 1)."""
    cout, cin = weight.shape[:2]
    buf = _bytes(lib().slr_conv4x4_weight_bytes(cout, cin, backward), weight)
    call("slr_conv4x4_f32_weights", weight.device, weight, scale, buf, cout, cin, stride, backward)
    return buf


class _Conv4x4(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, scale, stride, leaky, splits):
        N, cin, H, W = x.shape
        cout = weight.shape[0]
        out = x.new_empty(N, cout, H // stride + 1, W // stride + 1)
        call("slr_conv4x4_forward", x.device, x, _prepared(weight, scale, stride, 0), bias, out, N, cin, cout, H, W, stride, int(leaky), SLOPE)
        ctx.save_for_backward(x, weight, scale, out if leaky else None)
        ctx.cfg = (stride, bias is not None, splits)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight, scale, gate = ctx.saved_tensors
        stride, has_bias, splits = ctx.cfg
        g = g.contiguous()
        require_device(g)
        N, cin, H, W = x.shape
        cout = weight.shape[0]
        need_x, need_w, need_b, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2], \
            scale is not None and ctx.needs_input_grad[3]
        gx = gw = gb = gs = None
        if need_x:
            gx = torch.empty_like(x)
            call("slr_conv4x4_backward_data", x.device, g, gate, _prepared(weight, scale, stride, 1), gx, N, cin, cout, H, W, stride, SLOPE)
        if need_w or need_b or need_s:
            dw = torch.empty_like(weight)                # the gradient at the effective weight, weight * scale
            gb = x.new_empty(cout) if need_b else None
            ws = _bytes(lib().slr_conv4x4_grad_ws_bytes(N, cin, cout, H, W, stride, splits), x)
            call("slr_conv4x4_weight_grad", x.device, x, g, gate, dw, gb, N, cin, cout, H, W, stride, SLOPE, splits, ws, ws.numel())
            if need_w:
                gw = dw if scale is None else dw * scale
            if need_s:
                gs = (dw * weight).sum().reshape(scale.shape)
        return gx, gw, gb, gs, None, None, None


def _check(name, x, *others):
    for t in (x,) + others:
        if t is not None and not torch.is_tensor(t):
            raise TypeError(f"slr_sfs_amd.{name}: tensors required, got {type(t).__name__}")
    for t in (x,) + others:
        if t is not None and not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd operators run on ROCm device tensors only (no CPU path)")
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{name}: input [N,C,H,W] with N, C, H, W >= 1 required, got {tuple(x.shape)}")
    for t in (x,) + others:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: tensors must be contiguous")
    require_device(x, *others)


def conv4x4(x, weight, bias=None, *, stride, leaky=False, weight_scale=None, _splits=0):
    """conv2d(x, weight * weight_scale, bias, stride, padding 2) for a 4x4 ``weight`` [Cout,Cin,4,4] and stride 1 or 2, with
    leaky_relu(., 0.2) of the result if ``leaky`` (its backward gate is the output's sign).  ``weight_scale``: a one-element device tensor
    (the 1 / sigma of ``spectral_weight``) folded into the weight preparation.  Differentiable in x, weight, bias and weight_scale; a
    gradient whose input does not require it is not computed."""
    if stride not in (1, 2):
        raise ValueError(f"conv4x4: stride 1 or 2, got {stride}")
    _check("conv4x4", x, weight, bias, weight_scale)
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 4, 4):
        raise ValueError(f"conv4x4: weight {tuple(weight.shape)}, expected [Cout,{x.shape[1]},4,4]")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"conv4x4: bias {tuple(bias.shape)}, expected ({weight.shape[0]},)")
    if weight_scale is not None and weight_scale.numel() != 1:
        raise ValueError("conv4x4: weight_scale is a one-element tensor")
    return _Conv4x4.apply(x, weight, bias, weight_scale, int(stride), bool(leaky), int(_splits))


class _InstNormLRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, slope):
        N, C, H, W = x.shape
        y, mean, rstd = torch.empty_like(x), x.new_empty(N * C), x.new_empty(N * C)
        call("slr_instnorm_lrelu_forward", x.device, x, y, mean, rstd, N, C, H, W, eps, slope)
        ctx.save_for_backward(x, mean, rstd)
        ctx.slope = slope
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, mean, rstd = ctx.saved_tensors
        gy = gy.contiguous()
        require_device(gy)
        gx = torch.empty_like(x)
        call("slr_instnorm_lrelu_backward", x.device, x, gy, mean, rstd, gx, *x.shape, ctx.slope)
        return gx, None, None


def instnorm_lrelu(x, eps=1e-5, slope=0.2):
    """leaky_relu(InstanceNorm2d(affine=False, eps)(x), slope) for planes of at least 2 x 2, differentiable in x."""
    _check("instnorm_lrelu", x)
    if x.shape[2] * x.shape[3] < 4:
        raise ValueError(f"instnorm_lrelu: planes of at least 2 x 2, got {tuple(x.shape)}")
    return _InstNormLRelu.apply(x, float(eps), float(slope))


def spectral_weight(weight_orig, u, v, training):
    """1 / sigma of torch.nn.utils.spectral_norm (one power iteration, eps 1e-12) as a one-element tensor on the weight's device.  In
    training mode u and v are first updated in place, without gradient: v <- normalize(Wm^T u), u <- normalize(Wm v), Wm = weight_orig as
    [Cout, 16 Cin].  sigma = u^T Wm v with u, v constants of the gradient, so that with W = weight_orig / sigma the gradient reaching
    weight_orig through ``conv4x4(..., weight_scale=1 / sigma)`` is (dW - <dW, W> u v^T) / sigma."""
    wm = weight_orig.reshape(weight_orig.shape[0], -1)
    if training:
        with torch.no_grad():                            # (products and torch's own sums rather than a BLAS call: a fixed order of addition)
            F.normalize((wm * u.unsqueeze(1)).sum(0), dim=0, eps=1e-12, out=v)
            F.normalize((wm * v).sum(1), dim=0, eps=1e-12, out=u)
        u, v = u.clone(), v.clone()                      # (the buffers may move again before this forward's backward runs)
    return (1.0 / (u * (wm * v).sum(1)).sum()).reshape(1)


class _Conv4x4Layer(nn.Module):
    """nn.Conv2d(cin, cout, 4, stride, 2) with a bias: state-dict keys ``weight``, ``bias``."""

    def __init__(self, cin, cout, stride, leaky):
        super().__init__()
        self.stride, self.leaky = stride, leaky
        self.weight = nn.Parameter(torch.empty(cout, cin, 4, 4))
        self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.xavier_normal_(self.weight, gain=0.02)   # define_D: init_weights("xavier", 0.02), biases 0

    def forward(self, x):
        return conv4x4(x, self.weight, self.bias, stride=self.stride, leaky=self.leaky)


class _SpectralConv4x4(nn.Module):
    """spectral_norm(nn.Conv2d(cin, cout, 4, stride, 2)) without bias: state-dict keys ``weight_orig``, ``weight_u``, ``weight_v``."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.stride = stride
        self.weight_orig = nn.Parameter(torch.empty(cout, cin, 4, 4))
        nn.init.xavier_normal_(self.weight_orig, gain=0.02)
        self.register_buffer("weight_u", F.normalize(torch.randn(cout), dim=0, eps=1e-12))
        self.register_buffer("weight_v", F.normalize(torch.randn(cin * 16), dim=0, eps=1e-12))

    def scale(self):
        return spectral_weight(self.weight_orig, self.weight_u, self.weight_v, self.training)

    def forward(self, x):
        return conv4x4(x, self.weight_orig, None, stride=self.stride, weight_scale=self.scale())


class TrainableNLayerDiscriminator(nn.Module):
    """NLayerDiscriminator (discriminators.py:78-139; n_layers_D = 4, norm_D = spectralinstance) with its module and state-dict names:
    ``model0.0.{weight,bias}``, ``model{1,2,3}.0.0.{weight_orig,weight_u,weight_v}``, ``model4.0.{weight,bias}``.  forward returns the
    five outputs (no_ganFeat_loss = False)."""

    def __init__(self, ndf=64, output_nc=3):
        super().__init__()
        nf = ndf
        self.model0 = nn.Sequential(_Conv4x4Layer(output_nc, nf, 2, True))
        for n in (1, 2, 3):
            prev, nf = nf, min(nf * 2, 512)
            self.add_module(f"model{n}", nn.Sequential(nn.Sequential(_SpectralConv4x4(prev, nf, 1 if n == 3 else 2))))
        self.model4 = nn.Sequential(_Conv4x4Layer(nf, 1, 1, False))

    def forward(self, x):
        results = [self.model0[0](x)]
        for n in (1, 2, 3):
            results.append(instnorm_lrelu(getattr(self, f"model{n}")[0][0](results[-1])))
        results.append(self.model4[0](results[-1]))
        return results


class TrainableMultiscaleDiscriminator(nn.Module):
    """MultiscaleDiscriminator (discriminators.py:142-207): num_D = 2 copies, the second on the counted 3x3 / stride 2 average of the
    input.  forward returns [[five outputs] per copy]."""

    def __init__(self, ndf=64, output_nc=3, num_D=2):
        super().__init__()
        for i in range(num_D):
            self.add_module(f"discriminator_{i}", TrainableNLayerDiscriminator(ndf, output_nc))

    def forward(self, x):
        result = []
        for D in self.children():
            result.append(D(x))
            x = F.avg_pool2d(x, kernel_size=3, stride=2, padding=[1, 1], count_include_pad=False).contiguous()
        return result


class GANLoss(nn.Module):
    """gan_loss.py:20-118: ``hinge``, ``ls``, ``original`` and ``w`` on the final maps (a few lines of torch on maps of <= 35 x 35)."""

    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        if gan_mode not in ("ls", "original", "w", "hinge"):
            raise ValueError(f"Unexpected gan_mode {gan_mode}")
        self.gan_mode, self.real_label, self.fake_label = gan_mode, target_real_label, target_fake_label

    def loss(self, p, target_is_real, for_discriminator=True):
        if self.gan_mode == "original":
            return F.binary_cross_entropy_with_logits(p, torch.full_like(p, self.real_label if target_is_real else self.fake_label))
        if self.gan_mode == "ls":
            return F.mse_loss(p, torch.full_like(p, self.real_label if target_is_real else self.fake_label))
        if self.gan_mode == "hinge":
            if for_discriminator:
                return -torch.mean(torch.clamp_max((p if target_is_real else -p) - 1, 0.0))
            assert target_is_real, "The generator's hinge loss must be aiming for real"
            return -torch.mean(p)
        return -p.mean() if target_is_real else p.mean()

    def forward(self, preds, target_is_real, for_discriminator=True):
        if not isinstance(preds, list):
            return self.loss(preds, target_is_real, for_discriminator)
        total = 0
        for p in preds:
            total = total + self.loss(p[-1] if isinstance(p, list) else p, target_is_real, for_discriminator).reshape(1)
        return total / len(preds)


class _BaseDiscriminator(nn.Module):
    """BaseDiscriminator (gan_loss.py:121-246) for name = pix2pixHD."""

    def __init__(self, gan_mode, lambda_feat, no_ganFeat_loss, ndf, output_nc):
        super().__init__()
        self.netD = TrainableMultiscaleDiscriminator(ndf, output_nc)
        self.criterionGAN = GANLoss(gan_mode)
        self.lambda_feat, self.no_ganFeat_loss = lambda_feat, no_ganFeat_loss

    def discriminate(self, fake, real):
        out = self.netD(torch.cat([fake, real], dim=0))
        n = fake.shape[0]
        return [[t[:n] for t in p] for p in out], [[t[n:] for t in p] for p in out]

    def compute_discriminator_loss(self, fake, real):
        pred_fake, pred_real = self.discriminate(fake.detach(), real)
        losses = {"D_Fake": self.criterionGAN(pred_fake, False, for_discriminator=True),
                  "D_real": self.criterionGAN(pred_real, True, for_discriminator=True)}
        losses["Total Loss"] = sum(losses.values()).mean()
        return losses

    def compute_generator_loss(self, fake, real):
        pred_fake, pred_real = self.discriminate(fake, real)
        losses = {"GAN": self.criterionGAN(pred_fake, True, for_discriminator=False)}
        if not self.no_ganFeat_loss:
            num_D = len(pred_fake)
            feat = fake.new_zeros(1)
            for pf, pr in zip(pred_fake, pred_real):
                for a, b in zip(pf[:-1], pr[:-1]):       # (the last output is the final prediction)
                    feat = feat + l1_loss(a, b.detach()) * (self.lambda_feat / num_D)
            losses["GAN_Feat"] = feat
        losses["Total Loss"] = sum(losses.values()).mean()
        return losses

    def forward(self, fake, real, mode="generator"):
        if mode == "generator":
            return self.compute_generator_loss(fake, real)
        if mode == "discriminator":
            return self.compute_discriminator_loss(fake, real)
        raise ValueError(f"mode {mode!r}")


class DiscriminatorLoss(nn.Module):
    """DiscriminatorLoss (gan_loss.py:254-307) with --discriminator_losses pix2pixHD: state-dict keys ``netD.netD.discriminator_*...``, so a
    reference checkpoint's netD loads with ``load_state_dict``.  Both steps return the reference's dictionaries: ``GAN`` / ``GAN_Feat``
    [1] (``D_Fake`` / ``D_real`` [1]) and a 0-d ``Total Loss``.  Every forward in train() mode moves u and v of the spectral layers, as
    the reference's does; a training step runs two."""

    def __init__(self, gan_mode="hinge", lambda_feat=10.0, no_ganFeat_loss=False, ndf=64, output_nc=3):
        super().__init__()
        self.netD = _BaseDiscriminator(gan_mode, lambda_feat, no_ganFeat_loss, ndf, output_nc)

    def run_generator_one_step(self, pred_img, gt_img):
        return self.netD(pred_img, gt_img, mode="generator")

    def run_discriminator_one_step(self, pred_img, gt_img):
        return self.netD(pred_img, gt_img, mode="discriminator")
