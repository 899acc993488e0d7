"""The generator loss of the reference's training step on this package's kernels -- drop-ins for models/losses/synthesis.py:
``SynthesisLoss`` (:61-109) with ``L1LossWrapper`` (:134-140), ``PerceptualLoss`` (:166-185) on a frozen VGG19 cut at relu1_1 ... relu5_1
(models/networks/architectures.py:82-115), ``PSNR`` (:113-122) and ``SSIM`` (:125-130).

The two differentiable terms are one ``torch.autograd.Function`` each.  The VGG19 runs its 13 convolutions on the fp32 rung of
csrc/conv.hip with channel-blocked features, like ``metrics.PerceptualVGG16``; its backward runs the 13 backward-data convolutions on the
SAME kernels (3x3 / stride 1 / pad 1: the convolution with ``w.flip(2, 3).transpose(0, 1)``), and the distances, their gradients, the
ReLU gates and the pooling backward on csrc/loss.hip.  The VGG is frozen: there is no weight gradient, and none for the ground truth.
Images are used as given (the reference does not normalise them: its generators end in tanh, [-1, 1]).  Device tensors only: CPU
tensors raise, there is no fallback.  Nothing here synchronises the host; results have the same bits from run to run."""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, metrics, nets

VGG19_CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)            # torchvision vgg19().features indices of the convolutions
VGG19_CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
VGG19_POOLS = (2, 4, 8, 12)              # convolutions (positions in VGG19_CONVS) with ReLU + MaxPool2d(2, 2) in front (features 4, 9, 18, 27)
VGG19_SLICE_ENDS = (0, 2, 4, 8, 12)      # ... whose ReLU'd output is relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 (architectures.py:93-102)
PERCEPTUAL_WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)          # synthesis.py:173


def _image_pair(pred_img, gt_img, what):
    """(N, C, H, W) of a (prediction, ground truth) pair: float32 [N,C,H,W], contiguous, on one device -- checked before the device is
    touched."""
    for t in (pred_img, gt_img):
        if not torch.is_tensor(t):
            raise TypeError(f"slr_sfs_amd.losses.{what}: tensors required, got {type(t).__name__}")
    for t in (pred_img, gt_img):                         # (the reference raises NotImplementedError for CPU tensors, softsplat.py:418-419)
        if not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd.losses run on ROCm device tensors only (no CPU path)")
    for t in (pred_img, gt_img):
        if t.dtype != torch.float32:
            raise TypeError(f"slr_sfs_amd.losses.{what}: float32 tensors required, got {t.dtype}")
    if pred_img.dim() != 4 or min(pred_img.shape) < 1:
        raise ValueError(f"{what}: images [N,C,H,W] with N, C, H, W >= 1 required, got {tuple(pred_img.shape)}")
    if pred_img.shape != gt_img.shape or pred_img.device != gt_img.device:
        raise ValueError(f"{what}: prediction {tuple(pred_img.shape)} on {pred_img.device} and ground truth {tuple(gt_img.shape)} on "
                         f"{gt_img.device} do not match")
    if not (pred_img.is_contiguous() and gt_img.is_contiguous()):
        raise ValueError(f"{what}: images must be contiguous")
    return tuple(pred_img.shape)


def _sum_ws(like, N, C, H, W):
    return torch.empty(_lib.lib().slr_loss_ws_bytes(N, C, H, W), dtype=torch.uint8, device=like.device)


# ---------------------------------------------------------------------------------------------- L1

class _L1(torch.autograd.Function):
    """mean |pred - gt| (slr_l1_loss_grad); backward: sign(pred - gt) * ((1 / count) * dL) from the same kernel, dL read on the device."""

    @staticmethod
    def forward(ctx, pred, gt):
        N, C, H, W = pred.shape
        loss = pred.new_empty(1)
        ws = _sum_ws(pred, N, C, H, W)
        _lib.call("slr_l1_loss_grad", pred.device, pred, gt, loss, None, 0.0, None, N, C, H, W, ws, ws.numel())
        ctx.save_for_backward(pred, gt)
        return loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, dL):
        pred, gt = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        dL = dL.contiguous()
        _lib.require_device(dL)
        grad = torch.empty_like(pred)
        _lib.call("slr_l1_loss_grad", pred.device, pred, gt, None, grad, 1.0 / pred.numel(), dL, *pred.shape, None, 0)
        return grad, None


def l1_loss(pred_img, gt_img):
    """nn.L1Loss()(pred_img, gt_img) for float32 [N,C,H,W] device tensors, differentiable in ``pred_img`` (``gt_img`` gets none)."""
    _image_pair(pred_img, gt_img, "l1_loss")
    return _L1.apply(pred_img, gt_img.detach())


class L1LossWrapper(nn.Module):
    """models/losses/synthesis.py:134-140."""

    def __init__(self, subname=""):
        super().__init__()
        self.subname = subname

    def forward(self, pred_img, gt_img):
        err = l1_loss(pred_img, gt_img)
        return {"L1" + self.subname: err, "Total Loss": err}


# ---------------------------------------------------------------------------------------------- VGG19

class VGG19Features(nn.Module):
    """The frozen VGG19 of PerceptualLoss (architectures.py:82-115): the 13 convolutions of torchvision's vgg19().features[:30], and for
    each the convolution that takes a gradient back through it (``backward_conv``).  Built like ``metrics.PerceptualVGG16``: activations
    are kept RAW (pre-ReLU) and channel-blocked; the ReLU is applied by the consumer -- the next convolution's prologue, the pooling
    kernel, the distance kernel.  Weights: a torchvision-format VGG19 state dict (``from_file`` / ``load_vgg19_state_dict``); nothing
    is downloaded.  The input is used as given."""

    def __init__(self):
        super().__init__()
        ch = VGG19_CHANNELS
        self.convs = nn.ModuleList(nets.Conv(ch[k], ch[k + 1], 3) for k in range(13))
        self.bwd = nn.ModuleList(nets.Conv(ch[k + 1], ch[k], 3, bias=False) for k in range(13))     # weights: backward_conv
        self.register_buffer("_ones", torch.ones(max(ch)), persistent=False)
        self.register_buffer("_zeros", torch.zeros(max(ch)), persistent=False)

    @classmethod
    def from_file(cls, path, device=None):
        """A torchvision VGG19 state dict file (vgg19-*.pth: classifier.* and features.30+ are ignored) -> the module (on ``device``)."""
        net = load_vgg19_state_dict(cls(), torch.load(path, map_location="cpu", weights_only=True))
        return net.to(device) if device is not None else net

    def backward_conv(self, k):
        """The backward-data convolution of convolution ``k``: a ``nets.Conv`` holding ``w.flip(2, 3).transpose(0, 1)``, written when the
        weights are loaded and again only if the forward weight has changed since (another device, an in-place update)."""
        conv, bconv = self.convs[k], self.bwd[k]

        def make():
            with torch.no_grad():
                bconv.weight.copy_(conv.weight.flip(2, 3).transpose(0, 1))
            return True
        nets._cached(bconv, "_flipped", make, conv.weight)                      # (the two move between devices together)
        return bconv

    def check_input(self, H, W):
        if min(H, W) < 16:
            raise ValueError(f"the VGG19 features need H, W >= 16 (four 2x2 poolings), got {H} x {W}")

    def features(self, x, every=False, pred=None):
        """Raw (pre-ReLU) activations of x [B,3,H,W] (NCHW), channel-blocked: the five slice ends conv1_1, conv2_1, conv3_1, conv4_1,
        conv5_1, or with ``every`` all 13 convolutions' outputs (what the backward needs); with ``pred`` = N the eight that end no slice
        are copies of their first N images, [N,C,H,W], so that the other half is not kept alive."""
        acts, h = [], x
        with torch.no_grad(), nets.fp32_kernels(winograd=False):
            for k, conv in enumerate(self.convs):
                relu = None
                if k in VGG19_POOLS:
                    h = metrics.relu_maxpool2x2(h)                            # (ReLU'd already)
                elif k:
                    relu = (self._ones[:conv.cin], self._zeros[:conv.cin])
                h = conv.conv(h, conv.bias, relu, layout=nets.OUT_B8 | (nets.IN_B8 if k else 0))
                if k in VGG19_SLICE_ENDS:
                    acts.append(h)
                elif every:                                                   # (a copy of the half the backward needs: the batch's tensor is freed)
                    acts.append(h if pred is None else h[:pred].clone())
        return acts


@torch.no_grad()
def load_vgg19_state_dict(net, sd):
    """Fill a VGG19Features from a torchvision VGG19 state dict: features.{0,2,5,...,28}.{weight,bias}.  classifier.* and features.30+
    (a full vgg19-*.pth) are ignored; a missing or misshaped key, or any other key, raises."""
    used = set()
    for k, idx in enumerate(VGG19_CONVS):
        conv = net.convs[k]
        for name, p in (("weight", conv.weight), ("bias", conv.bias)):
            key = f"features.{idx}.{name}"
            if key not in sd:
                raise KeyError(f"VGG19 state dict: {key} is missing")
            v = sd[key]
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"VGG19 state dict: {key} has shape {tuple(v.shape)}, expected {tuple(p.shape)}")
            p.copy_(v)
            used.add(key)
        net.backward_conv(k)

    def ignored(key):
        parts = key.split(".")
        return parts[0] == "classifier" or (parts[0] == "features" and len(parts) > 1 and parts[1].isdigit() and int(parts[1]) >= 30)
    left = sorted(k for k in sd if k not in used and not ignored(k))
    if left:
        raise ValueError(f"VGG19 state dict: unexpected keys {left[:8]}")
    return net


# ---------------------------------------------------------------------------------------------- perceptual loss

def _gate(a, b, g_in, total, g_out, coef, gscale, ws):
    N, C, H, W = a.shape
    _lib.call("slr_feature_l1_gate_b8", a.device, a, b, g_in, total, g_out, coef, gscale, N, C, H, W, ws, 0 if ws is None else ws.numel())


def _perceptual_forward(vgg, pred_img, gt_img, every):
    """(distances, activations): the five mean |relu(a_s(pred)) - relu(a_s(gt))| as a float32 [5] device tensor, and the raw activations
    (channel-blocked; index [:N] is the prediction's half): with ``every`` all 13 -- the five slice ends of the batch [pred; gt],
    [2N,C,H,W], the other eight of the prediction alone, [N,C,H,W] -- else the five slice ends."""
    N, _, H, W = pred_img.shape
    x = pred_img.new_empty(2 * N, 3, H, W)
    x[:N].copy_(pred_img)
    x[N:].copy_(gt_img)
    acts = vgg.features(x, every, N)
    ends = [acts[k] for k in VGG19_SLICE_ENDS] if every else acts
    sums = pred_img.new_empty(5)
    ws = _sum_ws(pred_img, N, *ends[0].shape[1:])                             # (the largest slice; the five passes follow each other on the stream)
    for s, f in enumerate(ends):
        _gate(f[:N], f[N:], None, sums[s:s + 1], None, 0.0, None, ws)
    return torch.cat([sums[s:s + 1] / float(f[:N].numel()) for s, f in enumerate(ends)]), acts


def _weighted(dists):
    loss = 0                                                                  # synthesis.py:181-183, in its order
    for s in range(5):
        loss = loss + PERCEPTUAL_WEIGHTS[s] * dists[s]
    return loss


class _Perceptual(torch.autograd.Function):
    """forward(pred, gt, vgg) -> (loss, distances [5]); saved, only when pred needs a gradient: the prediction's 13 raw activations and
    the ground truth's five slice features (the slice ends as views of the batch's tensors, the other eight as copies of their half).  backward walks the layers in reverse: gate / seed kernel -> backward-data convolution ->
    pooling backward, the incoming dL a device scalar throughout."""

    @staticmethod
    def forward(ctx, pred, gt, vgg):
        N = pred.shape[0]
        keep = bool(ctx.needs_input_grad[0])
        dists, acts = _perceptual_forward(vgg, pred, gt, keep)
        if keep:
            ctx.save_for_backward(*[a[:N] for a in acts], *[acts[k][N:] for k in VGG19_SLICE_ENDS])
            ctx.vgg = vgg
        ctx.mark_non_differentiable(dists)
        return _weighted(dists), dists

    @staticmethod
    @once_differentiable
    def backward(ctx, dL, _d_dists):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        saved, vgg = ctx.saved_tensors, ctx.vgg
        a_pred, b_gt = saved[:13], saved[13:]
        dL = dL.contiguous()
        _lib.require_device(dL)
        g = None                                                              # the gradient at the (ReLU'd, pooled) input of convolution k + 1
        with nets.fp32_kernels(winograd=False):
            for k in range(12, -1, -1):
                a = a_pred[k]
                if k in VGG19_SLICE_ENDS:                                     # seed of the slice's distance + what came from above, gated
                    s = VGG19_SLICE_ENDS.index(k)
                    ga = torch.empty_like(a)
                    _gate(a, b_gt[s], g, None, ga, PERCEPTUAL_WEIGHTS[s] / a.numel(), dL, None)
                elif k + 1 in VGG19_POOLS:                                    # ReLU + pooling in one backward
                    ga = torch.empty_like(a)
                    _lib.call("slr_relu_maxpool2x2_backward_b8", a.device, a, g, ga, *a.shape)
                else:                                                         # plain ReLU backward
                    ga = torch.empty_like(a)
                    _gate(a, None, g, None, ga, 0.0, None, None)
                g = vgg.backward_conv(k).conv(ga, None, None, layout=nets.IN_B8 | (nets.OUT_B8 if k else 0))
        return g, None, None


def perceptual_loss(vgg, pred_img, gt_img, return_distances=False):
    """sum_s w_s mean |relu(a_s(pred)) - relu(a_s(gt))| over the five slices (w = 1/32, 1/16, 1/8, 1/4, 1), differentiable in
    ``pred_img``; with ``return_distances`` also the five means (float32 [5], no gradient)."""
    _, C, H, W = _image_pair(pred_img, gt_img, "perceptual_loss")
    if C != 3:
        raise ValueError(f"the perceptual loss takes RGB images, got {C} channels")
    vgg.check_input(H, W)
    loss, dists = _Perceptual.apply(pred_img, gt_img.detach(), vgg)
    return (loss, dists) if return_distances else loss


class PerceptualLoss(nn.Module):
    """models/losses/synthesis.py:166-185 on a ``VGG19Features`` (the reference builds its own from torchvision's download)."""

    def __init__(self, vgg, subname=""):
        super().__init__()
        if not isinstance(vgg, VGG19Features):
            raise TypeError("PerceptualLoss: a VGG19Features is required (VGG19Features.from_file(path))")
        self.model = vgg
        self.weights = list(PERCEPTUAL_WEIGHTS)
        self.subname = subname

    def forward(self, pred_img, gt_img, name="Perceptual"):
        loss = perceptual_loss(self.model, pred_img, gt_img)
        return {"Perceptual" + self.subname: loss, "Total Loss": loss}


# ---------------------------------------------------------------------------------------------- PSNR / SSIM (reported, detached)

def _ssim_mse(pred_img, gt_img):
    """[N,2] per image (SSIM, mean squared error) from ONE pass (slr_ssim_mse).  The pass has no notion of a value range: C1 and C2 are
    the reference's constants (ssim.py:54-55) whatever the images hold, the squared error is that of the values -- right for [-1, 1]."""
    _image_pair(pred_img, gt_img, "PSNR / SSIM")
    return metrics.ssim_mse(pred_img.detach(), gt_img.detach())


class PSNR(nn.Module):
    """models/losses/synthesis.py:113-122: 10 log10(1 / mean_hw sum_c (p - g)^2) per image, averaged over the batch."""

    def __init__(self, subname=""):
        super().__init__()
        self.subname = subname

    def forward(self, pred_img, gt_img, ssim_mse=None):
        sm = _ssim_mse(pred_img, gt_img) if ssim_mse is None else ssim_mse
        mse_err = sm[:, 1] * float(pred_img.shape[1])                         # mean over C, H, W -> sum over C of the mean over H, W
        psnr = 10 * (1 / mse_err).log10()
        return {"psnr" + self.subname: psnr.mean()}


class SSIM(nn.Module):
    """models/losses/synthesis.py:125-130: ssim(pred, gt), the mean of the SSIM map."""

    def __init__(self, subname=""):
        super().__init__()
        self.subname = subname

    def forward(self, pred_img, gt_img, ssim_mse=None):
        sm = _ssim_mse(pred_img, gt_img) if ssim_mse is None else ssim_mse
        return {"ssim" + self.subname: sm[:, 0].mean()}


# ---------------------------------------------------------------------------------------------- SynthesisLoss

class SynthesisLoss(nn.Module):
    """models/losses/synthesis.py:61-109.  ``opt.losses``: "<lambda>_<name>" strings, names l1 and content (the reference's default is
    ['1.0_l1', '10.0_content'], options/train_options.py:390); PSNR and SSIM are always appended and share one pass.  ``vgg``: the
    VGG19Features of the content term (may be None without one).  As in the reference the FIRST loss's "Total Loss" enters unweighted
    (its lambda is ignored, :105) and the later ones times their lambda."""

    def __init__(self, opt, vgg=None, subname=""):
        super().__init__()
        self.opt = opt
        self.subname = subname
        lambdas, loss_names = zip(*[l.split("_") for l in opt.losses])
        self.lambdas = [float(l) for l in lambdas]
        self.losses = nn.ModuleList([self.get_loss_from_name(name, vgg) for name in loss_names + ("PSNR", "SSIM")])

    def get_loss_from_name(self, name, vgg):
        if name == "l1":
            return L1LossWrapper(self.subname)
        if name == "content":
            if vgg is None:
                raise ValueError("SynthesisLoss: the content loss needs a VGG19Features (vgg=VGG19Features.from_file(path))")
            return PerceptualLoss(vgg, self.subname)
        if name == "PSNR":
            return PSNR(self.subname)
        if name == "SSIM":
            return SSIM(self.subname)
        if name == "style":
            raise NotImplementedError("SynthesisLoss: the style loss (StyleLoss, synthesis.py:187-233) is not implemented on this package's kernels")
        raise ValueError(f"SynthesisLoss: unknown loss {name!r} (l1, content)")

    def forward(self, pred_img, gt_img):
        _image_pair(pred_img, gt_img, "SynthesisLoss")
        sm = _ssim_mse(pred_img, gt_img)
        losses = [loss(pred_img, gt_img, sm) if isinstance(loss, (PSNR, SSIM)) else loss(pred_img, gt_img) for loss in self.losses]
        loss_dir = {}
        for i, l in enumerate(losses):                                        # synthesis.py:96-109, literally
            if "Total Loss" in l.keys():
                if "Total Loss" in loss_dir.keys():
                    loss_dir["Total Loss"] = loss_dir["Total Loss"] + l["Total Loss"] * self.lambdas[i]
                else:
                    loss_dir["Total Loss"] = l["Total Loss"]
            loss_dir = dict(l, **loss_dir)                                    # (loss_dir overrides l)
        return loss_dir
