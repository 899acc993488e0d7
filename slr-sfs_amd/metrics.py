"""Clip-evaluation metrics on this package's kernels -- drop-ins for the reference's SSIM (models/losses/ssim.py), PSNR and
"Perceptual" VGG16 distance (evaluation/animation/metrics.py; models/networks/pretrained_networks.py: PNet("vgg")), and for the LPIPS of
its evaluation scripts (lpips.LPIPS(net='alex', version='0.1'), evaluation/animation/eval_CLAW.py:24,37).

SSIM and the squared error of PSNR are ONE kernel (csrc/metrics.hip: slr_ssim_mse); the VGG16 of the Perceptual metric runs its 13
convolutions on the fp32 rung of csrc/conv.hip (SLR_CONV_F32: fp32 operands, products and accumulation) with channel-blocked
features, and its input scaling, ReLU + max pooling and feature distance on the kernels of csrc/metrics.hip.  LPIPS runs AlexNet's
11x11 / stride 4 and 5x5 convolutions, its 3x3 / stride 2 max pooling and the LPIPS distance on the kernels of csrc/lpips.hip, and its
three 3x3 convolutions on the same fp32 rung.

Images: float32 [N,C,H,W] in [0, 1] (what the reference's eval scripts pass), or uint8 [N,H,W,3] frames as PNG / video decoders give them
(value v / 255, = ToTensor).  Device tensors only: CPU tensors raise, there is no fallback.  Nothing here synchronises the host."""
import torch
import torch.nn as nn

from . import _lib, nets

VGG16_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)            # torchvision vgg16().features indices of the convolutions
VGG16_CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
VGG16_SLICES = (2, 2, 3, 3, 3)                                            # convolutions per slice: relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
PERCEPTUAL_BYTES = 4 << 30                                                # activation budget of one evaluate_clip batch (see perceptual_batch)
ALEX_CONVS = (0, 3, 6, 8, 10)                                             # torchvision alexnet().features indices of the convolutions
ALEX_CHANNELS = (3, 64, 192, 384, 256, 256)                               # = the channels of relu1 ... relu5 behind the input's 3
LPIPS_MIN_SIZE = 31                                                       # 30 leaves the second 3x3 / stride 2 pooling an empty output
LPIPS_BYTES = 1 << 30                                                     # activation budget of one evaluate_clip batch (see lpips_batch)


def _pair(img1, img2):
    """(u8, N, C, H, W) of an image pair; raises for CPU tensors and anything but the two accepted forms."""
    for t in (img1, img2):
        if not t.is_cuda:
            raise NotImplementedError("slr_sfs_amd.metrics run on ROCm device tensors only (no CPU path)")
    if img1.shape != img2.shape or img1.dtype != img2.dtype or img1.device != img2.device:
        raise ValueError(f"image pair: same shape, dtype and device expected, got {tuple(img1.shape)} {img1.dtype} {img1.device} and "
                         f"{tuple(img2.shape)} {img2.dtype} {img2.device}")
    if not (img1.is_contiguous() and img2.is_contiguous()):
        raise ValueError("images must be contiguous")
    if img1.dim() != 4:
        raise ValueError(f"images: [N,C,H,W] float or [N,H,W,3] uint8, got {tuple(img1.shape)}")
    if img1.dtype == torch.uint8:
        N, H, W, C = img1.shape
        if C != 3:
            raise ValueError(f"uint8 frames: [N,H,W,3], got {tuple(img1.shape)}")
        return 1, N, C, H, W
    if img1.dtype != torch.float32:
        raise TypeError(f"images: float32 in [0, 1] or uint8, got {img1.dtype}")
    N, C, H, W = img1.shape
    return 0, N, C, H, W


def ssim_mse(img1, img2, window_size=11, mask=None):
    """[N,2] float32 on the device: per image (SSIM, mean squared error), with ``mask`` [N,1,H,W] (or [1,1,H,W]) the masked forms of
    ssim.py:61-67 and metrics.py:12-17.  One pass over the inputs (slr_ssim_mse)."""
    u8, N, C, H, W = _pair(img1, img2)
    if mask is not None:
        if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[2:]) != (H, W) or mask.shape[0] not in (1, N):
            raise ValueError(f"mask: [N,1,H,W] = [{N},1,{H},{W}] expected, got {tuple(mask.shape)}")
        mask = mask.expand(N, 1, H, W).contiguous()
        _lib.require_device(mask)
    out = torch.empty(N, 2, device=img1.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().slr_ssim_ws_bytes(N, H, W), dtype=torch.uint8, device=img1.device)
    _lib.call("slr_ssim_mse", img1.device, img1, img2, u8, mask, out, N, C, H, W, int(window_size), ws, ws.numel())
    return out


def ssim(img1, img2, window_size=11, mask=None, size_average=True):
    """models/losses/ssim.py:ssim: per-image SSIM [N] with a mask or size_average=False, their mean (0-d) otherwise."""
    s = ssim_mse(img1, img2, window_size, mask)[:, 0]
    return s if (mask is not None or not size_average) else s.mean()


class SSIM(nn.Module):
    """models/losses/ssim.py:SSIM."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average

    def forward(self, img1, img2, mask=None):
        return ssim(img1, img2, self.window_size, mask, self.size_average)


def ssim_metric(img1, img2, mask=None):
    """evaluation/animation/metrics.py:ssim_metric -- per-image SSIM [N]."""
    return ssim(img1, img2, mask=mask, size_average=False)


def psnr_from_mse(mse):
    return 10 * (1 / mse).log10()                                          # metrics.py:22, in fp32 as there


def psnr(img1, img2, mask=None):
    """evaluation/animation/metrics.py:psnr -- per-image PSNR [N] in dB (the squared error comes out of the fused SSIM pass)."""
    return psnr_from_mse(ssim_mse(img1, img2, 11, mask)[:, 1])


def relu_maxpool2x2(x):
    """nn.ReLU + nn.MaxPool2d(2, 2) of channel-blocked [N,C,H,W] activations (floor mode) -> channel-blocked [N,C,H//2,W//2]."""
    N, C, H, W = x.shape
    out = torch.empty(N, C, H // 2, W // 2, device=x.device, dtype=x.dtype)
    _lib.call("slr_relu_maxpool2x2_b8", x.device, x, out, N, C, H, W)
    return out


def feature_distance(f0, f1):
    """1 - cos_sim(relu(f0), relu(f1)) per image [N] (pretrained_networks.py:11-31, :82): channel-blocked [N,C,H,W] features."""
    N, C, H, W = f0.shape
    out = torch.empty(N, device=f0.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().slr_feature_cos_ws_bytes(N, H, W), dtype=torch.uint8, device=f0.device)
    _lib.call("slr_feature_cos_distance", f0.device, f0, f1, out, N, C, H, W, ws, ws.numel())
    return out


class PerceptualVGG16(nn.Module):
    """PNet("vgg") (pretrained_networks.py:34-93) on this package's kernels: forward(in0, in1) -> [N], the sum over the five slices
    relu1_2 ... relu5_3 of 1 - mean_hw(cos) of the ReLU'd features; retPerLayer=True also returns the five per-slice [N] scores.
    in0 / in1: PNet's own input, float [N,3,H,W] in [-1, 1] (perceptual_sim passes img * 2 - 1; its counterpart here,
    ``perceptual_sim``, takes [0, 1] floats or uint8 frames and does the scaling in the input kernel).  Weights: a torchvision-format VGG16
    state dict (``from_file`` / ``load_vgg16_state_dict``); nothing is downloaded.  Both images run as ONE batch of 2N through the 13
    fp32-rung convolutions; features stay channel-blocked."""

    def __init__(self):
        super().__init__()
        self.convs = nn.ModuleList(nets.Conv(VGG16_CHANNELS[k], VGG16_CHANNELS[k + 1], 3) for k in range(13))
        self.L = len(VGG16_SLICES)
        self.register_buffer("_ones", torch.ones(max(VGG16_CHANNELS)), persistent=False)
        self.register_buffer("_zeros", torch.zeros(max(VGG16_CHANNELS)), persistent=False)

    @classmethod
    def from_file(cls, path, device=None):
        """A torchvision VGG16 state dict file (vgg16-*.pth: classifier.* is ignored) -> the module (on ``device``)."""
        net = load_vgg16_state_dict(cls(), torch.load(path, map_location="cpu", weights_only=True))
        return net.to(device) if device is not None else net

    def features(self, x):
        """The raw (pre-ReLU) outputs of conv1_2, conv2_2, conv3_3, conv4_3, conv5_3 for the prepared input x [B,3,H,W] (NCHW),
        channel-blocked.  The ReLU of each slice is applied by its consumer: the next convolution's prologue (scale 1, shift 0), the
        pooling kernel, the distance kernel."""
        outs, h, k = [], x, 0
        with torch.no_grad(), nets.fp32_kernels(winograd=False):
            for s, n in enumerate(VGG16_SLICES):
                if s:
                    h = relu_maxpool2x2(h)
                for i in range(n):
                    conv = self.convs[k]
                    relu = (self._ones[:conv.cin], self._zeros[:conv.cin]) if i else None    # (after a pool: already ReLU'd)
                    h = conv.conv(h, conv.bias, relu, layout=nets.OUT_B8 | (nets.IN_B8 if k else 0))
                    k += 1
                outs.append(h)
        return outs

    def score(self, img0, img1, from01, retPerLayer=False):
        """The metric for an image pair: float [N,3,H,W] (in [0, 1] with from01, PNet's [-1, 1] without) or uint8 [N,H,W,3] frames."""
        u8, N, C, H, W = _pair(img0, img1)
        if C != 3:
            raise ValueError("the perceptual metric takes RGB images")
        if min(H, W) < 16:
            raise ValueError(f"the perceptual metric needs H, W >= 16 (four 2x2 poolings), got {H} x {W}")
        x = torch.empty(2 * N, 3, H, W, device=img0.device, dtype=torch.float32)
        for t, part in ((img0, x[:N]), (img1, x[N:])):
            _lib.call("slr_vgg_prep", img0.device, t, u8, int(bool(from01)), part, N, H, W)
        per = [feature_distance(f[:N], f[N:]) for f in self.features(x)]
        val = 1.0 * per[0]                                                   # pretrained_networks.py:81-89, in its order
        for p in per[1:]:
            val = val + p
        return (val, per) if retPerLayer else val

    def forward(self, in0, in1, retPerLayer=False):
        return self.score(in0, in1, False, retPerLayer)


@torch.no_grad()
def load_vgg16_state_dict(net, sd):
    """Fill a PerceptualVGG16 from a torchvision VGG16 state dict: features.{0,2,5,...,28}.{weight,bias}.  classifier.* (a full
    vgg16-*.pth) is ignored; a missing or misshaped key, or any other key, raises."""
    used = set()
    for k, idx in enumerate(VGG16_CONVS):
        conv = net.convs[k]
        for name, p in (("weight", conv.weight), ("bias", conv.bias)):
            key = f"features.{idx}.{name}"
            if key not in sd:
                raise KeyError(f"VGG16 state dict: {key} is missing")
            v = sd[key]
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"VGG16 state dict: {key} has shape {tuple(v.shape)}, expected {tuple(p.shape)}")
            p.copy_(v)                                                       # (in place: the prepared weight buffers see the new version)
            used.add(key)
    left = sorted(k for k in sd if k not in used and not k.startswith("classifier."))
    if left:
        raise ValueError(f"VGG16 state dict: unexpected keys {left[:8]}")
    return net


def perceptual_sim(img1, img2, net):
    """evaluation/animation/metrics.py:perceptual_sim -- net(img1 * 2 - 1, img2 * 2 - 1) with the scaling inside the input kernel;
    img1 / img2 float [N,3,H,W] in [0, 1] or uint8 [N,H,W,3] frames.  -> [N]."""
    return net.score(img1, img2, True)


def perceptual_batch(H, W):
    """Frame pairs per Perceptual batch: the two widest tensors alive at once (64 channels at full size, both images of every pair,
    4 bytes) stay within PERCEPTUAL_BYTES -- 4 pairs at 720 x 1280."""
    return max(1, PERCEPTUAL_BYTES // (2 * 2 * 64 * 4 * H * W))


def relu_maxpool3x3s2(x):
    """nn.ReLU + nn.MaxPool2d(3, 2) of channel-blocked [N,C,H,W] activations (floor mode, no padding) -> channel-blocked
    [N,C,(H-3)//2+1,(W-3)//2+1]."""
    N, C, H, W = x.shape
    out = torch.empty(N, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1, device=x.device, dtype=x.dtype)
    _lib.call("slr_relu_maxpool3x3s2_b8", x.device, x, out, N, C, H, W)
    return out


def lpips_distance(f0, f1, w):
    """One layer of LPIPS, [N]: mean_hw sum_c w[c] (n(relu(f0))_c - n(relu(f1))_c)^2 with n(f) = f / (sqrt(sum_c f_c^2) + 1e-10);
    f0 / f1 raw channel-blocked [N,C,H,W] features, w [C]."""
    N, C, H, W = f0.shape
    out = torch.empty(N, device=f0.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().slr_lpips_distance_ws_bytes(N, H, W), dtype=torch.uint8, device=f0.device)
    _lib.call("slr_lpips_distance", f0.device, f0, f1, w, out, N, C, H, W, ws, ws.numel())
    return out


class LPIPSAlex(nn.Module):
    """lpips.LPIPS(net='alex', version='0.1') in eval() mode with spatial averaging, on this package's kernels:
    forward(in0, in1, retPerLayer=False, normalize=False) -> [N,1,1,1], with retPerLayer also the five per-layer [N,1,1,1] -- the
    package's signature and shapes.  in0 / in1: float [N,3,H,W] in [-1, 1] (in [0, 1] with normalize=True), H, W >= 31.  The trunk is
    torchvision's alexnet.features cut after each ReLU (pretrained_networks.py:154-196), the heads are the package's lin0 ... lin4
    (1x1, no bias); ``from_files`` / ``load_lpips_state_dicts`` fill both; nothing is downloaded.  Both images run as ONE batch of 2N
    through the trunk; features stay raw and channel-blocked, each consumer applies the ReLU."""

    def __init__(self):
        super().__init__()
        self.conv1 = nets.ConvKxK(3, 64, 11, 4, 2)
        self.conv2 = nets.ConvKxK(64, 192, 5, 1, 2)
        self.convs = nn.ModuleList(nets.Conv(ALEX_CHANNELS[k], ALEX_CHANNELS[k + 1], 3) for k in (2, 3, 4))
        self.lins = nn.ParameterList(nn.Parameter(torch.zeros(c), requires_grad=False) for c in ALEX_CHANNELS[1:])
        self.L = 5
        self.register_buffer("_ones", torch.ones(max(ALEX_CHANNELS)), persistent=False)
        self.register_buffer("_zeros", torch.zeros(max(ALEX_CHANNELS)), persistent=False)

    @classmethod
    def from_files(cls, alexnet_path, linear_path, device=None):
        """A torchvision AlexNet state dict file (alexnet-*.pth: classifier.* is ignored) and the lpips package's weights/v0.1/alex.pth
        -> the module (on ``device``)."""
        net = load_lpips_state_dicts(cls(), torch.load(alexnet_path, map_location="cpu", weights_only=True),
                                     torch.load(linear_path, map_location="cpu", weights_only=True))
        return net.to(device) if device is not None else net

    def features(self, x):
        """The raw (pre-ReLU) outputs of the five convolutions for the prepared input x [B,3,H,W] (NCHW), channel-blocked."""
        with torch.no_grad(), nets.fp32_kernels(winograd=False):
            h1 = self.conv1(x)
            h2 = self.conv2(relu_maxpool3x3s2(h1), in_b8=True)
            outs, h = [h1, h2], relu_maxpool3x3s2(h2)
            for i, conv in enumerate(self.convs):
                relu = (self._ones[:conv.cin], self._zeros[:conv.cin]) if i else None          # (after the pool: already ReLU'd)
                h = conv.conv(h, conv.bias, relu, layout=nets.IN_B8 | nets.OUT_B8)
                outs.append(h)
        return outs

    def score(self, img0, img1, normalize=False, retPerLayer=False):
        """The metric for an image pair, [N] (and the five per-layer [N]): float [N,3,H,W] or uint8 [N,H,W,3] frames (v / 255), taken as
        they are, or as 2 x - 1 with ``normalize``."""
        u8, N, C, H, W = _pair(img0, img1)
        if C != 3:
            raise ValueError("LPIPS takes RGB images")
        if min(H, W) < LPIPS_MIN_SIZE:
            raise ValueError(f"LPIPS (alex) needs H, W >= {LPIPS_MIN_SIZE} (a smaller image leaves a pooling no output), got {H} x {W}")
        x = torch.empty(2 * N, 3, H, W, device=img0.device, dtype=torch.float32)
        for t, part in ((img0, x[:N]), (img1, x[N:])):
            _lib.call("slr_lpips_prep", img0.device, t, u8, int(bool(normalize)), part, N, H, W)
        per = [lpips_distance(f[:N], f[N:], w) for f, w in zip(self.features(x), self.lins)]
        val = per[0]                                                         # lpips: val = res[0]; val += res[l], l = 1 .. 4
        for p in per[1:]:
            val = val + p
        return (val, per) if retPerLayer else val

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        val, per = self.score(in0, in1, normalize, True)
        val = val.view(-1, 1, 1, 1)
        return (val, [p.view(-1, 1, 1, 1) for p in per]) if retPerLayer else val


@torch.no_grad()
def load_lpips_state_dicts(net, alexnet_sd, linear_sd):
    """Fill a LPIPSAlex: the trunk from a torchvision AlexNet state dict, features.{0,3,6,8,10}.{weight,bias} (classifier.* is
    ignored), the heads from the lpips package's weights/v0.1/alex.pth, lin{0..4}.model.1.weight [1,C,1,1].  A missing or misshaped key,
    or any other key, raises."""
    used = set()
    for conv, idx in zip((net.conv1, net.conv2, *net.convs), ALEX_CONVS):
        for name, p in (("weight", conv.weight), ("bias", conv.bias)):
            key = f"features.{idx}.{name}"
            if key not in alexnet_sd:
                raise KeyError(f"AlexNet state dict: {key} is missing")
            v = alexnet_sd[key]
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"AlexNet state dict: {key} has shape {tuple(v.shape)}, expected {tuple(p.shape)}")
            p.copy_(v)                                                       # (in place: the prepared weight buffers see the new version)
            used.add(key)
    left = sorted(k for k in alexnet_sd if k not in used and not k.startswith("classifier."))
    if left:
        raise ValueError(f"AlexNet state dict: unexpected keys {left[:8]}")
    used = set()
    for k, p in enumerate(net.lins):
        key = f"lin{k}.model.1.weight"
        if key not in linear_sd:
            raise KeyError(f"LPIPS linear state dict: {key} is missing")
        v = linear_sd[key]
        if tuple(v.shape) != (1, p.shape[0], 1, 1):
            raise ValueError(f"LPIPS linear state dict: {key} has shape {tuple(v.shape)}, expected {(1, p.shape[0], 1, 1)}")
        p.copy_(v.reshape(-1))
        used.add(key)
    left = sorted(k for k in linear_sd if k not in used)
    if left:
        raise ValueError(f"LPIPS linear state dict: unexpected keys {left[:8]}")
    return net


def lpips_sim(img1, img2, net):
    """What eval_CLAW.py:37 computes, loss_fn_alex(p_img, t_img) on images in [0, 1] WITHOUT normalize=True: LPIPS of the [0, 1] values
    taken as they are (the numbers of the reference's tables).  img1 / img2 float [N,3,H,W] in [0, 1] or uint8 [N,H,W,3] frames.  -> [N]."""
    return net.score(img1, img2, False)


def lpips_batch(H, W):
    """Frame pairs per LPIPS batch: the prepared input and the first convolution's output of both images of every pair (3 channels at
    full size, 64 at a sixteenth: 56 H W bytes a pair, rounded up) stay within LPIPS_BYTES -- 18 pairs at 720 x 1280."""
    return max(1, LPIPS_BYTES // (64 * H * W))


def evaluate_clip(pred, gt, perceptual=None, mask=None, batch=None, lpips=None):
    """Per-frame metrics of a clip against its ground truth, as eval_CLAW.py:35-45 computes them one frame at a time:
    {"PSNR": [n], "SSIM": [n]} (+ "Perceptual": [n] with a PerceptualVGG16, + "LPIPS": [n] with a LPIPSAlex), float32 device tensors.
    pred / gt: uint8 [n,h,w,3] frames or float [n,3,h,w] in [0, 1]; mask [n|1,1,h,w]: the masked PSNR / SSIM.  SSIM and PSNR take the
    whole clip in one call; the Perceptual metric and LPIPS run ``batch`` frame pairs at a time (default perceptual_batch / lpips_batch)."""
    sm = ssim_mse(pred, gt, 11, mask)
    res = {"PSNR": psnr_from_mse(sm[:, 1]), "SSIM": sm[:, 0]}
    H, W = (pred.shape[1], pred.shape[2]) if pred.dtype == torch.uint8 else (pred.shape[2], pred.shape[3])
    if perceptual is not None:
        b = batch or perceptual_batch(H, W)
        res["Perceptual"] = torch.cat([perceptual_sim(pred[i:i + b], gt[i:i + b], perceptual) for i in range(0, pred.shape[0], b)])
    if lpips is not None:
        b = batch or lpips_batch(H, W)
        res["LPIPS"] = torch.cat([lpips_sim(pred[i:i + b], gt[i:i + b], lpips) for i in range(0, pred.shape[0], b)])
    return res
