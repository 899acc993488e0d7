"""Encoder / decoder networks either side of the splat path, as INFERENCE modules,
so the full configurations C3/C4 of BASELINE.json can be run and real checkpoints load.
On a device every 3x3 (partial) convolution, with the BN / ReLU / mask / ratio / bias / residual
stages around it, is ONE hand-written matrix-core kernel (csrc/conv.hip, split-f16 implicit GEMM),
the 1x1 skip convolutions run on the same arithmetic and the resampling stages are HIP kernels
(csrc/resample.hip): nothing goes to MIOpen.  On the CPU (validation against the reference's own classes,
tests/test_nets_vs_reference.py) the same modules run the torch composition that defines them.

Own definitions, folded for inference (reference file:line cited per class):
  * spectral norm (legacy hook, models/layers/blocks.py:5-18): eval-mode weight is
    weight_orig / (u^T W v), no power iteration -> folded once at load time;
  * noise-conditioned BN (models/layers/normalization.py:19-90) with the zero noise the test
    scripts force (bn_noise_misc=True, test_animating/test_baseline_4eval_rawsize.py:127):
    gain = 1, bias = 0, stored statistics -> a per-channel scale/shift (:219-231);
  * partial convolution (models/layers/partialconv2d.py:41-81, multi_channel=True): the mask
    update conv(mask, ones[out,in,k,k]) is the same for every output channel and equals
    box_filter(sum_c mask); masks are binary so this is exact integer arithmetic in fp32
    (< 2^24) -> computed on ONE channel instead of a second full-size convolution
    (halves the decoder FLOPs without changing a bit of its result).

``load_reference_state_dict`` maps the reference's checkpoint key scheme onto these modules.
"""
import collections
import ctypes
import math
import types

import threading

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


IN_B8, OUT_B8, RES_B8, CONV_F32, CONV_WINO, SKIP_B8, POOL_OUT, UP_OUT = 1, 2, 4, 8, 16, 32, 64, 128      # include/slr_splat.h: SLR_CONV_IN_B8 / _OUT_B8 / _RES_B8 / SLR_CONV_F32 / _WINO / _SKIP_B8 / _POOL_OUT / _UP_OUT


class _Route(threading.local):
    """What the context managers below switch, per HOST THREAD (two animators on two threads do not see each other's route or
    activation scale).  The saturation counter they react to is one per DEVICE (include/slr_splat.h: slr_conv_saturation_count):
    its attribution to a batch assumes one renderer per device at a time."""
    cpu_reference = False
    torch_convs = False                  # inside torch_convolutions(): every stage through its torch definition (fp32)
    act_scale = 64.0                     # pre-scale of the activations in the split-f16 kernels (include/slr_splat.h: xscale)
    f32_kernels = False                  # inside fp32_kernels(): the convolutions on the fp32 matrix instructions (the fp32 rung)
    winograd = False                     # ... its 3x3 convolutions as Winograd F(2x2, 3x3) (csrc/conv_wino.hpp); False (= FP32_WINOGRAD): direct
    fused_skips = True                   # a block's 1x1 skip convolution rides in its second 3x3 kernel (slr_*_forward_skip); staged_skips(): two kernels
    fused_pools = True                   # ... and a "Down" block's average pool in that kernel's epilogue; staged_skips(pools_only=True): pool kernel
    narrow_tail = True                   # the 128 -> 3 block's first convolution and skip ride in the block before (slr_pconv3x3_forward_tail + slr_narrow_gather); staged_narrow_end(): the two-kernel path


_S = _Route()


def _b8(x, channels):
    """On the device every activation whose channel count is a multiple of 8 lives channel-blocked ([N,C/8,H,W,8]
    in memory, carried in a tensor of the logical shape [N,C,H,W]): all its producers and consumers are our kernels,
    which then move 16 bytes per lane and instruction instead of 4.  The networks' inputs and outputs (3-, 65-, 2-channel
    ends, the splat's feature planes) stay NCHW; no torch op ever touches a blocked tensor."""
    return x.is_cuda and channels % 8 == 0 and not _S.torch_convs


class torch_convolutions:
    """VALIDATION AID, not a product route: no animator policy selects it (pipeline.CONV_POLICIES = auto | split | fp32 | fp32-winograd, all on this
    package's kernels).  Inside it every stage runs the torch composition that DEFINES it (nets.py: F.conv2d -> MIOpen fp32 on ROCm,
    elementwise stages as torch ops) -- the arithmetic the reference's decoder uses (models/layers/partialconv2d.py:61-74,
    models/networks/architectures.py:345-375).  The GPU tests compare the HIP stages with it, and bench.py times it beside the fp32
    rung (fps_fp32_convs.through_torch_miopen)."""

    def __enter__(self):
        self._prev, _S.torch_convs = _S.torch_convs, True
        return self

    def __exit__(self, *exc):
        _S.torch_convs = self._prev
        return False


FP32_WINOGRAD = False                    # what fp32_kernels() without an argument selects (the strict rung: direct 3x3 kernels)


class fp32_kernels:
    """Context manager: the FULL-RANGE fp32 rung of these networks on this package's own kernels.  Inside it every 3x3 / 1x1
    convolution runs on v_mfma_f32_32x32x2_f32 (csrc/conv.hip, SLR_CONV_F32): fp32 operands, fp32 products, fp32 accumulation --
    the arithmetic of the reference's decoder (models/layers/partialconv2d.py:61-74, models/networks/architectures.py:345-375) with
    no limit on the magnitude of the activations, at the fp32 matrix rate (157 TFLOP/s against the ~830 effective of the split-f16
    rung); prologue, epilogue, mask update, layouts and every other kernel are the ones of the split-f16 rung.  The animators enter
    it on request (convs="fp32") or by themselves when the split-f16 kernels report a clamped activation (convs="auto").
    winograd=True (the animators' convs="fp32-winograd"): the 3x3 convolutions with more than 4 output channels as Winograd F(2x2, 3x3) on
    the same instructions (csrc/conv_wino.hpp, SLR_CONV_WINO) -- 16 instead of 36 multiplications per 2x2 outputs, still fp32 operands /
    products / accumulation, 1.5x the direct kernel's speed.  Accuracy, measured per layer against fp64 on 3 .. 272 input channels
    (tests/test_gpu_conv_wino.py, profiles/conv_wino_range.txt; E = max error / max|output|): E <= 1.5e-6 (1.3e-6 up to 256 channels), 0.8 - 3.6x
    a plain fp32 convolution's on the CPU and 1.0 - 2.5x an fp32 Winograd's written out in torch; the direct kernel on the same layers: E <= 4.1e-6,
    from 16 input channels on 1.4 - 3.9x the Winograd kernel's (it adds up 9 Cin products per output in one chain, this one Cin per transformed
    position) -- NOT the "2 - 4x the direct kernel's error" this text used to state.  Whole networks are another matter: the seeded
    random-weight networks of the native fixture amplify a perturbation of a
    layer about 400x at a few ill-conditioned pixels (the reference's own two fp32 runs differ by 2e-4 there), so whole frames come out
    9e-7 from the direct rung's on average and up to 3.9e-4 at ~50 pixels -- 2.6e-4 from the fp64 frames at worst, where the direct
    rung (the default, winograd=False / nets.FP32_WINOGRAD) stays within 1.4e-5 (tests/test_large_golden.py).  Fast fp32, not the anchor."""

    def __init__(self, winograd=None):
        self.winograd = FP32_WINOGRAD if winograd is None else bool(winograd)

    def __enter__(self):
        self._prev, _S.f32_kernels = _S.f32_kernels, True
        self._prev_w, _S.winograd = _S.winograd, self.winograd
        return self

    def __exit__(self, *exc):
        _S.f32_kernels = self._prev
        _S.winograd = self._prev_w
        return False


class activation_scale:
    """Context manager: pre-scale of the activations in the split-f16 kernels (a power of two in (0, 64]; default 64).
    The exact domain of the split is |activation| < 65472 / scale: 1023 at 64, 65472 at 1 (csrc/conv.hip).
    The lower edge (include/slr_splat.h: xscale; measured by tests/test_gpu_conv_range.py): below |activation| * scale = 2^-2 the lo half is an
    f16 subnormal, which gfx950 keeps, so a layer's error against fp64 grows smoothly as its inputs shrink -- input std 1 / 2^-8 / 2^-16:
    5.9e-7 / 6.3e-7 / 2.1e-5 of the output range at scale 64, 5.9e-7 / 4.9e-6 / 1.4e-3 at scale 1 (plain fp32: 0.9 - 3e-7); worse than ten
    times plain fp32 below an input std of about 2^-13 at scale 64, 2^-7 at scale 1.  Nothing counts this underflow."""

    def __init__(self, scale):
        m, e = math.frexp(float(scale))
        if not (0.0 < scale <= 64.0 and m == 0.5):
            raise ValueError("activation_scale: a power of two in (0, 64]")
        self.scale = float(scale)

    def __enter__(self):
        self._prev, _S.act_scale = _S.act_scale, self.scale
        return self

    def __exit__(self, *exc):
        _S.act_scale = self._prev
        return False


class staged_skips:
    """VALIDATION AID: inside, a residual block's 1x1 skip convolution is a kernel of its own again (slr_conv1x1_forward, its result the
    residual of the second 3x3 kernel) -- the form the fused kernels are tested against (tests/test_gpu_parity.py)."""

    def __init__(self, pools_only=False):
        self.pools_only = pools_only                 # keep the fused skip, stage only the "Down" blocks' average pool

    def __enter__(self):
        self._prev = (_S.fused_skips, _S.fused_pools)
        _S.fused_skips = self.pools_only
        _S.fused_pools = False

    def __exit__(self, *exc):
        _S.fused_skips, _S.fused_pools = self._prev
        return False


class staged_narrow_end:
    """VALIDATION AID: inside, the decoder's last 128-channel block writes its result and the 128 -> 3 block reads it back with the
    <= 4-channel kernel (slr_pconv3x3_forward -> slr_pconv3x3_forward_skipout) -- the two-kernel path the tail route is tested against
    (tests/test_gpu_decoder_tail.py)."""

    def __enter__(self):
        self._prev, _S.narrow_tail = _S.narrow_tail, False

    def __exit__(self, *exc):
        _S.narrow_tail = self._prev
        return False


_BlockRoute = collections.namedtuple("_BlockRoute", "form b8 first skip second pool")


def _block_route(blk, x, b8_in, explicit_mask=True):
    """How a residual block (ResBlock, PconvResBlock) runs on ``x``: form "narrow" (<= 4 output channels: the first 3x3 kernel also
    writes the skip conv_b(x), slr_*_forward_skipout; needs an explicit mask), "fused" (the skip rides in the second 3x3 kernel,
    slr_*_forward_skip: channel-blocked block input and intermediate, more than 4 output channels; on the fp32 rung the 128-channel
    kernels only, none in the Winograd kernel) or "staged" (1x1 kernel -> residual of the second 3x3 kernel); ``b8``: the block's
    output is channel-blocked (see _b8); the layout flags of the ``first`` 3x3, the ``skip`` 1x1 (staged) and the ``second`` 3x3
    kernel; ``pool``: the resampling the fused second kernel takes into its epilogue (False, True = "Down", "Up")."""
    cout = blk.conv_aa.weight.shape[0]
    b8 = _b8(x, cout)                                   # layout of everything the block produces
    lin = IN_B8 if b8_in else 0
    rides = blk.conv_b is not None and b8_in and _S.fused_skips and x.is_cuda and not _S.torch_convs
    if rides and cout <= 4 and explicit_mask:           # the narrow end (128 -> 3): conv_aa and conv_b(x) from one pass over x
        return _BlockRoute("narrow", b8, lin, 0, 0, False)
    first = lin | (OUT_B8 if b8 else 0)
    if rides and b8 and cout > 4 and not (_S.f32_kernels and (_S.winograd or cout <= 64)):
        return _BlockRoute("fused", b8, first, 0, IN_B8 | OUT_B8, blk.pools if (cout > 64 and _S.fused_pools) else False)
    skip_b8 = b8 and cout > 4 if blk.conv_b is not None else b8_in          # (the <= 4-channel skip kernel writes NCHW)
    second = (IN_B8 | OUT_B8 if b8 else 0) | (RES_B8 if skip_b8 and b8 else 0)
    return _BlockRoute("staged", b8, first, lin | (OUT_B8 if skip_b8 else 0), second, False)


def _pool_out(N, cout, H, W, like, pool):
    """(output tensor, pooling scratch, its bytes, layout flag) of the *_forward_skip calls: with ``pool`` the output is the block's
    avgpool3x3s2 result and the kernel needs side buffers (include/slr_splat.h: SLR_CONV_POOL_OUT)."""
    if not pool:
        return torch.empty(N, cout, H, W, device=like.device, dtype=like.dtype), None, 0, 0
    if pool == "Up":                                  # x2 bilinear up-sampling in the epilogue (SLR_CONV_UP_OUT)
        nbytes = _lib.lib().slr_conv_up_ws_bytes(N, cout, H, W)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
        return torch.empty(N, cout, 2 * H, 2 * W, device=like.device, dtype=like.dtype), ws, nbytes, UP_OUT
    nbytes = _lib.lib().slr_conv_pool_ws_bytes(N, cout, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
    return torch.empty(N, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=like.device, dtype=like.dtype), ws, nbytes, POOL_OUT


class cpu_reference:
    """Context manager for the TESTS that validate these module definitions against the reference's own
    classes (which only exist where the reference checkout is, on the CPU): inside it, CPU tensors run
    the torch composition that defines every fused stage.  Outside it CPU tensors raise, like the
    reference's operators do (models/softsplat.py:418-419): the product has no CPU path.  (bench.py's `cpu_baseline` leg
    also enters it, to TIME the decoder on the host cores for its reported CPU figure -- never a product path.)"""

    def __enter__(self):
        self._prev, _S.cpu_reference = _S.cpu_reference, True
        return self

    def __exit__(self, *exc):
        _S.cpu_reference = self._prev
        return False


def _fused_ok(*ts):
    """Device tensors ALWAYS take the HIP kernels (fp32, contiguous, no autograd -- anything else on a
    device raises: there is no silent torch path on the GPU).  CPU tensors raise NotImplementedError
    unless the caller is inside ``cpu_reference()`` (validation of these definitions against the
    reference classes): then they take the torch composition, which IS the definition the kernels are
    tested against (tests/test_gpu_parity.py)."""
    if _S.torch_convs and all(t.is_cuda for t in ts):
        return False                                       # the supported fp32 route (torch_convolutions)
    if not any(t.is_cuda for t in ts):
        if not _S.cpu_reference:
            raise NotImplementedError("slr_sfs_amd.nets run on ROCm device tensors only (no CPU path); the torch "
                                      "definition used for validation is available inside nets.cpu_reference()")
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts):
        raise ValueError("slr_sfs_amd.nets: fused decoder stages need fp32 contiguous tensors on one device")
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise RuntimeError("slr_sfs_amd.nets are inference modules: run them under torch.no_grad()")
    return True


def _cached(owner, name, make, *tensors):
    """``make()``, kept in ``owner.__dict__[name]`` while ``tensors`` (what the value is derived from) keep their (data_ptr, _version,
    device): a move to another device, an in-place update (``load_state_dict``, ``copy_``) or a new tensor makes it again."""
    key = tuple((t.data_ptr(), t._version, t.device) for t in tensors)
    c = owner.__dict__.get(name)
    if c is None or c[0] != key:
        c = owner.__dict__[name] = (key, make())
    return c[1]


def bn_relu_mask(x, scale, shift, mask):
    """relu(x*scale - shift) * mask;  mask None = (x != 0), mask False = no mask."""
    if _fused_ok(x, *([mask] if torch.is_tensor(mask) else [])):
        y = torch.empty_like(x)
        mc = -1 if mask is False else 0 if mask is None else mask.shape[1]
        _lib.call("slr_bn_relu_mask", x.device, x, scale, shift, mask if torch.is_tensor(mask) else None, mc, y, *x.shape)
        return y
    y = F.relu(x * scale.view(1, -1, 1, 1) - shift.view(1, -1, 1, 1))
    if mask is False:
        return y
    return y * ((x != 0).to(x.dtype) if mask is None else mask)


def pconv_epilogue(raw0, bias, mask_box, mask_scale, winsize, residual=None, next_bn=None):
    """(raw0*ratio + b)*um on the bias-free convolution output, then `+ residual` or the next
    convolution's relu(bn(.))*um  (partialconv2d.py:61-74, blocks.py:233-236,248).
    um_raw = mask_box*mask_scale.  Returns (out, um)."""
    if _fused_ok(raw0, mask_box, *([] if residual is None else [residual])):
        out = torch.empty_like(raw0)
        um = torch.empty_like(mask_box)
        sc, sh = next_bn if next_bn is not None else (None, None)
        _lib.call("slr_pconv_epilogue", raw0.device, raw0, bias, mask_box, float(mask_scale), residual, sc, sh, out, um, float(winsize),
                   *raw0.shape)
        return out, um
    um_raw = mask_box * mask_scale
    um = torch.clamp(um_raw, 0, 1)
    ratio = winsize / (um_raw + 1e-8) * um
    out = (raw0 * ratio + bias.view(1, -1, 1, 1)) * um
    if residual is not None:
        out = out + residual
    if next_bn is not None:
        out = F.relu(out * next_bn[0].view(1, -1, 1, 1) - next_bn[1].view(1, -1, 1, 1)) * um
    return out, um


# --------------------------------------------------------------------------- building blocks

class AffineBN(nn.Module):
    """Eval-mode noise-BN with zero noise: y = x*scale - shift, scale = rsqrt(var+eps),
    shift = mean*scale (fused_bn, models/layers/normalization.py:219-231)."""

    def __init__(self, ch, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("stored_mean", torch.zeros(ch))
        self.register_buffer("stored_var", torch.ones(ch))

    def scale_shift(self):
        """(scale, shift), computed once per device and version of the statistics."""
        def make():
            scale = torch.rsqrt(self.stored_var + self.eps)
            return scale, self.stored_mean * scale
        return _cached(self, "_ss", make, self.stored_mean, self.stored_var)

    def forward(self, x):
        scale, shift = self.scale_shift()
        return x * scale.view(1, -1, 1, 1) - shift.view(1, -1, 1, 1)


class Conv(nn.Module):
    """Convolution with its spectral normalisation already folded into ``weight``."""

    def __init__(self, cin, cout, k, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False) if bias else None
        self.pad = k // 2
        self.cin, self.k = cin, k
        nn.init.normal_(self.weight, std=math.sqrt(1.0 / (cin * k * k)))

    def forward(self, x, pre_bn=None, residual=None, layout=0):
        return self.conv(x, self.bias, pre_bn, residual, layout)

    def _w4(self):
        """This 1x1 convolution's weights as plain fp32 [Cin][4] (row ci = w[0..3][ci], zero padded): the skip operand of the <= 4-channel
        3x3 kernel (slr_*_forward_skipout); prepared once per device / weight version."""
        w = self.weight

        def make():
            w4 = torch.zeros(w.shape[1], 4, device=w.device, dtype=torch.float32)
            w4[:, :w.shape[0]] = w.view(w.shape[0], w.shape[1]).t()
            return w4.contiguous()
        return _cached(self, "_w4c", make, w)

    def _conv3x3(self, name, x, args, layout=0, pre_bn=None, next_bn=None, partial=False, skipout=False, skip_conv=None,
                 skip_b8=False, pool=False):
        """The device path of the six 3x3 methods (conv, forward_skip, forward_skipout; PartialConv's forward, forward_skip,
        forward_skipout): weights and rung flags, outputs, the call of entry point ``name`` and its check.  ``args(c)`` puts the
        entry point's arguments before ``layout`` in its order, from ``c``: buf, wscale, xscale (the weights), psc, psh / nsc, nsh
        (``pre_bn`` / ``next_bn``), out, um (the update mask of a ``partial`` convolution), skip (the ``skipout`` forms' skip result),
        dims = (N, Cin, Cout, H, W); with ``skip_conv`` (the fused skip forms) sbuf, swscale, ws, ws_bytes: the skip's weights and the
        pooling scratch of ``pool``.  Returns ``c``."""
        N, cin, H, W = x.shape
        cout = self.weight.shape[0]
        c = types.SimpleNamespace(dims=(N, cin, cout, H, W), um=None, skip=None)
        c.buf, c.wscale, c.xscale, arith = self._split_weights()
        c.psc, c.psh = pre_bn if pre_bn is not None else (None, None)
        c.nsc, c.nsh = next_bn if next_bn is not None else (None, None)
        layout |= arith
        if skip_conv is not None:
            c.sbuf, c.swscale, _, sarith = skip_conv._split_weights()
            assert arith == sarith and not (arith & CONV_WINO)
            c.out, c.ws, c.ws_bytes, pflag = _pool_out(N, cout, H, W, x, pool)
            layout |= pflag | (SKIP_B8 if skip_b8 else 0)
        else:
            c.out = torch.empty(N, cout, H, W, device=x.device, dtype=x.dtype)
        if skipout:
            c.skip = torch.empty(N, cout, H, W, device=x.device, dtype=x.dtype)
        if partial:
            c.um = torch.empty(N, 1, H, W, device=x.device, dtype=x.dtype)
        _lib.call(name, x.device, *args(c), layout)
        return c

    def forward_skipout(self, x, pre_bn, skip_conv, layout=0):
        """(conv(relu(bn(x))) + bias, skip_conv(x)) from ONE pass over x: Cout <= 4, channel-blocked x (slr_conv3x3_forward_skipout)."""
        assert self.k == 3 and skip_conv.k == 1 and _fused_ok(x)
        c = self._conv3x3("slr_conv3x3_forward_skipout", x, lambda c: (
            x, c.buf, self.bias, None, c.out, *c.dims, c.wscale, c.xscale, c.psc, c.psh, skip_conv._w4(), skip_conv.bias, c.skip),
            layout, pre_bn, skipout=True)
        return c.out, c.skip

    def forward_skip(self, x, pre_bn, skip_x, skip_conv, layout=0, skip_b8=False, pool=False):
        """conv(relu(bn(x))) + bias + skip_conv(skip_x) in ONE kernel (slr_conv3x3_forward_skip; blocks.py:83-87); ``pool``: and the
        "Down" block's average pool (:196-199) in its epilogue."""
        assert self.k == 3 and skip_conv.k == 1 and _fused_ok(x, skip_x)
        return self._conv3x3("slr_conv3x3_forward_skip", x, lambda c: (
            x, c.buf, self.bias, c.out, *c.dims, c.wscale, c.xscale, c.psc, c.psh,
            skip_x, c.sbuf, skip_conv.bias, skip_x.shape[1], c.swscale, c.ws, c.ws_bytes),
            layout, pre_bn, skip_conv=skip_conv, skip_b8=skip_b8, pool=pool).out

    def _split_weights(self):
        """Weights of the matrix-core kernels (csrc/conv.hip) in fragment order, prepared once per device / weight version and
        arithmetic: (buffer, wscale, xscale, layout flag).  Split-f16 rung: hi / lo halves scaled by wscale; fp32 rung
        (inside fp32_kernels()): the fp32 values themselves, no scales."""
        w = self.weight
        f32 = _S.f32_kernels
        wino = f32 and _S.winograd and self.k == 3 and w.shape[0] > 4 and w.shape[1] <= 256     # (its prologue table holds 256 channels)
        kind = "wino" if wino else "f32" if f32 else "split"
        conv = "conv3x3" if self.k == 3 else "conv1x1"

        def make():
            nbytes = getattr(_lib.lib(), "slr_conv3x3_wino_weight_bytes" if wino else f"slr_{conv}_weight_bytes")
            buf = torch.empty(nbytes(w.shape[0], w.shape[1]), dtype=torch.uint8, device=w.device)
            if f32:
                wscale = 1.0
                _lib.call(f"slr_{conv}_{'wino' if wino else 'f32'}_weights", w.device, w, buf, w.shape[0], w.shape[1])
            else:
                amax = float(w.abs().max())
                wscale = 2.0 ** math.floor(math.log2(4096.0 / amax)) if amax > 0 else 1.0
                _lib.call(f"slr_{conv}_split_weights", w.device, w, buf, w.shape[0], w.shape[1], wscale)
            return buf, wscale
        buf, wscale = _cached(self, "_w" + kind, make, w)
        return (buf, 1.0, 1.0, CONV_F32 | (CONV_WINO if wino else 0)) if f32 else (buf, wscale, _S.act_scale, 0)

    def conv(self, x, bias, pre_bn=None, residual=None, layout=0):
        """conv(relu(bn(x))) + bias + residual (``pre_bn`` = (scale, shift) of the BN in front, or None).
        On a device 3x3 layers run on the matrix cores (split-f16 implicit GEMM of csrc/conv.hip, BN +
        ReLU fused into its prologue, bias / residual into its epilogue) and so do the 1x1 skips; CPU
        tensors (validation against the reference classes, inside nets.cpu_reference()) take the torch
        composition."""
        if self.k == 3 and _fused_ok(x, *([] if residual is None else [residual])):
            return self._conv3x3("slr_conv3x3_forward", x, lambda c: (
                x, c.buf, bias, residual, c.out, *c.dims, c.wscale, c.xscale, c.psc, c.psh), layout, pre_bn).out
        assert layout == 0 or x.is_cuda        # the channel-blocked intermediate exists on the device path only
        if residual is not None:
            return self.conv(x, bias, pre_bn) + residual
        if pre_bn is not None:
            x = bn_relu_mask(x, pre_bn[0], pre_bn[1], False)
        if self.k == 1 and self.weight.shape[0] <= 4 and ((layout & IN_B8) or (x.shape[2] * x.shape[3]) % 4 == 0) \
                and _fused_ok(x):
            N, cin, H, W = x.shape                      # skip branch onto the 3 output channels: HBM-bound HIP kernel
            cout = self.weight.shape[0]
            out = torch.empty(N, cout, H, W, device=x.device, dtype=x.dtype)
            assert not (layout & OUT_B8)
            _lib.call("slr_conv1x1_small", x.device, x, self.weight, bias, out, N, cin, cout, H, W, int(bool(layout & IN_B8)))
            return out
        if self.k == 1 and _fused_ok(x):                 # the other 1x1 skip branches: split-f16 MFMA, HBM-bound
            N, cin, H, W = x.shape
            cout = self.weight.shape[0]
            buf, wscale, xscale, arith = self._split_weights()
            out = torch.empty(N, cout, H, W, device=x.device, dtype=x.dtype)
            _lib.call("slr_conv1x1_forward", x.device, x, buf, bias, out, N, cin, cout, H, W, wscale, xscale, layout | arith)
            return out
        return F.conv2d(x, self.weight, bias, padding=self.pad)


class PartialConv(Conv):
    """PartialConv2d(multi_channel=True, return_mask=True), models/layers/partialconv2d.py:41-81,
    together with the BN + ReLU + input*mask in front of it (blocks.py:229-236).

    ``mask``: [N,1,H,W] channel-uniform mask, or None = (x != 0) per element
    (models/networks/architectures.py:369; needs ``pre_bn``).  ``pre_bn`` = (scale, shift): the input
    of the convolution is relu(x*scale - shift)*mask; None: ``x`` is already that tensor (the output
    of the previous partial convolution called with ``next_bn``).
    conv(mask, ones[out,in,k,k]) (:61) is the same k x k box sum for every output channel:
    box_k(mplane)*mscale with (mplane, mscale) = (mask, Cin) or (channel sum of the per-element
    mask, 1) -- exact integer arithmetic in fp32.
    Returns (out, update_mask [N,1,H,W]); with ``next_bn`` the output is already the activated,
    masked input of the block's second convolution.  On a device all of this is ONE kernel
    (slr_pconv3x3_forward, which also forms the box sum and the per-element mask from the staged
    input); on the CPU the torch composition that defines it."""

    def forward_skipout(self, x, mask, skip_conv, next_bn, pre_bn, layout=0):
        """The block's first partial convolution and, from the same pass over x, the block's 1x1 skip convolution of the raw x: Cout <= 4,
        channel-blocked x (slr_pconv3x3_forward_skipout; blocks.py:229-236, 243-247).  Returns (out, update_mask, skip)."""
        assert self.k == 3 and skip_conv.k == 1 and skip_conv.bias is None and _fused_ok(x, *([] if mask is None else [mask]))
        c = self._conv3x3("slr_pconv3x3_forward_skipout", x, lambda c: (
            x, c.psc, c.psh, mask, c.buf, c.wscale, c.xscale, self.bias, None, c.nsc, c.nsh, c.out, c.um, *c.dims,
            skip_conv._w4(), c.skip), layout, pre_bn, next_bn, partial=True, skipout=True)
        return c.out, c.um, c.skip

    def forward_skip(self, x, mask, skip_x, skip_conv, layout=0, skip_b8=False, pool=False):
        """The block's second partial convolution with the 1x1 skip branch inside (slr_pconv3x3_forward_skip; blocks.py:237-248):
        ``x`` is the activated, masked output of the first one.  Returns (out, update_mask)."""
        assert self.k == 3 and skip_conv.k == 1 and skip_conv.bias is None and _fused_ok(x, mask, skip_x)
        c = self._conv3x3("slr_pconv3x3_forward_skip", x, lambda c: (
            x, None, None, mask, c.buf, c.wscale, c.xscale, self.bias, c.out, c.um, *c.dims,
            skip_x, c.sbuf, skip_x.shape[1], c.swscale, c.ws, c.ws_bytes),
            layout, partial=True, skip_conv=skip_conv, skip_b8=skip_b8, pool=pool)
        return c.out, c.um

    def _tail_weights(self, skip_conv):
        """Column weights of the tail phase for THIS 128 -> 3 convolution and the block's 1x1 ``skip_conv`` (slr_conv_tail_weights), prepared
        once per device / weight version: (buffer, wscale, skip wscale) -- each branch its own power of two, by _split_weights' rule."""
        w, wb = self.weight, skip_conv.weight

        def make():
            def scale(t):
                amax = float(t.abs().max())
                return 2.0 ** math.floor(math.log2(4096.0 / amax)) if amax > 0 else 1.0
            buf = torch.empty(_lib.lib().slr_conv_tail_weight_bytes(w.shape[1]), dtype=torch.uint8, device=w.device)
            wscale, swscale = scale(w), scale(wb)
            _lib.call("slr_conv_tail_weights", w.device, w, wb, buf, w.shape[1], wscale, swscale)
            return buf, wscale, swscale
        return _cached(self, "_wtail", make, w, wb)

    def forward_tail(self, x, mask, residual, nxt):
        """This block's second partial convolution (``x``: the activated output of the first, channel-blocked like ``residual``) WITHOUT its
        result: the tail phase hands the next block ``nxt`` (128 -> 3, narrow form) what its first convolution and skip need, and the gather
        finishes them (slr_pconv3x3_forward_tail, slr_narrow_gather; split-f16 rung).  Returns what ``nxt.conv_aa.forward_skipout`` returns
        on the unwritten result: (activated input of nxt's second convolution, update mask, skip)."""
        assert self.k == 3 and _fused_ok(x, mask, residual) and not _S.f32_kernels
        N, cin, H, W = x.shape
        cout = self.weight.shape[0]
        buf, wscale, xscale, _ = self._split_weights()
        tbuf, twscale, tswscale = nxt.conv_aa._tail_weights(nxt.conv_b)
        tsc, tsh = nxt.bn1.scale_shift()
        nsc, nsh = nxt.bn2.scale_shift()
        z = torch.empty(N, 32, H, W, device=x.device, dtype=x.dtype)
        um = torch.empty(N, 1, H, W, device=x.device, dtype=x.dtype)
        _lib.call("slr_pconv3x3_forward_tail", x.device, x, mask, buf, wscale, xscale, self.bias, residual, tsc, tsh, tbuf, z, um,
                  N, cin, cout, H, W)
        a, m, skip = (torch.empty(N, c, H, W, device=x.device, dtype=x.dtype) for c in (3, 1, 3))
        _lib.call("slr_narrow_gather", x.device, z, um, nxt.conv_aa.bias, nsc, nsh, None, a, m, skip, N, cout, H, W, twscale, tswscale, xscale)
        return a, m, skip

    def forward(self, x, mask, residual=None, next_bn=None, pre_bn=None, layout=0):
        cin = x.shape[1]
        assert mask is not None or pre_bn is not None
        if self.k == 3 and _fused_ok(x, *([] if mask is None else [mask]), *([] if residual is None else [residual])):
            c = self._conv3x3("slr_pconv3x3_forward", x, lambda c: (
                x, c.psc, c.psh, mask, c.buf, c.wscale, c.xscale, self.bias, residual, c.nsc, c.nsh, c.out, c.um, *c.dims),
                layout, pre_bn, next_bn, partial=True)
            return c.out, c.um
        assert layout == 0
        if mask is None:
            mplane, mscale = (x != 0).sum(1, keepdim=True).to(x.dtype), 1.0
        else:
            mplane, mscale = mask, float(cin)
        box = F.avg_pool2d(mplane, self.k, stride=1, padding=self.pad, divisor_override=1)
        xin = bn_relu_mask(x, pre_bn[0], pre_bn[1], mask) if pre_bn is not None else x
        raw0 = self.conv(xin, None)                                                # bias joins in the epilogue
        return pconv_epilogue(raw0, self.bias, box, mscale, cin * self.k * self.k, residual, next_bn)


def avgpool_down(x, b8=False):
    """nn.AvgPool2d(3, stride=2, padding=1), blocks.py:196-199 (b8: x and the result are channel-blocked)."""
    if _fused_ok(x):
        N, C, H, W = x.shape
        out = torch.empty(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=x.device, dtype=x.dtype)
        _lib.call("slr_avgpool3x3s2", x.device, x, out, N, C, H, W, int(b8))
        return out
    return F.avg_pool2d(x, 3, stride=2, padding=1)


def upsample_up(x, b8=False):
    """nn.Upsample(scale_factor=2, mode='bilinear'), blocks.py:200-203 (b8: x and the result are channel-blocked)."""
    if _fused_ok(x):
        N, C, H, W = x.shape
        out = torch.empty(N, C, 2 * H, 2 * W, device=x.device, dtype=x.dtype)
        _lib.call("slr_upsample_bilinear2x", x.device, x, out, N, C, H, W, int(b8))
        return out
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


def _resample(kind):
    if kind == "Up":
        return upsample_up
    if kind:                                                       # "Down" / encoder "downsample=True"
        return avgpool_down
    return lambda x, b8=False: x


def _resample_mask(kind):
    if kind == "Down":
        return lambda m: F.max_pool2d(m, 3, stride=2, padding=1)
    if kind == "Up":
        return lambda m: F.interpolate(m, scale_factor=2, mode="nearest")
    return lambda m: m


class ResBlock(nn.Module):
    """ResNet_Block, models/layers/blocks.py:47-87."""

    def __init__(self, cin, cout, resample=None):
        super().__init__()
        self.bn1, self.bn2 = AffineBN(cin), AffineBN(cout)
        self.conv_aa, self.conv_ab = Conv(cin, cout, 3), Conv(cout, cout, 3)
        self.conv_b = Conv(cin, cout, 1) if (resample or cin != cout) else None
        self.resample = _resample(resample)
        self.pools = "Up" if resample == "Up" else bool(resample)        # the resampling the fused second convolution can take into its epilogue

    def forward(self, x, b8_in=False):
        """-> (y, b8_out): ``b8_in`` / ``b8_out`` = x / y are channel-blocked in memory (see _b8)."""
        r = _block_route(self, x, b8_in)
        if r.form == "narrow":
            a, b = self.conv_aa.forward_skipout(x, self.bn1.scale_shift(), self.conv_b, layout=r.first)
            a = self.conv_ab(a, self.bn2.scale_shift(), residual=b)
            return self.resample(a, r.b8), r.b8
        a = self.conv_aa(x, self.bn1.scale_shift(), layout=r.first)                         # BN + ReLU ride in the prologue
        if r.form == "fused":                                                                # x_a + conv_b(x) (:83-87) in one kernel
            a = self.conv_ab.forward_skip(a, self.bn2.scale_shift(), x, self.conv_b, layout=r.second, skip_b8=b8_in, pool=r.pool)
            return (a if r.pool else self.resample(a, r.b8)), r.b8
        b = self.conv_b(x, layout=r.skip) if self.conv_b is not None else x
        a = self.conv_ab(a, self.bn2.scale_shift(), residual=b, layout=r.second)             # x_a + x_b (:87) in the epilogue
        return self.resample(a, r.b8), r.b8       # == resample(x_a) + resample(x_b): both resamplers are linear


class PconvResBlock(nn.Module):
    """ResNet_Block_Pconv2 with pconv_pbn_woresbias, models/layers/blocks.py:173-248."""

    def __init__(self, cin, cout, resample=None):
        super().__init__()
        self.bn1, self.bn2 = AffineBN(cin), AffineBN(cout)
        self.conv_aa, self.conv_ab = PartialConv(cin, cout, 3), PartialConv(cout, cout, 3)
        self.conv_b = Conv(cin, cout, 1, bias=False) if (resample or cin != cout) else None   # :192-193
        self.resample, self.resample_mask = _resample(resample), _resample_mask(resample)
        self.has_resample = bool(resample)
        self.pools = "Up" if resample == "Up" else bool(resample)        # the resampling the fused second convolution can take into its epilogue

    def tail_route(self, nxt, x, mask, b8_in):
        """Does this block run on ``x`` with the next block's (``nxt``) first convolution and skip folded into its second kernel?  This one:
        128 -> 128 with the identity residual (staged form), channel-blocked, no resampling; ``nxt``: 128 -> 3 in the narrow form; the
        split-f16 rung (either activation scale).  The fp32 and Winograd rungs, torch_convolutions() and staged_narrow_end() keep the
        two-kernel path."""
        if not (_S.narrow_tail and x.is_cuda and b8_in and mask is not None) or _S.f32_kernels or _S.torch_convs or _S.cpu_reference:
            return False
        if self.conv_b is not None or self.has_resample or tuple(self.conv_ab.weight.shape[:2]) != (128, 128):
            return False
        return (_block_route(self, x, b8_in).form == "staged" and nxt.conv_b is not None and nxt.conv_aa.weight.shape[0] == 3 and
                nxt.conv_aa.weight.shape[1] == 128 and _block_route(nxt, x, True).form == "narrow")

    def forward_with_narrow(self, nxt, x, mask):
        """This block and ``nxt`` on the tail route (see tail_route): -> what ``nxt`` returns."""
        r = _block_route(self, x, True)
        a, m = self.conv_aa(x, mask, next_bn=self.bn2.scale_shift(), pre_bn=self.bn1.scale_shift(), layout=r.first)
        a, m, skip = self.conv_ab.forward_tail(a, m, x, nxt)
        a, m = nxt.conv_ab(a, m, residual=skip)
        return nxt.resample(a, False), nxt.resample_mask(m), False

    def forward(self, x, mask, b8_in=False):
        """-> (y, update_mask, b8_out).  mask: None = (x != 0) per channel (architectures.py:369; x is NCHW then), else
        [N,1,H,W] channel-uniform; ``b8_in`` / ``b8_out``: x / y are channel-blocked in memory (see _b8)."""
        r = _block_route(self, x, b8_in, mask is not None)
        if r.form == "narrow":
            a, m, skip = self.conv_aa.forward_skipout(x, mask, self.conv_b, self.bn2.scale_shift(), self.bn1.scale_shift(), layout=r.first)
            a, m = self.conv_ab(a, m, residual=skip)
            return self.resample(a, r.b8), self.resample_mask(m), r.b8
        a, m = self.conv_aa(x, mask, next_bn=self.bn2.scale_shift(), pre_bn=self.bn1.scale_shift(), layout=r.first)   # :229-236
        # x_a + x_b (:248).  The reference resamples the two branches separately and adds; avg-pool
        # and bilinear up-sampling are linear, so resample(x_a + x_b) is the same result up to fp32
        # rounding, lets the residual join the epilogue, and halves the resampling work.
        if r.form == "fused":                                                      # :237-248 in one kernel
            a, m = self.conv_ab.forward_skip(a, m, x, self.conv_b, layout=r.second, skip_b8=b8_in, pool=r.pool)
            return (a if r.pool else self.resample(a, r.b8)), self.resample_mask(m), r.b8
        skip = self.conv_b(x, layout=r.skip) if self.conv_b is not None else x   # :243-247
        a, m = self.conv_ab(a, m, residual=skip, layout=r.second)                  # :237-239
        return self.resample(a, r.b8), self.resample_mask(m), r.b8                 # :240-241


# --------------------------------------------------------------------------- networks

_ENC = [3, 32, 32, 32, 64, 64, 64, 64]                      # configs.py:96-106 (ngf = 64)
_DEC = [64, 128, 256, 256, 128, 128, 128]                   # configs.py:117-127, inner widths
_UPDOWN = [False, "Down", "Down", False, "Up", "Up", False, False]   # configs.py:128-137


class EncoderWithZ(nn.Module):
    """ResNetEncoder_with_Z, models/networks/architectures.py:155-197: 8 blocks, no down-sampling,
    last block emits 64 features + 1 Z channel."""

    def __init__(self, cin=3, feat=64):
        super().__init__()
        ch = [cin] + _ENC[1:] + [feat + 1]
        self.blocks = nn.ModuleList(ResBlock(ch[i], ch[i + 1]) for i in range(8))

    def forward(self, x):
        b8 = False
        for b in self.blocks:
            x, b8 = b(x, b8)
        assert not b8                                    # 65 channels: NCHW
        return x[:, :-1].contiguous(), x[:, -1:].contiguous()          # :195-197


class Encoder(nn.Module):
    """ResNetEncoder (alpha encoder of SLR v1: 3 -> ... -> 2), architectures.py:121-153."""

    def __init__(self, cin=3, cout=2):
        super().__init__()
        ch = [cin] + _ENC[1:] + [cout]
        self.blocks = nn.ModuleList(ResBlock(ch[i], ch[i + 1]) for i in range(8))

    def forward(self, x):
        b8 = False
        for b in self.blocks:
            x, b8 = b(x, b8)
        assert not b8
        return x


class DecoderPconv2(nn.Module):
    """ResNetDecoderPconv2, architectures.py:345-375: input mask = (x != 0) (:369)."""

    def __init__(self, cin=64, cout=3):
        super().__init__()
        ch = [cin] + _DEC + [cout]
        self.blocks = nn.ModuleList(PconvResBlock(ch[i], ch[i + 1], _UPDOWN[i]) for i in range(8))

    def forward(self, x, return_mask=False):
        """``return_mask``: -> (frame, the last block's update mask [N,1,H,W]) (the tests compare routes on both)."""
        mask, b8 = None, False                           # (x != 0) per channel, derived inside the first block
        blocks, i = self.blocks, 0
        while i < len(blocks):
            if i + 1 < len(blocks) and blocks[i].tail_route(blocks[i + 1], x, mask, b8):       # the narrow end rides in the block before it
                x, mask, b8 = blocks[i].forward_with_narrow(blocks[i + 1], x, mask)
                i += 2
                continue
            x, mask, b8 = blocks[i](x, mask, b8)
            i += 1
        assert not b8                                    # the 1- / 3-channel end is NCHW
        return (x, mask) if return_mask else x


class BGDecoder(nn.Module):
    """ResNetBGDecoder (net_bg of SLR v1), architectures.py:233-260, arch 256W8UpDown64BG."""

    def __init__(self, cin=3, cout=3):
        super().__init__()
        ch = [cin] + _DEC + [cout]
        self.blocks = nn.ModuleList(ResBlock(ch[i], ch[i + 1], _UPDOWN[i]) for i in range(8))

    def forward(self, x):
        b8 = False
        for b in self.blocks:
            x, b8 = b(x, b8)
        assert not b8
        return x


def saturation_count(device, reset=True):
    """Waves of the split-f16 kernels on ``device`` that had to clamp an activation since the last reset (|x| beyond the
    exact domain of the split, csrc/conv.hip).  The counter is one per device; the read is ordered on torch's current
    stream of that device and synchronises it with the host."""
    n = ctypes.c_ulonglong(0)
    _lib.call("slr_conv_saturation_count", device, ctypes.byref(n), 1 if reset else 0)
    return int(n.value)


def check_saturation(device, what="convolution", reset=True):
    """Raise if a split-f16 kernel on ``device`` had to clamp an activation since the last check.  The result of such a
    launch is wrong, not merely inexact, and the reference's fp32 convolution has no such limit -- so it is an error,
    never silent.  (The animators do better than raising: pipeline.py, convs="auto".)"""
    n = saturation_count(device, reset)
    if n:
        raise RuntimeError(f"slr_sfs_amd: {n} wave(s) of the {what} kernels met activations >= {65472.0 / _S.act_scale:.0f} in "
                           f"magnitude, outside the exact range of the split-f16 matrix-core convolution; the result is not "
                           f"valid (use a smaller nets.activation_scale, nets.fp32_kernels(), or the animators' "
                           f"convs='auto')")
    return 0


class SaturationLog:
    """Asynchronous per-piece saturation records of one clip: ``mark()`` after a piece of work (a decoder batch) copies
    the device counter into pinned host memory in stream order -- no host synchronisation; ``bad()`` (after the stream
    has been synchronised) lists the pieces during which the counter moved."""

    def __init__(self, device, capacity):
        self.device = device
        self.slots = torch.zeros(capacity + 1, dtype=torch.int32).pin_memory()
        self.n = 0
        self._record()                                   # the value the clip starts from

    def _record(self):
        _lib.call("slr_conv_saturation_record", self.device, ctypes.c_void_p(self.slots.data_ptr() + 4 * self.n))
        self.n += 1

    def mark(self):
        self._record()

    def bad(self):
        torch.cuda.current_stream(self.device).synchronize()
        v = self.slots[:self.n].tolist()
        return [i for i in range(self.n - 1) if v[i + 1] != v[i]]


RUNG_SCALES = (64.0, 1.0)                # the "auto" ladder: split-f16 at these activation scales, then the fp32 rung
RUNG_FP32 = len(RUNG_SCALES)


def rung_context(rung):
    """Arithmetic of the convolutions on rung ``rung`` of the "auto" ladder: 0 split-f16 at activation scale 2^6 (exact for
    |x| < 1023), 1 split-f16 at scale 1 (|x| < 65472), RUNG_FP32 the fp32 matrix instructions (fp32_kernels(winograd=False):
    no limit; the safety net is the strict rung).  The ladder reacts to the UPPER edge only: rung 1 is 64 times coarser than rung 0 on small
    activations (activation_scale: worse than ten times plain fp32 below an input std of about 2^-7 instead of 2^-13), "auto" does not detect
    underflow, and an animator that once moved to rung 1 stays there for its later clips (guarded: ``owner``)."""
    return fp32_kernels(winograd=False) if rung >= RUNG_FP32 else activation_scale(RUNG_SCALES[rung])


def guarded(fn, device, policy, what, owner=None):
    """Run ``fn()`` (networks on split-f16 kernels) under the saturation policy of the animators:
    "split": as is, raise if an activation was clamped; "fp32" / "fp32-winograd": inside fp32_kernels() (direct / Winograd 3x3);
    "auto": split-f16 at the default activation scale; clamped -> again at scale 1 (exact up to 65472); clamped again ->
    inside fp32_kernels() (the fp32 matrix instructions: no limit).  ``owner`` (an animator) remembers the rung that worked, so later clips start there.
    Synchronises with the device once per call (per rung tried)."""
    if policy in ("fp32", "fp32-winograd"):
        with fp32_kernels(winograd=policy == "fp32-winograd"):
            return fn()
    if policy == "split":
        out = fn()
        check_saturation(device, what)
        return out
    assert policy == "auto", policy
    rung = getattr(owner, "_conv_rung", 0) if owner is not None else 0
    saturation_count(device)                                   # start from a clean counter
    for r in range(rung, RUNG_FP32):
        with rung_context(r):
            out = fn()
        if saturation_count(device) == 0:
            return out
        import warnings
        warnings.warn(f"slr_sfs_amd: activations of the {what} exceed the exact range of the split-f16 convolutions at "
                      f"activation scale {RUNG_SCALES[r]:g}; rendering again " +
                      (f"at scale {RUNG_SCALES[r + 1]:g}" if r + 1 < RUNG_FP32 else "on the fp32 rung"))
        if owner is not None:
            owner._conv_rung = r + 1
    with rung_context(RUNG_FP32):
        return fn()


# --------------------------------------------------------------------------- checkpoints

def _fold_sn(sd, key):
    """Effective eval-mode weight of a legacy spectral_norm layer: W / (u^T W_mat v)."""
    w = sd[key + ".weight_orig"] if key + ".weight_orig" in sd else sd[key + ".weight"]
    if key + ".weight_u" in sd:
        u, v = sd[key + ".weight_u"], sd[key + ".weight_v"]
        sigma = torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))
        w = w / sigma
    return w


def _load_bn(bn, sd, key):
    """key = '...bn' or '...pbn' of a (Partial)LinearNoiseLayer; zero noise -> gain 1, bias 0."""
    bn.stored_mean.copy_(sd[key + ".stored_mean"])
    bn.stored_var.copy_(sd[key + ".stored_var"])
    if isinstance(getattr(bn, "gain", None), nn.Linear):          # trainable.TrainableNoiseBN: the noise layers next to the statistics
        layer = key.rsplit(".", 1)[0]
        bn.gain.weight.copy_(_fold_sn(sd, layer + ".gain"))
        bn.bias.weight.copy_(_fold_sn(sd, layer + ".bias"))


def _load_conv(conv, sd, key):
    conv.weight.copy_(_fold_sn(sd, key))              # (in place: the prepared weight buffers see the new version)
    if conv.bias is not None:
        conv.bias.copy_(sd[key + ".bias"])


@torch.no_grad()
def load_reference_state_dict(net, sd, prefix):
    """Fill ``net`` from a reference state dict (SURVEY App. C key scheme).  ``prefix`` e.g.
    'model.module.encoder.' / 'model.module.projector.' / 'model.module.net_bg.' ..."""
    sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    for i, blk in enumerate(net.blocks):
        if isinstance(blk, PconvResBlock):
            b = f"eblocks.{i}."
            _load_bn(blk.bn1, sd, b + "bn_noise1.pbn")
            _load_bn(blk.bn2, sd, b + "bn_noise2.pbn")
            _load_conv(blk.conv_aa, sd, b + "conv_aa")
            _load_conv(blk.conv_ab, sd, b + "conv_ab")
            if blk.conv_b is not None:
                _load_conv(blk.conv_b, sd, b + "conv_b")
        else:
            b = ("eblocks" if isinstance(net, BGDecoder) else "gblocks") + f".{i}."
            _load_bn(blk.bn1, sd, b + "ch_a.0.bn")
            _load_bn(blk.bn2, sd, b + "ch_a.3.bn")
            _load_conv(blk.conv_aa, sd, b + "ch_a.2")
            _load_conv(blk.conv_ab, sd, b + "ch_a.5")
            if blk.conv_b is not None:
                _load_conv(blk.conv_b, sd, b + "ch_b.0")
    return net


# --------------------------------------------------------------------------- motion U-Nets (still image -> motion field)
# Unet4Motion (models/networks/architectures.py:382-493) and SPADEUnet4MaskMotion (:602-743 with SPADE, models/networks/networks.py:422-463),
# the motion predictors of models/unet_motion.py:30-191.  On a device every stage is one of this package's kernels and every convolution runs
# on the fp32 rung (v_mfma_f32_32x32x2_f32): the 4x4 / stride 2 encoder convolutions on slr_conv4x4s2_forward (csrc/conv4x4.hip), the 3x3
# ones on slr_conv3x3_forward with SLR_CONV_F32 (direct, not Winograd).  The predicted field feeds the Euler integration, which rounds
# positions at every step: a perturbation of the motion moves whole trajectories, so no reduced-precision rung is offered here.
MOTION_GRID = 256                        # eight stride-2 halvings: H and W must be multiples of 256 (the reference fails in torch.cat otherwise)


def _check_motion_grid(x):
    H, W = x.shape[-2:]
    if H % MOTION_GRID or W % MOTION_GRID or H == 0 or W == 0:
        raise ValueError(f"motion U-Net: H and W must be positive multiples of {MOTION_GRID} (eight stride-2 halvings), got {H} x {W}")


class EvalBN(nn.Module):
    """nn.BatchNorm2d / SyncBatchNorm in eval mode (the 'sync:spectral_batch' norm of the motion U-Net): y = (x - mean) * rsqrt(var + eps) *
    weight + bias, i.e. the per-channel affine y * scale + shift (folded into the convolution in front of it on the device)."""

    def __init__(self, ch, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("running_mean", torch.zeros(ch))
        self.register_buffer("running_var", torch.ones(ch))
        self.register_buffer("weight", torch.ones(ch))
        self.register_buffer("bias", torch.zeros(ch))

    def scale_shift(self):
        scale = self.weight / torch.sqrt(self.running_var + self.eps)
        return scale, self.bias - self.running_mean * scale

    def forward(self, x):
        return F.batch_norm(x, self.running_mean, self.running_var, self.weight, self.bias, False, 0.0, self.eps)


class Conv4x4s2(nn.Module):
    """nn.Conv2d(cin, cout, 4, stride=2, padding=1) (spectral norm folded into ``weight``), with the LeakyReLU(0.2) in front of it and an
    eval BatchNorm behind it when asked (architectures.py:448-462): ONE kernel on a device (slr_conv4x4s2_forward)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 4, 4), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        nn.init.normal_(self.weight, std=math.sqrt(1.0 / (cin * 16)))

    def _frag(self):
        w = self.weight

        def make():
            buf = torch.empty(_lib.lib().slr_conv4x4s2_weight_bytes(w.shape[0], w.shape[1]), dtype=torch.uint8, device=w.device)
            _lib.call("slr_conv4x4s2_f32_weights", w.device, w, buf, w.shape[0], w.shape[1])
            return buf
        return _cached(self, "_wfrag", make, w)

    def forward(self, x, leaky=None, bn=None):
        if _fused_ok(x):
            N, cin, H, W = x.shape
            cout = self.weight.shape[0]
            out = torch.empty(N, cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1, device=x.device, dtype=x.dtype)
            sc, sh = bn.scale_shift() if bn is not None else (None, None)
            _lib.call("slr_conv4x4s2_forward", x.device, x, self._frag(), self.bias, sc, sh, out, N, cin, cout, H, W, int(leaky is not None),
                       float(leaky or 0.0))
            return out
        if leaky is not None:
            x = F.leaky_relu(x, leaky)
        y = F.conv2d(x, self.weight, self.bias, stride=2, padding=1)
        return bn(y) if bn is not None else y


class ConvKxK(nn.Module):
    """nn.Conv2d(cin, cout, k, stride, padding) + bias for the two shapes of AlexNet that no other kernel here covers, (k, stride,
    padding) = (11, 4, 2) and (5, 1, 2) (slr_convkxk_forward: fp32 MFMA, the arithmetic of the fp32 rung).  The output is RAW and
    channel-blocked, like a ``Conv`` with OUT_B8; ``in_b8``: so is the input.  Device tensors only."""

    def __init__(self, cin, cout, k, stride, padding):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        self.cin, self.k, self.stride, self.pad = cin, k, stride, padding
        nn.init.normal_(self.weight, std=math.sqrt(1.0 / (cin * k * k)))

    def _frag(self):
        w = self.weight

        def make():
            buf = torch.empty(_lib.lib().slr_convkxk_weight_bytes(w.shape[0], w.shape[1], self.k), dtype=torch.uint8, device=w.device)
            _lib.call("slr_convkxk_f32_weights", w.device, w, buf, w.shape[0], w.shape[1], self.k)
            return buf
        return _cached(self, "_wfrag", make, w)

    def out_size(self, H, W):
        return (H + 2 * self.pad - self.k) // self.stride + 1, (W + 2 * self.pad - self.k) // self.stride + 1

    def forward(self, x, in_b8=False):
        if not x.is_cuda:
            raise NotImplementedError("slr_sfs_amd.nets.ConvKxK runs on ROCm device tensors only (no CPU path)")
        _lib.require_device(x)
        N, cin, H, W = x.shape
        cout = self.weight.shape[0]
        OH, OW = self.out_size(H, W)
        if cin != self.cin or OH < 1 or OW < 1:
            raise ValueError(f"ConvKxK({self.cin}, {cout}, {self.k}, {self.stride}, {self.pad}): input {tuple(x.shape)} gives no output")
        out = torch.empty(N, cout, OH, OW, device=x.device, dtype=x.dtype)
        _lib.call("slr_convkxk_forward", x.device, x, self._frag(), self.bias, out, N, cin, cout, H, W, self.k, self.stride, self.pad,
                  int(bool(in_b8)))
        return out


class BNConv3x3(Conv):
    """3x3 convolution followed by an eval BatchNorm (or nothing): on a device the BN is folded into the weights and bias of ONE fp32-rung
    3x3 kernel (prepared once per weight / statistics version); the torch composition runs the two stages as the reference does."""

    def __init__(self, cin, cout, bn=True):
        super().__init__(cin, cout, 3)
        self.bn = EvalBN(cout) if bn else None

    def forward(self, x):
        if self.bn is None:
            return self.conv(x, self.bias)
        if not _fused_ok(x):
            return self.bn(F.conv2d(x, self.weight, self.bias, padding=1))
        def make():
            scale, shift = self.bn.scale_shift()
            folded = Conv(self.cin, self.weight.shape[0], 3).to(self.weight.device)
            folded.weight.data.copy_(self.weight * scale.view(-1, 1, 1, 1))
            folded.bias.data.copy_(self.bias * scale + shift)
            return folded
        folded = _cached(self, "_folded", make, self.weight, self.bias, self.bn.running_mean, self.bn.running_var, self.bn.weight,
                         self.bn.bias)
        return folded.conv(x, folded.bias)


def instnorm_spade(x, gamma_beta, eps=1e-5):
    """SPADE with InstanceNorm2d (networks.py:441-463): instance_norm(x) * (1 + gamma) + beta, gamma_beta = cat(gamma, beta) [N,2C,H,W]."""
    if _fused_ok(x, gamma_beta):
        N, C, H, W = x.shape
        out = torch.empty_like(x)
        _lib.call("slr_instnorm_spade", x.device, x, gamma_beta, out, N, C, H, W, float(eps))
        return out
    C = x.shape[1]
    return F.instance_norm(x, eps=eps) * (1 + gamma_beta[:, :C]) + gamma_beta[:, C:]


def resize_segmap(seg, k, nearest_channel=3):
    """The SPADE segmap at 1 / 2^k of the input's size (networks.py:446-457): bilinear (align_corners=False, size=) for every channel but
    ``nearest_channel`` (the mask), which is nearest."""
    if _fused_ok(seg):
        N, C, H, W = seg.shape
        out = torch.empty(N, C, H >> k, W >> k, device=seg.device, dtype=seg.dtype)
        _lib.call("slr_resize_segmap", seg.device, seg, out, N, C, H, W, k, nearest_channel)
        return out
    size = (seg.shape[2] >> k, seg.shape[3] >> k)
    parts = [F.interpolate(seg[:, :nearest_channel], size=size, mode="bilinear", align_corners=False),
             F.interpolate(seg[:, nearest_channel:nearest_channel + 1], size=size, mode="nearest")]
    if seg.shape[1] > nearest_channel + 1:
        parts.append(F.interpolate(seg[:, nearest_channel + 1:], size=size, mode="bilinear", align_corners=False))
    return torch.cat(parts, 1)


RELU_NONE, RELU_BEFORE, RELU_AFTER = 0, 1, 2


def upsample2x_concat(a, b=None, nearest_channel=-1, relu=RELU_NONE):
    """cat(up(a), up(b)) with up = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False), except channel ``nearest_channel`` of
    EACH source, which is nn.Upsample(scale_factor=2, mode='nearest') (architectures.py:710-740); ReLU of the inputs (RELU_BEFORE,
    Unet4Motion :463-489) or of the result (RELU_AFTER, SPADEUnet4MaskMotion :715-741).  ONE kernel on a device (slr_upsample2x_concat)."""
    if _fused_ok(a, *([] if b is None else [b])):
        N, Ca, H, W = a.shape
        Cb = 0 if b is None else b.shape[1]
        out = torch.empty(N, Ca + Cb, 2 * H, 2 * W, device=a.device, dtype=a.dtype)
        _lib.call("slr_upsample2x_concat", a.device, a, Ca, b, Cb, out, N, H, W, nearest_channel, relu)
        return out

    def up(x):
        if relu == RELU_BEFORE:
            x = F.relu(x)
        if nearest_channel < 0:
            return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        q = nearest_channel
        return torch.cat([F.interpolate(x[:, :q], scale_factor=2, mode="bilinear", align_corners=False),
                          F.interpolate(x[:, q:q + 1], scale_factor=2, mode="nearest"),
                          F.interpolate(x[:, q + 1:], scale_factor=2, mode="bilinear", align_corners=False)], 1)
    y = up(a) if b is None else torch.cat([up(a), up(b)], 1)
    return F.relu(y) if relu == RELU_AFTER else y


class SPADEIN(nn.Module):
    """SPADE(nn.InstanceNorm2d, C, label_nc) (networks.py:422-463).  mlp_gamma and mlp_beta are ONE 3x3 convolution 128 -> 2C
    (``mlp_gb``: gamma's weights, then beta's), the ReLU of mlp_shared is that convolution's prologue; ``seg`` is the segmap already
    resized to x's size (resize_segmap)."""

    def __init__(self, C, label_nc=6, nhidden=128):
        super().__init__()
        self.C = C
        self.mlp_shared = Conv(label_nc, nhidden, 3)
        self.mlp_gb = Conv(nhidden, 2 * C, 3)
        self.register_buffer("_ones", torch.ones(nhidden), persistent=False)
        self.register_buffer("_zeros", torch.zeros(nhidden), persistent=False)

    def forward(self, x, seg):
        if _fused_ok(x, seg):
            actv = self.mlp_shared.conv(seg, self.mlp_shared.bias)
            gb = self.mlp_gb.conv(actv, self.mlp_gb.bias, pre_bn=(self._ones, self._zeros))     # relu(actv * 1 - 0)
        else:
            gb = F.conv2d(F.relu(F.conv2d(seg, self.mlp_shared.weight, self.mlp_shared.bias, padding=1)), self.mlp_gb.weight,
                          self.mlp_gb.bias, padding=1)
        return instnorm_spade(x, gb)


# per level: the suffix of the reference's norm layer (batch_norm<suffix> / spade_layer<suffix>, architectures.py:423-436, 683-695) after
# encoder conv_i (i = 2..7) and decoder dconv_k (k = 1..7)
_MOTION_ENC_NORM = {2: "2_0", 3: "4_0", 4: "8_0", 5: "8_1", 6: "8_2", 7: "8_3"}
_MOTION_DEC_NORM = {1: "8_4", 2: "8_5", 3: "8_6", 4: "8_7", 5: "4_1", 6: "2_1", 7: ""}


class _MotionUnet(nn.Module):
    """The layers both motion U-Nets share (architectures.py:389-410, 612-633): conv1..conv8 4x4 / stride 2 (nf, 2nf, 4nf, 8nf x 5 output
    channels), dconv1..dconv8 3x3 (the last one onto ``cout`` channels)."""

    def __init__(self, cin, cout, nf, bn):
        super().__init__()
        self.cin = cin
        enc = [cin, nf, nf * 2, nf * 4, nf * 8, nf * 8, nf * 8, nf * 8, nf * 8]
        for i in range(1, 9):
            setattr(self, f"conv{i}", Conv4x4s2(enc[i - 1], enc[i]))
        dec = [(nf * 8, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 4), (nf * 8, nf * 2),
               (nf * 4, nf), (nf * 2, cout)]
        for k, (ci, co) in enumerate(dec, 1):
            setattr(self, f"dconv{k}", BNConv3x3(ci, co, bn=bn and k < 8))

    def _check_input(self, x):
        _check_motion_grid(x)
        if x.dim() != 4 or x.shape[1] != self.cin:
            raise ValueError(f"{type(self).__name__}: input [N, {self.cin}, H, W] expected, got {tuple(x.shape)}")


class Unet4Motion(_MotionUnet):
    """Unet4Motion (architectures.py:382-493) in eval mode with BatchNorm (norm_G 'sync:spectral_batch'): e1 = conv1(x),
    e_i = bn(conv_i(leaky_relu(e_{i-1}, 0.2))) for i = 2..7, e8 = conv8(leaky_relu(e7)); decoder
    d_k = bn(dconv_k(up(relu(cat(d_{k-1}, e_{9-k}))))) with all-bilinear x2 up-sampling (align_corners=False), out = dconv8(...) (no BN).
    The encoder's BNs ride in the 4x4 kernel's epilogue, the decoder's are folded into the 3x3 weights.  H, W multiples of 256."""

    def __init__(self, cin=3, cout=2, nf=32):
        super().__init__(cin, cout, nf, bn=True)
        for i, s in _MOTION_ENC_NORM.items():
            setattr(self, f"bn{s}", EvalBN(getattr(self, f"conv{i}").weight.shape[0]))

    @torch.no_grad()
    def forward(self, x):
        self._check_input(x)
        with fp32_kernels(winograd=False):
            e = [self.conv1(x)]
            for i in range(2, 9):
                e.append(getattr(self, f"conv{i}")(e[-1], leaky=0.2, bn=getattr(self, f"bn{_MOTION_ENC_NORM[i]}") if i < 8 else None))
            d = upsample2x_concat(e[7], None, -1, RELU_BEFORE)                       # up(relu(e8))
            for k in range(1, 8):
                d = upsample2x_concat(getattr(self, f"dconv{k}")(d), e[7 - k], -1, RELU_BEFORE)
            return self.dconv8(d)


class SPADEUnet4MaskMotion(_MotionUnet):
    """SPADEUnet4MaskMotion (architectures.py:602-743) with SPADE(InstanceNorm2d, C, 6) after conv2..conv7 and dconv1..dconv7, conditioned on
    the network input (RGB, mask, hint) resized to each level (mask nearest).  Decoder quirks reproduced: every x2 up-sampling is bilinear
    except channel 3 of each up-sampled tensor (nearest), feature map and skip alike; ReLU after up-sampling + concatenation, except for e8
    (ReLU first, :709-710).  The segmap branch needs the 6-channel input (mask + hint): with 3 channels the reference's SPADE does not resize
    its segmap, with 4 its mlp_shared (6 input channels) does not match -- both fail there, and raise here.  H, W multiples of 256."""

    def __init__(self, cin=6, cout=2, nf=32):
        if cin != 6:
            raise ValueError(f"SPADEUnet4MaskMotion: the SPADE segmap is the 6-channel input (RGB, mask, hint); got {cin} channels "
                             "(the reference fails for these too: its mlp_shared takes 6)")
        super().__init__(cin, cout, nf, bn=False)
        for i, s in _MOTION_ENC_NORM.items():
            setattr(self, f"spade_layer{s}", SPADEIN(getattr(self, f"conv{i}").weight.shape[0]))
        for k, s in _MOTION_DEC_NORM.items():
            setattr(self, f"spade_layer{s}", SPADEIN(getattr(self, f"dconv{k}").weight.shape[0]))

    @torch.no_grad()
    def forward(self, x):
        self._check_input(x)
        with fp32_kernels(winograd=False):
            seg = {k: resize_segmap(x, k) for k in range(1, 8)}                   # once per prediction, every level
            e = [self.conv1(x)]
            for i in range(2, 8):
                y = getattr(self, f"conv{i}")(e[-1], leaky=0.2)
                e.append(getattr(self, f"spade_layer{_MOTION_ENC_NORM[i]}")(y, seg[i]))
            e.append(self.conv8(e[-1], leaky=0.2))
            d = upsample2x_concat(e[7], None, 3, RELU_BEFORE)                        # relu(e8), then the mixed up-sampling
            for k in range(1, 8):
                d_ = getattr(self, f"spade_layer{_MOTION_DEC_NORM[k]}")(getattr(self, f"dconv{k}")(d), seg[8 - k])
                d = upsample2x_concat(d_, e[7 - k], 3, RELU_AFTER)
            return self.dconv8(d)


def _take(sd, used, key):
    used.add(key)
    return sd[key]


@torch.no_grad()
def load_motion_state_dict(net, sd, prefix):
    """Fill a motion U-Net from the reference's state dict of Unet4Motion / SPADEUnet4MaskMotion under ``prefix``
    ('model.module.motion_regressor.motion_predictor.' in an animating checkpoint trained with --train_motion,
    'model.module.motion_predictor.' in a motion checkpoint of train_motion_unet.py).  Spectral norm is folded at load (weight_orig /
    (u^T W v), no power iteration: its eval mode).  Every key under the prefix must be consumed, and every parameter found."""
    sub = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    if not sub:
        raise KeyError(f"no key of the state dict starts with {prefix!r}")
    used = set()

    def conv(mod, key):
        w = _fold_sn(sub, key)
        used.update(k for k in (key + ".weight", key + ".weight_orig", key + ".weight_u", key + ".weight_v") if k in sub)
        if tuple(w.shape) != tuple(mod.weight.shape):
            raise ValueError(f"{prefix}{key}: weight {tuple(w.shape)}, the network expects {tuple(mod.weight.shape)}")
        mod.weight.copy_(w)
        mod.bias.copy_(_take(sub, used, key + ".bias"))

    def bn(mod, key):
        for name in ("running_mean", "running_var", "weight", "bias"):
            getattr(mod, name).copy_(_take(sub, used, f"{key}.{name}"))
        if key + ".num_batches_tracked" in sub:
            used.add(key + ".num_batches_tracked")

    for i in range(1, 9):
        conv(getattr(net, f"conv{i}"), f"conv{i}")
        conv(getattr(net, f"dconv{i}"), f"dconv{i}")
    if isinstance(net, Unet4Motion):
        for s in _MOTION_ENC_NORM.values():
            bn(getattr(net, f"bn{s}"), f"batch_norm{s}")
        for k, s in _MOTION_DEC_NORM.items():
            bn(getattr(net, f"dconv{k}").bn, f"batch_norm{s}")
    else:
        for s in list(_MOTION_ENC_NORM.values()) + list(_MOTION_DEC_NORM.values()):
            sp = getattr(net, f"spade_layer{s}")
            key = f"spade_layer{s}"
            sp.mlp_shared.weight.copy_(_take(sub, used, key + ".mlp_shared.0.weight"))
            sp.mlp_shared.bias.copy_(_take(sub, used, key + ".mlp_shared.0.bias"))
            sp.mlp_gb.weight.copy_(torch.cat([_take(sub, used, key + ".mlp_gamma.weight"), _take(sub, used, key + ".mlp_beta.weight")]))
            sp.mlp_gb.bias.copy_(torch.cat([_take(sub, used, key + ".mlp_gamma.bias"), _take(sub, used, key + ".mlp_beta.bias")]))
    left = sorted(set(sub) - used)
    if left:
        raise KeyError(f"motion U-Net: {len(left)} key(s) under {prefix!r} not consumed (another norm / architecture?): {left[:6]}")
    return net
