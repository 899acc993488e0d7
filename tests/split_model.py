"""The CPU definition of the split-f16 convolutions (csrc/conv.hip: the default arithmetic of every 3x3 and 1x1 decoder convolution), WRITTEN OUT
in plain torch: what the kernels document, nothing they do not.

    v  = clamp(x * xscale, -65472, 65472)            fp32; xscale a power of two (nets.activation_scale)
    hi = f16(v),  lo = f16(v - hi)                   round to nearest even, f16 subnormals KEPT (``flush=False``)
    ww = w * wscale(w), split the same way           wscale(w) = 2 ** floor(log2(4096 / max|w|))   (nets.Conv._split_weights)
    out = (hi*hi + hi*lo + lo*hi, summed over taps and input channels) / (xscale * wscale)

A product of two halves has at most 22 significant bits: it is exact in fp32, so the ONLY thing a kernel may legitimately do differently from
this model is the order and precision (fp32) of the accumulation.  ``acc=torch.float64`` is the model (E_model of the tests),
``acc=torch.float32`` stands in for a kernel's accumulation (tests/test_split_model.py keeps it inside the bound the GPU tests use).

``flush=True`` is the same arithmetic on hardware that treats f16 subnormals (|half| < 2^-14) as zero: a half that is subnormal after the
conversion counts as 0.  (Flushing in the conversion or at the matrix instruction's inputs gives the same halves: a value whose hi half is
flushed is itself below 2^-14, so its lo half is flushed with it.)

The error measures have NO floor: E = max|a - ref| / max|ref|, per tensor or per output channel -- a layer whose outputs are 1e-4 is judged
on the scale of 1e-4.  tests/conv_train_f64.py holds the plain convolution (float64: the reference; float32: "plain32")."""
import math

import torch

import conv_train_f64 as cf

F16_MAX_SPLIT = 65472.0                     # the clamp of stage_value (csrc/conv.hip)
F16_MIN_NORMAL = 2.0 ** -14


def split(v, flush=False):
    """(hi, lo) of the fp32 tensor ``v``, as float16 tensors: hi = f16(v), lo = f16(v - hi), both rounded to nearest even with subnormals kept;
    ``flush``: halves below 2^-14 in magnitude are zero."""
    v = v.float()
    hi = v.half()
    lo = (v - hi.float()).half()                       # v - hi is exact in fp32
    if flush:
        hi = torch.where(hi.float().abs() < F16_MIN_NORMAL, torch.zeros_like(hi), hi)
        lo = torch.where(lo.float().abs() < F16_MIN_NORMAL, torch.zeros_like(lo), lo)
    return hi, lo


def wscale(w):
    """nets.Conv._split_weights' rule: the largest power of two that keeps max|w| * wscale <= 4096."""
    amax = float(w.abs().max())
    return 2.0 ** math.floor(math.log2(4096.0 / amax)) if amax > 0 else 1.0


def split_activations(x, xscale, flush=False):
    return split((x.float() * xscale).clamp(-F16_MAX_SPLIT, F16_MAX_SPLIT), flush)


def plain(x, w, k):
    """The convolution itself in the dtype of its arguments: k = 3 (stride 1, zero pad 1, nine taps written out) or k = 1."""
    return cf.conv(x, w) if k == 3 else torch.einsum("nchw,oc->nohw", x, w[:, :, 0, 0])


def conv(x, w, xscale, k, flush=False, acc=torch.float64):
    """The split-f16 convolution of fp32 ``x`` [N,Cin,H,W] with fp32 ``w`` [Cout,Cin,k,k] at activation scale ``xscale``: three products per
    operand pair, accumulated in ``acc``, unscaled (exactly: powers of two).  No bias."""
    ws = wscale(w)
    xh, xl = (t.to(acc) for t in split_activations(x, xscale, flush))
    wh, wl = (t.to(acc) for t in split(w.float() * ws, flush))
    out = plain(xh, wh, k) + plain(xh, wl, k) + plain(xl, wh, k)
    return out * (1.0 / (xscale * ws))


def E(a, ref):
    """max|a - ref| / max|ref| over the tensor, in float64.  No floor."""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((a - ref).abs().max() / ref.abs().max())


def E_per_channel(a, ref):
    """E of every output channel on that channel's own scale: float64 [Cout].  No floor."""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return (a - ref).abs().amax((0, 2, 3)) / ref.abs().amax((0, 2, 3))


# ---- the inputs the CPU test and the GPU tests share

SHAPES_3X3 = [(16, 32, 8, 32), (32, 64, 9, 33), (64, 128, 16, 40)]            # (Cin, Cout, H, W): the 32- / 64- / 128-channel workgroups
SHAPES_1X1 = [(64, 128, 9, 33), (3, 32, 7, 19)]
SHAPE_FEW = (64, 3, 9, 33)                                                    # the <= 4-channel kernel: fp32 FMAs, a control
BATCH = 2
MAGNITUDES = [1.0, 2.0 ** -4, 2.0 ** -8, 2.0 ** -12, 2.0 ** -16, 2.0 ** -20]
TOP = {64.0: 2.0 ** 7, 1.0: 2.0 ** 13}                                       # the largest magnitude of a sweep, by activation scale


def magnitudes(xscale):
    return [TOP[float(xscale)]] + MAGNITUDES


def seeded(cin, cout, h, w, k, seed=0):
    """(base [BATCH,cin,h,w] ~ N(0, 1), weights [cout,cin,k,k] ~ N(0, 1 / (cin k k))) -- the initialisation of nets.Conv."""
    g = torch.Generator().manual_seed(1000 * cin + 10 * h + k + seed)
    base = torch.randn(BATCH, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    return base, wt


def probe_values(xscale, signed=True):
    """The exact probes, as x * xscale, by class: A lo half normal; B lo half subnormal; C hi half subnormal; D rounds to 0;
    E (activation scale 64 only: 1000.125 * 64 < 65472) large with a normal lo half.  -> (values x, their classes), negatives included
    when ``signed``."""
    table = [("A", 1.0 + 2.0 ** -10 + 2.0 ** -12), ("B", 1.0 + 2.0 ** -18), ("C", 3.0 * 2.0 ** -20), ("C", 2.0 ** -24), ("D", 2.0 ** -26)]
    if xscale == 64.0:
        table.append(("E", (1000.0 + 2.0 ** -3) * 64.0))
    vals, classes = [], []
    for cls, v in table:
        for sgn in ((1.0, -1.0) if signed else (1.0,)):
            vals.append(sgn * v / xscale)
            classes.append(cls)
    return torch.tensor(vals, dtype=torch.float32), classes


def probe_tensor(cin, h, w, xscale, signed=True):
    """(x [BATCH,cin,h,w] tiled with the probe values, index [cin,h,w] into them, classes)."""
    vals, classes = probe_values(xscale, signed)
    c, y, xx = torch.meshgrid(torch.arange(cin), torch.arange(h), torch.arange(w), indexing="ij")
    idx = (7 * c + 3 * y + xx) % len(vals)
    return vals[idx].unsqueeze(0).repeat(BATCH, 1, 1, 1).contiguous(), idx, classes


def centre_identity(cin, cout, k, value=1.0):
    """w[c, c, centre] = value, everything else 0."""
    wt = torch.zeros(cout, cin, k, k)
    for c in range(min(cin, cout)):
        wt[c, c, k // 2, k // 2] = value
    return wt
