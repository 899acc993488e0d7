"""The yardstick of the trainable generator networks (slr_sfs_amd.trainable, csrc/decoder_grad.hip): the decoder's first block with its
per-element mask k = (x != 0) (models/networks/architectures.py:369), ResNet_Block (models/layers/blocks.py:47-87) and the chains of
blocks WRITTEN OUT -- forward and every gradient, no autograd.  It extends block_train_f64.py / conv_train_f64.py and, like them, computes
in the dtype of its arguments: float64 is the reference, float32 on the CPU the "plain32" of the GPU tests' criterion.
tests/test_decoder_train_f64.py ties it to torch's float64 autograd.

Batch-norm with the per-element mask (normalization.py:319-354 with a [N,C,H,W] mask; gain, bias [N,C]):
    cnt[c] = sum_{n,h,w} k + eps,  m = sum x / cnt,  v = sum x^2 / cnt - m^2,  scale = rsqrt(v + eps) gain,  shift = m scale - bias,
    y = x scale - shift,  a = relu(y) k
Backward for ga at a: gy = ga k [y > 0]; s0, s1, dgain, dbias, P, Q, dv, dm as block_train_f64; dx = gy scale + dm / cnt + 2 dv x / cnt at
EVERY element, the zeros included (k is a constant of the graph, the statistics are sums over all of x).
Partial convolution behind it (partialconv2d.py:61-72 with a [N,Cin,H,W] mask), msum = sum_c k:
    box = box3x3(msum),  um = clamp(box, 0, 1),  ratio = 9 Cin / (box + 1e-8) um,  out = (conv(xm, w) ratio + b) um"""
import torch

import block_train_f64 as B64
import conv_train_f64 as C64

EPS = B64.EPS
_t = B64._t


def kept(x):
    return (x != 0).to(x.dtype)


# ------------------------------------------------------------------ batch-norm + ReLU + per-element mask

def bn_nz_stats(x, eps=EPS):
    """(mean [C], var [C], cnt [C])"""
    cnt = kept(x).sum((0, 2, 3)) + eps
    m = x.sum((0, 2, 3)) / cnt
    return m, (x * x).sum((0, 2, 3)) / cnt - m * m, cnt


def bn_nz_train(x, gain, bias, eps=EPS, stored=None):
    """(a, mean, var, msum)"""
    mean, var = stored if stored is not None else bn_nz_stats(x, eps)[:2]
    scale, shift = B64.bn_tables(mean, var, gain, bias, eps)
    k = kept(x)
    return torch.relu(x * _t(scale) - _t(shift)) * k, mean, var, k.sum(1, keepdim=True)


def bn_nz_train_grads(x, gain, bias, ga, eps=EPS, stored=None, addend=None):
    """(dx, dgain, dbias) for the gradient ga at a."""
    if stored is not None:
        m, v = stored
    else:
        m, v, cnt = bn_nz_stats(x, eps)
    scale, shift = B64.bn_tables(m, v, gain, bias, eps)
    y = x * _t(scale) - _t(shift)
    gy = torch.where((y <= 0) | (x == 0), torch.zeros_like(ga), ga)     # (torch's ReLU backward: a select, closed on `<= 0` only)
    rs = torch.rsqrt(v + eps)
    s0, s1 = gy.sum((2, 3)), (gy * x).sum((2, 3))
    dbias, dgain = s0, rs[None] * (s1 - m[None] * s0)
    dx = gy * _t(scale)
    if stored is None:
        P, Q = (gain * s0).sum(0), (gain * s1).sum(0)
        dv = -0.5 * rs ** 3 * (Q - m * P)
        dm = -rs * P - 2.0 * m * dv
        dx = dx + (dm / cnt)[None, :, None, None] + (2.0 * dv / cnt)[None, :, None, None] * x
    return (dx if addend is None else dx + addend), dgain, dbias


# ------------------------------------------------------------------ the partial convolution of a count plane

def partial_factors_counts(msum, cin):
    """(ratio, um, r = ratio * um), each [N,1,H,W]."""
    box = sum(C64.shifted(msum, ky - 1, kx - 1) for ky, kx in C64.TAPS)
    um = box.clamp(0, 1)
    ratio = (9.0 * cin) / (box + 1e-8) * um
    return ratio, um, ratio * um


def pconv_counts(xm, msum, w, b, residual=None):
    """(out, update_mask)"""
    ratio, um, _ = partial_factors_counts(msum, xm.shape[1])
    out = (C64.conv(xm, w) * ratio + b.view(1, -1, 1, 1)) * um
    return (out if residual is None else out + residual), um


def pconv_counts_grads(xm, msum, w, g):
    """(dxm, dW, db) for the gradient g at out (the gradient at a residual is g itself)."""
    _, um, r = partial_factors_counts(msum, xm.shape[1])
    gr = g * r
    return C64.conv_dx(gr, w), C64.conv_dw(xm, gr), C64.conv_db(g * um)


# ------------------------------------------------------------------ the decoder's first block

def input_block(x, p, kind, gains, biases, eps=EPS, stored=None):
    """ResNet_Block_Pconv2.forward called with mask = (x != 0) (architectures.py:369); arguments and result as block_train_f64.block."""
    st1, st2 = stored if stored is not None else (None, None)
    a1, m1, v1, msum = bn_nz_train(x, gains[0], biases[0], eps, st1)
    o1, um1 = pconv_counts(a1, msum, p["w_aa"], p["b_aa"])
    a2, m2, v2 = B64.bn_train(o1, um1, gains[1], biases[1], eps, st2)
    o2, um2 = C64.pconv(a2, um1, p["w_ab"], p["b_ab"])
    skip = B64.conv1x1(x, p["w_b"]) if p.get("w_b") is not None else x
    return dict(y=B64.resample(o2, kind) + B64.resample(skip, kind), um=B64.resample_mask(um2, kind), mean1=m1, var1=v1, mean2=m2, var2=v2,
                a1=a1, msum=msum, o1=o1, um1=um1, a2=a2)


def input_block_grads(x, p, kind, gains, biases, g, eps=EPS, stored=None):
    st1, st2 = stored if stored is not None else (None, None)
    f = input_block(x, p, kind, gains, biases, eps, stored)
    gs = B64.resample_adjoint(g, kind, x.shape[2], x.shape[3])
    da2, dw_ab, db_ab = C64.pconv_grads(f["a2"], f["um1"], p["w_ab"], gs)
    do1, dgain2, dbias2 = B64.bn_train_grads(f["o1"], f["um1"], gains[1], biases[1], da2, eps, st2)
    da1, dw_aa, db_aa = pconv_counts_grads(f["a1"], f["msum"], p["w_aa"], do1)
    has_b = p.get("w_b") is not None
    dskip = B64.conv1x1_dx(gs, p["w_b"]) if has_b else gs
    dx, dgain1, dbias1 = bn_nz_train_grads(x, gains[0], biases[0], da1, eps, st1, addend=dskip)
    return dict(dx=dx, dgain1=dgain1, dbias1=dbias1, dgain2=dgain2, dbias2=dbias2, dw_aa=dw_aa, db_aa=db_aa, dw_ab=dw_ab, db_ab=db_ab,
                dw_b=B64.conv1x1_dw(x, gs) if has_b else None, db_aa_terms=C64.conv_db((do1 * f["um1"]).abs()),
                db_ab_terms=C64.conv_db((gs * C64.partial_factors(f["um1"], f["a2"].shape[1])[1]).abs()))


# ------------------------------------------------------------------ ResNet_Block

def res_block(x, p, kind, gains, biases, eps=EPS, stored=None):
    """ResNet_Block.forward (blocks.py:47-87).  p: w_aa, b_aa, w_ab, b_ab, w_b, b_b (w_b None: identity skip)."""
    st1, st2 = stored if stored is not None else (None, None)
    a1, m1, v1 = B64.bn_train(x, None, gains[0], biases[0], eps, st1)
    o1 = C64.conv(a1, p["w_aa"], p["b_aa"])
    a2, m2, v2 = B64.bn_train(o1, None, gains[1], biases[1], eps, st2)
    o2 = C64.conv(a2, p["w_ab"], p["b_ab"])
    skip = B64.conv1x1(x, p["w_b"], p["b_b"]) if p.get("w_b") is not None else x
    return dict(y=B64.resample(o2, kind) + B64.resample(skip, kind), mean1=m1, var1=v1, mean2=m2, var2=v2, a1=a1, o1=o1, a2=a2)


def res_block_grads(x, p, kind, gains, biases, g, eps=EPS, stored=None):
    st1, st2 = stored if stored is not None else (None, None)
    f = res_block(x, p, kind, gains, biases, eps, stored)
    gs = B64.resample_adjoint(g, kind, x.shape[2], x.shape[3])
    da2, dw_ab, db_ab = C64.conv_dx(gs, p["w_ab"]), C64.conv_dw(f["a2"], gs), C64.conv_db(gs)
    do1, dgain2, dbias2 = B64.bn_train_grads(f["o1"], None, gains[1], biases[1], da2, eps, st2)
    da1, dw_aa, db_aa = C64.conv_dx(do1, p["w_aa"]), C64.conv_dw(f["a1"], do1), C64.conv_db(do1)
    has_b = p.get("w_b") is not None
    dskip = B64.conv1x1_dx(gs, p["w_b"]) if has_b else gs
    dx, dgain1, dbias1 = B64.bn_train_grads(x, None, gains[0], biases[0], da1, eps, st1, addend=dskip)
    return dict(dx=dx, dgain1=dgain1, dbias1=dbias1, dgain2=dgain2, dbias2=dbias2, dw_aa=dw_aa, db_aa=db_aa, dw_ab=dw_ab, db_ab=db_ab,
                dw_b=B64.conv1x1_dw(x, gs) if has_b else None, db_b=C64.conv_db(gs) if has_b else None,
                db_aa_terms=C64.conv_db(do1.abs()), db_ab_terms=C64.conv_db(gs.abs()))


# ------------------------------------------------------------------ the chains

def decoder(x, ps, kinds, gains, biases, eps=EPS, stored=None):
    """ResNetDecoderPconv2.forward (architectures.py:345-375): block 0 with (x != 0), the others with the update mask.  ps / kinds /
    gains / biases / stored: one entry per block.  Returns the blocks' dicts (the last one's y is the output)."""
    fs, mask = [], None
    for i, p in enumerate(ps):
        st = None if stored is None else stored[i]
        f = input_block(x, p, kinds[i], gains[i], biases[i], eps, st) if i == 0 else B64.block(x, mask, p, kinds[i], gains[i], biases[i], eps, st)
        f["x"], f["mask"] = x, mask
        fs.append(f)
        x, mask = f["y"], f["um"]
    return fs


def decoder_grads(x, ps, kinds, gains, biases, g, eps=EPS):
    """The blocks' gradient dicts for the gradient g at the output (the first one's dx is the gradient at x)."""
    fs = decoder(x, ps, kinds, gains, biases, eps)
    ds = [None] * len(ps)
    for i in reversed(range(len(ps))):
        f = fs[i]
        if i == 0:
            d = input_block_grads(f["x"], ps[i], kinds[i], gains[i], biases[i], g, eps)
        else:
            d = B64.block_grads(f["x"], f["mask"], ps[i], kinds[i], gains[i], biases[i], g, eps)
            gs = B64.resample_adjoint(g, kinds[i], f["x"].shape[2], f["x"].shape[3])
            d["db_ab_terms"] = C64.conv_db((gs * C64.partial_factors(f["um1"], f["a2"].shape[1])[1]).abs())
        ds[i], g = d, d["dx"]
    return fs, ds


def encoder(x, ps, kinds, gains, biases, eps=EPS, stored=None):
    """A chain of ResNet_Blocks (ResNetEncoder_with_Z / ResNetEncoder / ResNetBGDecoder, architectures.py:121-260)."""
    fs = []
    for i, p in enumerate(ps):
        f = res_block(x, p, kinds[i], gains[i], biases[i], eps, None if stored is None else stored[i])
        f["x"] = x
        fs.append(f)
        x = f["y"]
    return fs


def encoder_grads(x, ps, kinds, gains, biases, g, eps=EPS):
    fs = encoder(x, ps, kinds, gains, biases, eps)
    ds = [None] * len(ps)
    for i in reversed(range(len(ps))):
        ds[i] = res_block_grads(fs[i]["x"], ps[i], kinds[i], gains[i], biases[i], g, eps)
        g = ds[i]["dx"]
    return fs, ds


# ------------------------------------------------------------------ inputs

def keep_pattern(N, C, H, W, seed, zero_channel=True):
    """[N,C,H,W] of 0 / 1: whole-pixel holes (conv_train_f64.holed_mask), about 10 % single-element zeros, channel 1 zero in image 0 and
    (zero_channel) channel 0 zero everywhere -- its cnt is eps and m = v = 0."""
    g = torch.Generator().manual_seed(seed)
    keep = C64.holed_mask(N, H, W, seed).expand(N, C, H, W) * (torch.rand(N, C, H, W, generator=g) > 0.1).float()
    if C > 1:
        keep[0, 1] = 0.0
    if zero_channel:
        keep[:, 0] = 0.0
    return keep


def gate_margin_nz(x, gain, bias, eps=EPS, stored=None):
    """min |y| of the float64 pre-activation over the KEPT elements (a zero element's gate is multiplied by k = 0)."""
    x, gain, bias = x.double(), gain.double(), bias.double()
    mean, var = (t.double() for t in stored) if stored is not None else bn_nz_stats(x, eps)[:2]
    scale, shift = B64.bn_tables(mean, var, gain, bias, eps)
    y = (x * _t(scale) - _t(shift)).abs()
    return float(y[x != 0].min())


def nudged_nz(x, gain, bias, eps=EPS, margin=1e-4, stored=None):
    """block_train_f64.nudged for the per-element mask: only kept elements move, and none of them onto zero; zeros stay exact zeros."""
    x = x.clone()
    zero = x == 0
    for _ in range(64):
        xd = x.double()
        mean, var = (t.double() for t in stored) if stored is not None else bn_nz_stats(xd, eps)[:2]
        scale, shift = B64.bn_tables(mean, var, gain.double(), bias.double(), eps)
        y = xd * _t(scale) - _t(shift)
        bad = (y.abs() < 1.5 * margin) & ~zero
        if not bad.any():
            break
        step = (8 * margin / _t(scale).abs().clamp_min(1e-3)).expand_as(xd)
        x[bad] = (xd + torch.where(y >= 0, step, -step) * torch.sign(_t(scale)))[bad].float()
    assert torch.equal(x == 0, zero) and gate_margin_nz(x, gain, bias, eps, stored) > margin
    return x


# ------------------------------------------------------------------ the reference fixture's parameters and number format

def fixture_param(case, key, shape):
    """The float32-valued parameter ``key`` of fixture case ``case``: seeded by its name, so that the fixture need not store it.  Noise
    layers 0.1 / 0.2 sigma (gains and biases differ per sample), convolution biases 0.3, weights 1 / sqrt(fan-in)."""
    import zlib
    gen = torch.Generator().manual_seed(zlib.crc32(f"{case}/{key}".encode()))
    scale = 0.1 if key.endswith("gain.weight") else 0.2 if key.endswith("bias.weight") else 0.3 if key.endswith(".bias") else \
        1.0 / float(shape[1] * shape[2] * shape[3]) ** 0.5
    return torch.randn(*shape, generator=gen, dtype=torch.float32) * scale


def packed(name, v):
    """npz entries of array v.  float64 arrays become a float32 part and an int16 correction with one scale per array: 6 bytes per
    element, the error at most max|v| 2^-24 / 65534 ~ 1e-12 max|v| -- the measure E divides by max|ref|."""
    import numpy as np
    if v.dtype != np.float64 or v.size < 64:
        return {name: v}
    hi = v.astype(np.float32)
    rest = v - hi.astype(np.float64)
    scale = max(float(np.abs(rest).max()), 1e-300) / 32767.0
    return {name + "#hi": hi, name + "#lo": np.round(rest / scale).astype(np.int16), name + "#scale": np.float64(scale)}


def load_packed(path):
    """{name: torch tensor} of a file written with ``packed``, with the parameters ``fixture_param`` regenerates."""
    import numpy as np
    g = np.load(path)
    out = {}
    for k in g.files:
        if k.endswith("#hi"):
            n = k[:-3]
            out[n] = torch.from_numpy(g[k].astype(np.float64) + g[n + "#lo"].astype(np.float64) * float(g[n + "#scale"]))
        elif "#" not in k:
            out[k] = torch.from_numpy(g[k])
    for k in [k for k in out if "/d/" in k]:             # the parameter a gradient belongs to: regenerated, not stored
        case, key = k.split("/d/")
        out[f"{case}/p/{key}"] = fixture_param(case, key, out[k].shape)
    return out
