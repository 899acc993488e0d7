"""The yardstick of the trainable decoder block (slr_sfs_amd.trainable, csrc/block_grad.hip): every operator of ResNet_Block_Pconv2 in
training mode (models/layers/blocks.py:218-248 with the partial batch-norm of models/layers/normalization.py:19-52, 256-354) and the block
itself WRITTEN OUT -- forward and every gradient, no autograd.  The functions compute in the dtype of their arguments: float64 is the
reference, the same code in float32 on the CPU is the "plain32" of the GPU tests' criterion.  tests/test_block_train_f64.py ties them to
torch's float64 autograd and to the reference's own block (tests/golden/block_train_vs_reference.npz).

Batch-norm (mask [N,1,H,W] channel-uniform or None; gain, bias [N,C]):
    cnt = sum(mask) + eps (partial_manual_bn) or N H W (manual_bn),  m = sum x / cnt,  v = sum x^2 / cnt - m^2   (sums over ALL elements)
    scale = rsqrt(v + eps) gain,  shift = m scale - bias,  y = x scale - shift,  a = relu(y) mask
Backward for the gradient ga at a, gy = ga mask [y > 0], rs = (v + eps)^-1/2, s0 = sum_hw gy, s1 = sum_hw gy x per (n, c):
    dbias = s0,  dgain = rs (s1 - m s0),  P = sum_n gain s0,  Q = sum_n gain s1,  dv = -rs^3 (Q - m P) / 2,  dm = -rs P - 2 m dv,
    dx = gy scale + dm / cnt + 2 dv x / cnt              (stored statistics: dm = dv = 0)"""
import torch

import conv_train_f64 as C64

E = C64.E
EPS = 1e-5


def _t(v):
    return v[:, :, None, None]


# ------------------------------------------------------------------ batch-norm + ReLU + mask

def bn_stats(x, mask, eps=EPS):
    """(mean [C], var [C], cnt)"""
    N, C, H, W = x.shape
    cnt = float(N * H * W) if mask is None else mask.sum() + eps
    m = x.sum((0, 2, 3)) / cnt
    return m, (x * x).sum((0, 2, 3)) / cnt - m * m, cnt


def bn_tables(mean, var, gain, bias, eps=EPS):
    scale = torch.rsqrt(var + eps)[None] * gain
    return scale, mean[None] * scale - bias


def bn_gate(x, scale, shift, mask):
    y = x * _t(scale) - _t(shift)
    a = torch.relu(y)
    return y, (a if mask is None else a * mask)


def bn_train(x, mask, gain, bias, eps=EPS, stored=None):
    """(a, mean, var); stored = (mean, var) selects stored statistics."""
    mean, var = stored if stored is not None else bn_stats(x, mask, eps)[:2]
    scale, shift = bn_tables(mean, var, gain, bias, eps)
    return bn_gate(x, scale, shift, mask)[1], mean, var


def bn_train_grads(x, mask, gain, bias, ga, eps=EPS, stored=None, addend=None):
    """(dx, dgain, dbias) for the gradient ga at a."""
    if stored is not None:
        m, v = stored
    else:
        m, v, cnt = bn_stats(x, mask, eps)
    scale, shift = bn_tables(m, v, gain, bias, eps)
    y = bn_gate(x, scale, shift, mask)[0]
    gm = ga if mask is None else ga * mask
    gy = torch.where(y <= 0, torch.zeros_like(gm), gm)   # (torch's ReLU backward: a select, closed on `<= 0` only -- a NaN arriving at a
                                                         #  closed gate stops, a NaN pre-activation leaves the gate open)
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


# ------------------------------------------------------------------ 1x1 convolution

def conv1x1(x, w, b=None):
    out = torch.einsum("nchw,oc->nohw", x, w[:, :, 0, 0])
    return out if b is None else out + b.view(1, -1, 1, 1)


def conv1x1_dw(x, g):
    return torch.einsum("nohw,nchw->oc", g, x)[:, :, None, None]


def conv1x1_dx(g, w):
    return torch.einsum("nohw,oc->nchw", g, w[:, :, 0, 0])


# ------------------------------------------------------------------ resampling: both are separable, out = R_H x R_W^T

def resample_matrix(kind, size, dtype):
    """[out, size]: nn.AvgPool2d(3, 2, 1) (count_include_pad: every tap weighs 1/3 per axis) or x2 bilinear, align_corners=False
    (src = max((o + 0.5) / 2 - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, size - 1), l1 = src - i0)."""
    if kind == "Down":
        R = torch.zeros((size - 1) // 2 + 1, size, dtype=dtype)
        for o in range(R.shape[0]):
            for i in (2 * o - 1, 2 * o, 2 * o + 1):
                if 0 <= i < size:
                    R[o, i] = 1.0
        return R / 3.0
    R = torch.zeros(2 * size, size, dtype=dtype)
    for o in range(2 * size):
        src = max((o + 0.5) * 0.5 - 0.5, 0.0)
        i0 = int(src)
        i1 = min(i0 + 1, size - 1)
        R[o, i0] += 1.0 - (src - i0)
        R[o, i1] += src - i0
    return R


def resample(x, kind):
    if not kind:
        return x
    return torch.einsum("ah,nchw,bw->ncab", resample_matrix(kind, x.shape[2], x.dtype), x, resample_matrix(kind, x.shape[3], x.dtype))


def resample_adjoint(g, kind, H, W):
    """The gradient at the input [.,.,H,W] of ``resample`` for the gradient g at its output."""
    if not kind:
        return g
    return torch.einsum("ah,ncab,bw->nchw", resample_matrix(kind, H, g.dtype), g, resample_matrix(kind, W, g.dtype))


def resample_mask(m, kind):
    """nn.MaxPool2d(3, 2, 1) / nearest x2 of a 0 / 1 mask."""
    if kind == "Down":
        return (resample(m, "Down") > 0).to(m.dtype)
    if kind == "Up":
        return m.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return m


# ------------------------------------------------------------------ the block

def block(x, mask, p, kind, gains, biases, eps=EPS, stored=None):
    """ResNet_Block_Pconv2.forward (pconv_pbn_woresbias).  p: w_aa, b_aa, w_ab, b_ab, w_b (None: identity skip); gains / biases: the
    two BNs' [N,C] tables; stored: ((mean1, var1), (mean2, var2)) for eval mode.  Returns a dict with y, um and the batch statistics."""
    st1, st2 = stored if stored is not None else (None, None)
    a1, m1, v1 = bn_train(x, mask, gains[0], biases[0], eps, st1)
    o1, um1 = C64.pconv(a1, mask, p["w_aa"], p["b_aa"])
    a2, m2, v2 = bn_train(o1, um1, gains[1], biases[1], eps, st2)
    o2, um2 = C64.pconv(a2, um1, p["w_ab"], p["b_ab"])
    skip = conv1x1(x, p["w_b"]) if p.get("w_b") is not None else x
    return dict(y=resample(o2, kind) + resample(skip, kind), um=resample_mask(um2, kind), mean1=m1, var1=v1, mean2=m2, var2=v2,
                a1=a1, o1=o1, um1=um1, a2=a2)


def block_grads(x, mask, p, kind, gains, biases, g, eps=EPS, stored=None):
    """Every gradient of ``block`` for the gradient g at y, by the written-out backward formulas."""
    st1, st2 = stored if stored is not None else (None, None)
    f = block(x, mask, p, kind, gains, biases, eps, stored)
    gs = resample_adjoint(g, kind, x.shape[2], x.shape[3])
    da2, dw_ab, db_ab = C64.pconv_grads(f["a2"], f["um1"], p["w_ab"], gs)
    do1, dgain2, dbias2 = bn_train_grads(f["o1"], f["um1"], gains[1], biases[1], da2, eps, st2)
    da1, dw_aa, db_aa = C64.pconv_grads(f["a1"], mask, p["w_aa"], do1)
    has_b = p.get("w_b") is not None
    dskip = conv1x1_dx(gs, p["w_b"]) if has_b else gs
    dx, dgain1, dbias1 = bn_train_grads(x, mask, gains[0], biases[0], da1, eps, st1, addend=dskip)
    return dict(dx=dx, dgain1=dgain1, dbias1=dbias1, dgain2=dgain2, dbias2=dbias2, dw_aa=dw_aa, db_aa=db_aa, dw_ab=dw_ab, db_ab=db_ab,
                dw_b=conv1x1_dw(x, gs) if has_b else None, db_aa_terms=C64.conv_db((do1 * f["um1"]).abs()))


def E_terms(got, ref, terms):
    """The error of a sum against the magnitude of its terms: max|got - ref| / max(sum of |terms|).  For conv_aa's bias gradient with batch
    statistics: the BN behind it removes a constant per channel (o1 = (raw ratio + b) um is zero in the holes and the count is
    sum(um) + eps), so db_aa = sum_{n,p} do1 um cancels to O(eps / count) of its terms -- 1e-6 here, where two float64 evaluations in
    different orders already differ by 1e-9 of the result.  Against the terms the figure means what E means for every other tensor."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((got - ref).abs().max() / torch.as_tensor(terms).double().max())


# ------------------------------------------------------------------ inputs

def gate_margin(x, mask, gain, bias, eps=EPS, stored=None):
    """min |y| of the float64 pre-activation over all elements."""
    x, gain, bias = x.double(), gain.double(), bias.double()
    mean, var = (t.double() for t in stored) if stored is not None else bn_stats(x, None if mask is None else mask.double(), eps)[:2]
    y = bn_gate(x, *bn_tables(mean, var, gain, bias, eps), None)[0].abs()
    return float(y.min())


def nudged(x, mask, gain, bias, eps=EPS, margin=1e-4, stored=None):
    """x (float32) with the elements whose float64 pre-activation lies within ``margin`` of zero moved away, so that the ReLU gate of
    every arithmetic agrees; the statistics move with x, hence the loop.  Asserts the property."""
    x = x.clone()
    for _ in range(64):
        xd = x.double()
        mean, var = (t.double() for t in stored) if stored is not None else bn_stats(xd, None if mask is None else mask.double(), eps)[:2]
        scale, shift = bn_tables(mean, var, gain.double(), bias.double(), eps)
        y = xd * _t(scale) - _t(shift)
        bad = y.abs() < 1.5 * margin
        if not bad.any():
            break
        step = (8 * margin / _t(scale).abs().clamp_min(1e-3)).expand_as(xd)
        x[bad] = (xd + torch.where(y >= 0, step, -step) * torch.sign(_t(scale)))[bad].float()
    assert gate_margin(x, mask, gain, bias, eps, stored) > margin
    return x


def holed(x, mask, gen):
    """x as a partial block sees it: (nearly) zero where the mask is 0 -- the sums run over ALL elements but the count over the mask, so
    with the full-size values of x in the holes m2 - m^2 goes negative.  The holes keep small values (1e-3 sigma: with few valid pixels larger ones turn
    the variance negative here, too): a sum that skipped them would still be off by ~1e-4."""
    return x * mask + 1e-3 * torch.randn(x.shape, generator=gen, dtype=x.dtype) * (1 - mask)


def bn_inputs(N, C, H, W, seed, mask=None):
    """x with per-channel means up to ~3 and standard deviations 0.5 .. 2 (sum x^2 - (sum x)^2 has something to cancel), ``holed`` by
    ``mask``, per-sample gains and biases, an incoming gradient that is constant in no direction."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                              # noqa: E731
    mu, sd = 3.0 * (2 * torch.rand(C, generator=g) - 1), 0.5 + 1.5 * torch.rand(C, generator=g)
    x = r(N, C, H, W) * sd[None, :, None, None] + mu[None, :, None, None]
    if mask is not None:
        x = holed(x, mask, g)
    gain, bias = 1.0 + 0.3 * r(N, C), 0.5 * r(N, C)
    ga = r(N, C, H, W) * (1.0 + torch.arange(W) / W)
    return x, gain, bias, ga
