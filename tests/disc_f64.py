"""The adversarial loss written out, without autograd: the multiscale PatchGAN discriminator of the reference's trainer
(models/networks/discriminators.py, models/losses/gan_loss.py, models/layers/normalization.py:95-130 "spectralinstance") forward and
backward in whatever dtype its inputs have -- float64 as the reference of the tests, float32 as the plain-fp32 yardstick E_plain32.

Convolutions (4x4, stride 1 / 2, padding 2: forward, backward-data, weight gradient), instance norm + LeakyReLU, spectral normalisation
with its gradient and the updated u / v, the counted 3x3 / stride 2 average pool and its gradient, and both steps' losses with the
gradient to the fake image and to every parameter.  tests/test_disc_f64.py ties all of it to torch autograd and to the reference's own
classes (tests/golden/disc_vs_reference.npz)."""
import zlib

import torch
import torch.nn.functional as F

SLOPE, EPS, SN_EPS = 0.2, 1e-5, 1e-12
STRIDES = (2, 2, 2, 1, 1)                     # model0 .. model4 (n_layers_D = 4)


def out_size(H, s):
    return H // s + 1                         # (H + 2 * 2 - 4) / s + 1


def leaky(x):
    return torch.where(x > 0, x, x * SLOPE)


def leaky_gate(x):
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, SLOPE))


# ---------------------------------------------------------------------------------------------- the 4x4 convolution

def _taps(H, W, s):
    OH, OW = out_size(H, s), out_size(W, s)
    for ky in range(4):
        for kx in range(4):
            yield ky, kx, slice(ky, ky + s * (OH - 1) + 1, s), slice(kx, kx + s * (OW - 1) + 1, s)


def conv_forward(x, w, b, s):
    N, _, H, W = x.shape
    xp = F.pad(x, (2, 2, 2, 2))
    out = x.new_zeros(N, w.shape[0], out_size(H, s), out_size(W, s))
    for ky, kx, ys, xs in _taps(H, W, s):
        out += torch.einsum("nchw,oc->nohw", xp[:, :, ys, xs], w[:, :, ky, kx])
    return out if b is None else out + b.view(1, -1, 1, 1)


def conv_backward_data(g, w, s, H, W):
    gp = g.new_zeros(g.shape[0], w.shape[1], H + 4, W + 4)
    for ky, kx, ys, xs in _taps(H, W, s):
        gp[:, :, ys, xs] += torch.einsum("nohw,oc->nchw", g, w[:, :, ky, kx])
    return gp[:, :, 2:2 + H, 2:2 + W].contiguous()


def conv_weight_grad(x, g, s):
    N, _, H, W = x.shape
    xp = F.pad(x, (2, 2, 2, 2))
    dw = x.new_zeros(g.shape[1], x.shape[1], 4, 4)
    for ky, kx, ys, xs in _taps(H, W, s):
        dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, xp[:, :, ys, xs])
    return dw, g.sum((0, 2, 3))


# ---------------------------------------------------------------------------------------------- instance norm + LeakyReLU

def instnorm_lrelu_forward(x, eps=EPS):
    m = x.mean((2, 3), keepdim=True)
    d = x - m
    rstd = 1.0 / torch.sqrt((d * d).mean((2, 3), keepdim=True) + eps)
    xh = d * rstd
    return leaky(xh), xh, rstd


def instnorm_lrelu_backward(gy, xh, rstd):
    gh = gy * leaky_gate(xh)
    return rstd * (gh - gh.mean((2, 3), keepdim=True) - xh * (gh * xh).mean((2, 3), keepdim=True))


def instnorm_margin(x, eps=EPS):
    return float(instnorm_lrelu_forward(x.double(), eps)[1].abs().min())


def nudged(x, margin=1e-4, eps=EPS):
    """x (float32) with the elements whose float64 x-hat lies within ``margin`` of zero moved away (the statistics move with x, hence the
    loop), so that the LeakyReLU gate of every arithmetic agrees."""
    x = x.clone()
    for _ in range(64):
        _, xh, rstd = instnorm_lrelu_forward(x.double(), eps)
        bad = xh.abs() < 1.5 * margin
        if not bad.any():
            break
        step = (8 * margin / rstd).expand_as(xh)
        x = torch.where(bad, (x.double() + torch.where(xh >= 0, step, -step)).float(), x)
    assert instnorm_margin(x, eps) >= margin
    return x


# ---------------------------------------------------------------------------------------------- spectral normalisation

def _normalize(t):
    return t / t.norm().clamp_min(SN_EPS)


def sn_power_iteration(w, u, v):
    """One power iteration of torch.nn.utils.spectral_norm in train() mode: (u, v) after it."""
    wm = w.reshape(w.shape[0], -1)
    v = _normalize(wm.t() @ u)
    u = _normalize(wm @ v)
    return u, v


def sn_sigma(w, u, v):
    return torch.dot(u, w.reshape(w.shape[0], -1) @ v)


def sn_weight_grad(dW, w, u, v):
    """d weight_orig from the gradient dW at W = weight_orig / sigma; u and v are constants of the gradient."""
    sigma = sn_sigma(w, u, v)
    return (dW - (dW * (w / sigma)).sum() * torch.outer(u, v).view_as(w)) / sigma


# ---------------------------------------------------------------------------------------------- the counted average pool

def _pool_count(H, W, like):
    ones = like.new_ones(1, 1, H, W)
    return F.pad(ones, (1, 1, 1, 1)).unfold(2, 3, 2).unfold(3, 3, 2).sum((4, 5))


def avgpool_forward(x):
    """F.avg_pool2d(x, 3, stride=2, padding=1, count_include_pad=False)."""
    H, W = x.shape[2:]
    return F.pad(x, (1, 1, 1, 1)).unfold(2, 3, 2).unfold(3, 3, 2).sum((4, 5)) / _pool_count(H, W, x)


def avgpool_backward(g, H, W):
    q = g / _pool_count(H, W, g)
    OH, OW = g.shape[2:]
    gp = g.new_zeros(g.shape[0], g.shape[1], H + 2, W + 2)
    for ky in range(3):
        for kx in range(3):
            gp[:, :, ky:ky + 2 * (OH - 1) + 1:2, kx:kx + 2 * (OW - 1) + 1:2] += q
    return gp[:, :, 1:1 + H, 1:1 + W].contiguous()


# ---------------------------------------------------------------------------------------------- the networks

def param_shapes(ndf, output_nc=3, num_D=2):
    """{state-dict key of MultiscaleDiscriminator: shape}, in the reference's order."""
    shapes = {}
    for d in range(num_D):
        p = f"discriminator_{d}."
        shapes[p + "model0.0.weight"] = (ndf, output_nc, 4, 4)
        shapes[p + "model0.0.bias"] = (ndf,)
        nf = ndf
        for j in (1, 2, 3):
            prev, nf = nf, min(nf * 2, 512)
            shapes[p + f"model{j}.0.0.weight_orig"] = (nf, prev, 4, 4)
            shapes[p + f"model{j}.0.0.weight_u"] = (nf,)
            shapes[p + f"model{j}.0.0.weight_v"] = (prev * 16,)
        shapes[p + "model4.0.weight"] = (1, nf, 4, 4)
        shapes[p + "model4.0.bias"] = (1,)
    return shapes


def fixture_param(case, key, shape):
    """The float32-valued tensor ``key`` of case ``case``, seeded by its name: weights randn / sqrt(fan-in) (the default initialisation
    makes the maps vanish), biases 0.3 randn, u / v unit vectors, images 0.7 randn."""
    gen = torch.Generator().manual_seed(zlib.crc32(f"{case}/{key}".encode()))
    t = torch.randn(*shape, generator=gen, dtype=torch.float32)
    if key.endswith("weight_u") or key.endswith("weight_v"):
        return t / t.norm()
    if key.endswith(".bias"):
        return t * 0.3
    if len(shape) == 4 and shape[2:] == (4, 4):
        return t / float(shape[1] * 16) ** 0.5
    return t * 0.7


def fixture_state(case, ndf, dtype=torch.float64):
    return {k: fixture_param(case, k, s).to(dtype) for k, s in param_shapes(ndf).items()}


def effective_weights(P, d, training):
    """The five convolution weights of discriminator d as the forward uses them, and the state after it: in training mode every spectral
    layer first runs one power iteration and stores u, v (returned as a new dict)."""
    p = f"discriminator_{d}."
    new, Ws = {}, [P[p + "model0.0.weight"]]
    for j in (1, 2, 3):
        k = p + f"model{j}.0.0.weight"
        w, u, v = P[k + "_orig"], P[k + "_u"], P[k + "_v"]
        if training:
            u, v = sn_power_iteration(w, u, v)
            new[k + "_u"], new[k + "_v"] = u, v
        Ws.append(w / sn_sigma(w, u, v))
    Ws.append(P[p + "model4.0.weight"])
    return Ws, new


def nlayer_forward(x, Ws, b0, b4):
    """NLayerDiscriminator.forward: the five outputs and what the backward needs."""
    z0 = conv_forward(x, Ws[0], b0, 2)
    feats, cache = [leaky(z0)], {"in": [x], "z0": z0, "xh": [None], "rstd": [None]}
    for j in (1, 2, 3):
        cache["in"].append(feats[-1])
        y, xh, rstd = instnorm_lrelu_forward(conv_forward(feats[-1], Ws[j], None, STRIDES[j]))
        cache["xh"].append(xh)
        cache["rstd"].append(rstd)
        feats.append(y)
    cache["in"].append(feats[-1])
    feats.append(conv_forward(feats[-1], Ws[4], b4, 1))
    return feats, cache


def nlayer_backward(gfeats, cache, Ws, need_input=True):
    """Gradients at the five effective weights, the two biases and (need_input) the input, from the gradients at the five outputs."""
    dW, xin = [None] * 5, cache["in"]
    dW[4], db4 = conv_weight_grad(xin[4], gfeats[4], 1)
    g = conv_backward_data(gfeats[4], Ws[4], 1, *xin[4].shape[2:]) + gfeats[3]
    for j in (3, 2, 1):
        gz = instnorm_lrelu_backward(g, cache["xh"][j], cache["rstd"][j])
        dW[j], _ = conv_weight_grad(xin[j], gz, STRIDES[j])
        g = conv_backward_data(gz, Ws[j], STRIDES[j], *xin[j].shape[2:]) + gfeats[j - 1]
    gz0 = g * leaky_gate(cache["z0"])
    dW[0], db0 = conv_weight_grad(xin[0], gz0, 2)
    gx = conv_backward_data(gz0, Ws[0], 2, *xin[0].shape[2:]) if need_input else None
    return dW, db0, db4, gx


def multiscale_forward(P, x, training, num_D=2):
    """MultiscaleDiscriminator.forward: feats[d][j], the caches, and the state with the updated u / v."""
    P = dict(P)
    feats, caches = [], []
    for d in range(num_D):
        Ws, new = effective_weights(P, d, training)
        P.update(new)
        f, c = nlayer_forward(x, Ws, P[f"discriminator_{d}.model0.0.bias"], P[f"discriminator_{d}.model4.0.bias"])
        c["Ws"], c["x"] = Ws, x
        feats.append(f)
        caches.append(c)
        x = avgpool_forward(x)
    return feats, caches, P


def multiscale_backward(P, gfeats, caches, need_input=True):
    """{key: gradient} for every parameter (weight_orig of the spectral layers) and "input"."""
    grads = {}
    for d in reversed(range(len(caches))):
        c, p = caches[d], f"discriminator_{d}."
        dW, db0, db4, gx = nlayer_backward(gfeats[d], c, c["Ws"], need_input)
        grads[p + "model0.0.weight"], grads[p + "model0.0.bias"] = dW[0], db0
        grads[p + "model4.0.weight"], grads[p + "model4.0.bias"] = dW[4], db4
        for j in (1, 2, 3):
            k = p + f"model{j}.0.0.weight"
            grads[k + "_orig"] = sn_weight_grad(dW[j], P[k + "_orig"], P[k + "_u"], P[k + "_v"])
        if need_input:
            c["gx"] = gx
    if need_input:
        g = caches[-1]["gx"]
        for d in reversed(range(len(caches) - 1)):
            g = caches[d]["gx"] + avgpool_backward(g, *caches[d]["x"].shape[2:])
        grads["input"] = g
    return grads


def _mean_grad(t, sign=1.0):
    return torch.full_like(t, sign / t.numel())


def generator_step(P, fake, real, lambda_feat=10.0, training=True, with_grads=True):
    """run_generator_one_step: (losses, per-term feature losses, gradients {key / "fake": tensor}, state after the forward)."""
    n = fake.shape[0]
    feats, caches, P2 = multiscale_forward(P, torch.cat([fake, real]), training)
    num_D = len(feats)
    gan, feat, terms, gfeats = 0.0, 0.0, [], []
    for f in feats:
        pf = f[4][:n]
        gan = gan + -pf.mean()
        gf = []
        for j in range(4):
            a, b = f[j][:n], f[j][n:]
            term = (a - b).abs().mean()
            terms.append(term)
            feat = feat + term * lambda_feat / num_D
            gf.append(torch.cat([torch.sign(a - b) * (lambda_feat / num_D / a.numel()), torch.zeros_like(b)]))
        gf.append(torch.cat([_mean_grad(pf, -1.0 / num_D), torch.zeros_like(f[4][n:])]))
        gfeats.append(gf)
    gan = gan / num_D
    losses = {"GAN": gan.reshape(1), "GAN_Feat": feat.reshape(1), "Total Loss": (gan + feat).reshape(())}
    grads = None
    if with_grads:
        grads = multiscale_backward(P2, gfeats, caches, need_input=True)
        grads["fake"] = grads.pop("input")[:n]
    return losses, terms, grads, P2


def discriminator_step(P, fake, real, training=True, with_grads=True):
    """run_discriminator_one_step (the fake image detached): (losses, gradients {key: tensor}, state after the forward)."""
    n = fake.shape[0]
    feats, caches, P2 = multiscale_forward(P, torch.cat([fake, real]), training)
    num_D = len(feats)
    d_fake, d_real, gfeats = 0.0, 0.0, []
    for f in feats:
        pf, pr = f[4][:n], f[4][n:]
        d_fake = d_fake + -torch.minimum(-pf - 1, torch.zeros_like(pf)).mean()
        d_real = d_real + -torch.minimum(pr - 1, torch.zeros_like(pr)).mean()
        g_f = (-pf - 1 < 0).to(pf.dtype) / (num_D * pf.numel())
        g_r = -(pr - 1 < 0).to(pr.dtype) / (num_D * pr.numel())
        gfeats.append([torch.zeros_like(t) for t in f[:4]] + [torch.cat([g_f, g_r])])
    d_fake, d_real = d_fake / num_D, d_real / num_D
    losses = {"D_Fake": d_fake.reshape(()), "D_real": d_real.reshape(()), "Total Loss": (d_fake + d_real).reshape(())}
    grads = multiscale_backward(P2, gfeats, caches, need_input=False) if with_grads else None
    return losses, grads, P2


def gate_margin(P, fake, real):
    """The smallest distance from zero of anything a sign or a comparison is taken of in the two steps, in float64: the LeakyReLU inputs,
    fake - real of every matched feature, p +- 1 of the final maps."""
    P = {k: v.double() for k, v in P.items()}
    n = fake.shape[0]
    margin = float("inf")
    for _ in range(2):                                    # (the two forwards of a training step see different u / v)
        feats, caches, P = multiscale_forward(P, torch.cat([fake, real]).double(), True)
        for f, c in zip(feats, caches):
            vals = [c["z0"]] + [c["xh"][j] for j in (1, 2, 3)] + [f[j][:n] - f[j][n:] for j in range(4)] + [f[4] - 1, f[4] + 1]
            margin = min(margin, min(float(v.abs().min()) for v in vals))
    return margin


def first_clean_seed(case, ndf, N, H, W, limit=1000, margin=1e-4):
    """(seed, state, fake, real): the first seed whose images keep every gate ``margin`` from zero with the parameters of ``case``."""
    P = fixture_state(case, ndf, torch.float32)
    for seed in range(limit):
        fake = fixture_param(case, f"fake{seed}", (N, 3, H, W))
        real = fixture_param(case, f"real{seed}", (N, 3, H, W))
        if gate_margin(P, fake, real) >= margin:
            return seed, P, fake, real
    raise AssertionError(f"no seed below {limit} keeps the gates {margin} from zero")


# ---------------------------------------------------------------------------------------------- fixture storage

def packed(name, v):
    """npz entries of array v: float64 arrays become a float32 part and an int16 correction with one scale per array (6 bytes per
    element, the error at most ~1e-12 max|v|)."""
    import numpy as np
    if v.dtype != np.float64 or v.size < 64:
        return {name: v}
    hi = v.astype(np.float32)
    rest = v - hi.astype(np.float64)
    scale = max(float(np.abs(rest).max()), 1e-300) / 32767.0
    return {name + "#hi": hi, name + "#lo": np.round(rest / scale).astype(np.int16), name + "#scale": np.float64(scale)}


def load_packed(path):
    import numpy as np
    g = np.load(path)
    out = {}
    for k in g.files:
        if k.endswith("#hi"):
            n = k[:-3]
            out[n] = torch.from_numpy(g[k].astype(np.float64) + g[n + "#lo"].astype(np.float64) * float(g[n + "#scale"]))
        elif "#" not in k:
            out[k] = g[k] if g[k].dtype.kind in "US" else torch.from_numpy(g[k])
    return out
