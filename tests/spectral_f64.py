"""The written-out definition of the generator's spectral normalisation (torch.nn.utils.spectral_norm as the reference applies it under
--norm_G sync:spectral_batch: models/layers/blocks.py:5-35, models/layers/normalization.py:6-16), in the dtype of its inputs (float64 for
the reference values, float32 for E_plain32): the power iteration, sigma, the effective weight, the gradient to weight_orig, and a block
and a whole network with it, on top of the block definitions of block_train_f64.py / decoder_train_f64.py.

A normalised layer is (W, u, v): weight_orig [rows, ...], u [rows], v [numel / rows].  In training mode every forward does ONE power
iteration (v <- W^T u / max(|W^T u|, eps), u <- W v / max(|W v|, eps)) and then uses W / sigma, sigma = u^T W v; u and v are constants of
the backward, so
    d weight_orig = (dW - <dW, W_eff> u v^T) / sigma,       W_eff = W / sigma, dW the gradient at W_eff."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_train_f64 as B64          # noqa: E402
import conv_train_f64 as C64           # noqa: E402
import decoder_train_f64 as D64        # noqa: E402

EPS = 1e-12
CONVS = ("w_aa", "w_ab", "w_b")                          # the normalised convolutions of a block (w_b may be None)
LINEARS = ("gain1", "bias1", "gain2", "bias2")           # the [C, noise_sz] maps of its two noise layers
BLOCKS = {"pconv": (B64.block, B64.block_grads), "input": (D64.input_block, D64.input_block_grads),
          "res": (D64.res_block, D64.res_block_grads)}


def mat(W):
    return W.reshape(W.shape[0], -1)


def power_iteration(W, u, v, eps=EPS):
    """One iteration of SpectralNorm.compute_weight: the new (u, v)."""
    Wm = mat(W)
    t = Wm.t() @ u
    v = t / torch.clamp(t.norm(), min=eps)
    s = Wm @ v
    u = s / torch.clamp(s.norm(), min=eps)
    return u, v


def sigma(W, u, v):
    return torch.dot(u, mat(W) @ v)


def effective(W, u, v, training=True, eps=EPS):
    """(W_eff, u, v, inv_sigma) of one forward: training iterates first, eval uses the stored u and v."""
    if training:
        u, v = power_iteration(W, u, v, eps)
    inv = 1.0 / sigma(W, u, v)
    return W * inv, u, v, inv


def weight_orig_grad(dW, W, u, v, inv_sigma):
    """The gradient to weight_orig from the gradient dW at the effective weight; u, v, inv_sigma: of that forward."""
    d = (dW * W).sum() * inv_sigma                                                       # <dW, W_eff>
    return ((mat(dW) - d * torch.outer(u, v)) * inv_sigma).reshape(W.shape)


def rank_one_term(dW, W, u, v, inv_sigma):
    """|<dW, W_eff>| max|u v^T| / sigma: the magnitude of the subtrahend (for E_terms)."""
    d = (dW * W).sum() * inv_sigma
    return (d.abs() * torch.outer(u, v).abs().max() * abs(inv_sigma)), (mat(dW).abs().max() * abs(inv_sigma))


def names_of(p):
    return [k for k in CONVS + LINEARS if p.get(k) is not None]


def normalise(p, uv, training=True):
    """One forward's normalisation of a block: p holds the weight_orig tensors (CONVS, LINEARS) and the biases; uv: name -> (u, v).
    Returns (p_eff: the same dict with effective weights, uv_new, inv: name -> 1 / sigma)."""
    pe, un, inv = dict(p), {}, {}
    for k in names_of(p):
        pe[k], u, v, inv[k] = effective(p[k], *uv[k], training=training)
        un[k] = (u, v)
    return pe, un, inv


def tables(pe, noise):
    """The two BNs' [N, C] gain and bias tables from the noise pair (normalization.py:45-46)."""
    n1, n2 = noise
    return (1.0 + n1 @ pe["gain1"].t(), 1.0 + n2 @ pe["gain2"].t()), (n1 @ pe["bias1"].t(), n2 @ pe["bias2"].t())


def block(form, x, mask, p, uv, kind, noise, training=True, stored=None):
    """A block of ``form`` ('pconv': ResNet_Block_Pconv2 with a mask, 'input': with mask = x != 0, 'res': ResNet_Block) under spectral
    normalisation.  Returns (the block definition's dict, uv_new, (pe, inv, gains, biases))."""
    pe, un, inv = normalise(p, uv, training)
    gains, biases = tables(pe, noise)
    fwd = BLOCKS[form][0]
    f = fwd(x, mask, pe, kind, gains, biases, stored=stored) if form == "pconv" else fwd(x, pe, kind, gains, biases, stored=stored)
    return f, un, (pe, inv, gains, biases)


def block_grads(form, x, mask, p, uv_used, kind, noise, g, ctx, stored=None):
    """Every gradient of ``block`` for the gradient g at y.  uv_used, ctx: what ``block`` returned for THAT forward.  The dict of the
    block definition plus d_<name>: the gradient to the weight_orig of every normalised tensor, and dW_<name>: the one at W_eff."""
    pe, inv, gains, biases = ctx
    bwd = BLOCKS[form][1]
    d = bwd(x, mask, pe, kind, gains, biases, g, stored=stored) if form == "pconv" else bwd(x, pe, kind, gains, biases, g, stored=stored)
    at = {"w_aa": d["dw_aa"], "w_ab": d["dw_ab"], "w_b": d.get("dw_b"),
          "gain1": d["dgain1"].t() @ noise[0], "bias1": d["dbias1"].t() @ noise[0],
          "gain2": d["dgain2"].t() @ noise[1], "bias2": d["dbias2"].t() @ noise[1]}
    for k in names_of(p):
        d["dW_" + k] = at[k]
        d["d_" + k] = weight_orig_grad(at[k], p[k], *uv_used[k], inv[k])
    return d


def network(forms, x, ps, uvs, kinds, noises, training=True, stored=None):
    """A chain of blocks (forms[i] per block: a decoder is 'input' then 'pconv's, an encoder 'res's).  Returns (the blocks' dicts with
    x and mask, the new uvs, the ctxs)."""
    fs, uns, ctxs, mask = [], [], [], None
    for i, p in enumerate(ps):
        f, un, ctx = block(forms[i], x, mask, p, uvs[i], kinds[i], noises[i], training, None if stored is None else stored[i])
        f["x"], f["mask"] = x, mask
        fs.append(f)
        uns.append(un)
        ctxs.append(ctx)
        x, mask = f["y"], f.get("um")
    return fs, uns, ctxs


def network_grads(forms, fs, ps, uns, kinds, noises, g, ctxs):
    ds = [None] * len(ps)
    for i in reversed(range(len(ps))):
        ds[i] = block_grads(forms[i], fs[i]["x"], fs[i]["mask"], ps[i], uns[i], kinds[i], noises[i], g, ctxs[i])
        g = ds[i]["dx"]
    return ds


# ------------------------------------------------------------------ inputs

def normal_uv(rows, cols, gen, dtype=torch.float64):
    u, v = torch.randn(rows, generator=gen, dtype=dtype), torch.randn(cols, generator=gen, dtype=dtype)
    return u / u.norm(), v / v.norm()


def matrix_case(rows, cols, seed, dtype=torch.float64):
    """(W, u, v) of the sigma-list tests: W of a convolution's scale, u and v normalised normal vectors; float32 values in ``dtype``."""
    gen = torch.Generator().manual_seed(seed)
    W = torch.randn(rows, cols, generator=gen, dtype=torch.float64) * (1.0 / cols) ** 0.5
    return tuple(t.float().to(dtype) for t in (W, *normal_uv(rows, cols, gen)))


def block_params(form, cin, cout, skip, seed, noise_sz=20):
    """weight_orig tensors, biases and (u, v) of one block, float64."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)                   # noqa: E731
    p = {"w_aa": r(cout, cin, 3, 3) * (1.0 / (9 * cin)) ** 0.5, "b_aa": 0.1 * r(cout),
         "w_ab": r(cout, cout, 3, 3) * (1.0 / (9 * cout)) ** 0.5, "b_ab": 0.1 * r(cout),
         "w_b": r(cout, cin, 1, 1) * (1.0 / cin) ** 0.5 if skip else None,
         "gain1": 0.2 * r(cin, noise_sz), "bias1": 0.2 * r(cin, noise_sz), "gain2": 0.2 * r(cout, noise_sz), "bias2": 0.2 * r(cout, noise_sz)}
    if form == "res":
        p["b_b"] = 0.1 * r(cout) if skip else None
    uv = {k: normal_uv(p[k].shape[0], p[k].numel() // p[k].shape[0], gen) for k in names_of(p)}
    return p, uv


def cast(tree, dtype):
    if torch.is_tensor(tree):
        return tree.to(dtype)
    if isinstance(tree, dict):
        return {k: cast(v, dtype) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return type(tree)(cast(v, dtype) for v in tree)
    return tree


def settle(net, iterations=3):
    """u and v of every normalised layer of a module after ``iterations`` float64 power iterations, in place: the state of a trained
    checkpoint (fresh random vectors give a sigma that is a difference of large terms, which no float32 fold resolves)."""
    with torch.no_grad():
        for m in net.modules():
            if getattr(m, "spectral_leaf", False):
                W, u, v = m.weight_orig.detach().double().cpu(), m.weight_u.double().cpu(), m.weight_v.double().cpu()
                for _ in range(iterations):
                    u, v = power_iteration(W, u, v)
                m.weight_u.copy_(u)
                m.weight_v.copy_(v)
    return net
