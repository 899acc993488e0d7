"""The operators that train the SPADE motion U-Net, written out without autograd (slr_sfs_amd.motion_training; the reference's
models/networks/architectures.py:602-743, models/networks/networks.py:422-463, models/losses/synthesis.py:142-160) in whatever dtype
their inputs have -- float64 as the reference of the tests, float32 as the plain-fp32 yardstick E_plain32.

  * Conv2d(Cin, Cout, 4, stride 2, padding 1) with the LeakyReLU in FRONT of it: forward, backward-data, weight and bias gradient;
  * instance norm + SPADE modulation: forward and the gradients to x, gamma and beta;
  * the mixed bilinear / nearest x2 up-sampling + concatenation with the ReLU before or after it: forward and backward;
  * EndPointError, MotionL1 and the PSNR's squared error, and the gradient to the prediction.

Every definition takes ``wrong=`` naming one deliberate mistake (WRONG below); tests/test_motion_train_f64.py shows that the criterion of
the device tests rejects each of them.  tests/test_motion_train_f64.py also ties every definition to torch autograd."""
import torch
import torch.nn.functional as F

EPS = 1e-5
RELU_NONE, RELU_BEFORE, RELU_AFTER = 0, 1, 2
WRONG = ("norm_no_xhat_term", "nearest_channel_bilinear", "no_leaky_gate", "padding2_taps", "epe_grad_not_zeroed", "first_lambda_ignored")


def out_size(H):
    return (H - 2) // 2 + 1                   # (H + 2 * 1 - 4) / 2 + 1


def leaky(x, slope):
    return x if slope is None else torch.where(x > 0, x, x * slope)


def leaky_gate(x, slope):
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))


# ---------------------------------------------------------------------------------------------- the 4x4 / stride 2 / padding 1 convolution

def _taps(H, W):
    OH, OW = out_size(H), out_size(W)
    for ky in range(4):
        for kx in range(4):
            yield ky, kx, slice(ky, ky + 2 * (OH - 1) + 1, 2), slice(kx, kx + 2 * (OW - 1) + 1, 2)


def conv_forward(x, w, b, slope):
    """conv2d(leaky_relu(x, slope), w, b, stride 2, padding 1); slope None: no LeakyReLU."""
    N, _, H, W = x.shape
    xp = F.pad(leaky(x, slope), (1, 1, 1, 1))
    out = x.new_zeros(N, w.shape[0], out_size(H), out_size(W))
    for ky, kx, ys, xs in _taps(H, W):
        out += torch.einsum("nchw,oc->nohw", xp[:, :, ys, xs], w[:, :, ky, kx])
    return out if b is None else out + b.view(1, -1, 1, 1)


def conv_backward_data(g, w, x, slope, wrong=None):
    """The gradient to x (the RAW input: the LeakyReLU's gate is part of it)."""
    H, W = x.shape[2:]
    pad = 2 if wrong == "padding2_taps" else 1
    gp = g.new_zeros(g.shape[0], w.shape[1], H + 4, W + 4)
    for ky, kx, ys, xs in _taps(H, W):
        gp[:, :, ys, xs] += torch.einsum("nohw,oc->nchw", g, w[:, :, ky, kx])
    gx = gp[:, :, pad:pad + H, pad:pad + W].contiguous()
    if slope is not None and wrong != "no_leaky_gate":
        gx = gx * leaky_gate(x, slope)
    return gx


def conv_weight_grad(x, g, slope):
    H, W = x.shape[2:]
    xp = F.pad(leaky(x, slope), (1, 1, 1, 1))
    dw = x.new_zeros(g.shape[1], x.shape[1], 4, 4)
    for ky, kx, ys, xs in _taps(H, W):
        dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, xp[:, :, ys, xs])
    return dw, g.sum((0, 2, 3))


def sn_weight_grad(dW, w, u, v, inv_sigma):
    """d weight_orig from the gradient dW at W = weight_orig * inv_sigma; u and v are constants of the gradient."""
    return (dW - (dW * (w * inv_sigma)).sum() * torch.outer(u, v).view_as(w)) * inv_sigma


# ---------------------------------------------------------------------------------------------- SPADE instance norm

def instnorm_spade_forward(x, gamma_beta, eps=EPS):
    """(out, xh, rstd): out = xh (1 + gamma) + beta, gamma | beta the halves of gamma_beta [N,2C,H,W]."""
    C = x.shape[1]
    m = x.mean((2, 3), keepdim=True)
    d = x - m
    rstd = 1.0 / torch.sqrt((d * d).mean((2, 3), keepdim=True) + eps)
    xh = d * rstd
    return xh * (1 + gamma_beta[:, :C]) + gamma_beta[:, C:], xh, rstd


def instnorm_spade_backward(g, gamma_beta, xh, rstd, wrong=None):
    """(gx, d gamma_beta) from g = d out."""
    C = xh.shape[1]
    gh = g * (1 + gamma_beta[:, :C])
    gx = gh - gh.mean((2, 3), keepdim=True)
    if wrong != "norm_no_xhat_term":
        gx = gx - xh * (gh * xh).mean((2, 3), keepdim=True)
    return rstd * gx, torch.cat([g * xh, g], 1)


def instnorm_margin(x, eps=EPS):
    return float(instnorm_spade_forward(x.double(), x.new_zeros(x.shape[0], 2 * x.shape[1], *x.shape[2:]).double(), eps)[1].abs().min())


# ---------------------------------------------------------------------------------------------- x2 up-sampling + concatenation

def up_matrix(L, like, nearest=False):
    """U [2L, L] with up(x) = U x along one axis: nn.Upsample(scale_factor=2, bilinear, align_corners=False) -- out[2k] = .25 x[k-1] +
    .75 x[k] (out[0] = x[0]), out[2k+1] = .75 x[k] + .25 x[min(k+1, L-1)] -- or mode='nearest'."""
    U = like.new_zeros(2 * L, L)
    for k in range(L):
        if nearest:
            U[2 * k, k] = U[2 * k + 1, k] = 1.0
            continue
        U[2 * k, k] += 0.75
        U[2 * k, max(k - 1, 0)] += 0.25
        U[2 * k + 1, k] += 0.75
        U[2 * k + 1, min(k + 1, L - 1)] += 0.25
    return U


def _up(x, nearest_channel, transpose=False, wrong=None):
    """up(x) per channel (transpose: its adjoint, [.., 2H, 2W] -> [.., H, W]); channel ``nearest_channel`` nearest."""
    H, W = (x.shape[2] // 2, x.shape[3] // 2) if transpose else x.shape[2:]
    out = x.new_zeros(x.shape[0], x.shape[1], *((H, W) if transpose else (2 * H, 2 * W)))
    for c in range(x.shape[1]):
        near = c == nearest_channel and wrong != "nearest_channel_bilinear"
        Uy, Ux = up_matrix(H, x, near), up_matrix(W, x, near)
        out[:, c] = Uy.t() @ x[:, c] @ Ux if transpose else Uy @ x[:, c] @ Ux.t()
    return out


def upsample_concat_forward(a, b, nearest_channel, relu):
    srcs = [a] if b is None else [a, b]
    if relu == RELU_BEFORE:
        srcs = [torch.clamp_min(s, 0) for s in srcs]
    out = torch.cat([_up(s, nearest_channel) for s in srcs], 1)
    return torch.clamp_min(out, 0) if relu == RELU_AFTER else out


def upsample_concat_backward(g, out, a, b, nearest_channel, relu, wrong=None):
    """(ga, gb) from g = d out; ``out`` the forward's result (RELU_AFTER gates by it), a / b the sources (RELU_BEFORE gates by them)."""
    if relu == RELU_AFTER:
        g = g * (out > 0).to(g.dtype)
    Ca = a.shape[1]
    ga = _up(g[:, :Ca], nearest_channel, True, wrong)
    gb = None if b is None else _up(g[:, Ca:], nearest_channel, True, wrong)
    if relu == RELU_BEFORE:
        ga = ga * (a > 0).to(g.dtype)
        gb = None if b is None else gb * (b > 0).to(g.dtype)
    return ga, gb


# ---------------------------------------------------------------------------------------------- the motion losses

def motion_losses(pred, gt):
    """(EndPointError, MotionL1, mse_err [N]) of pred, gt [N,2,H,W]."""
    d = pred - gt
    sq = (d * d).sum(1)
    return torch.sqrt(sq).mean(), d.abs().mean(), sq.reshape(d.shape[0], -1).mean(1)


def motion_losses_grad(pred, gt, w_epe, w_l1, wrong=None):
    """d (w_epe EndPointError + w_l1 MotionL1) / d pred; the EndPointError's part is 0 where pred == gt (torch's norm backward)."""
    d = pred - gt
    N, _, H, W = d.shape
    nrm = torch.sqrt((d * d).sum(1, keepdim=True))
    if wrong == "epe_grad_not_zeroed":
        unit = d / nrm
    else:
        unit = torch.where(nrm > 0, d / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(d))
    return w_epe * unit / (N * H * W) + w_l1 * torch.sign(d) / (2 * N * H * W)


def total_loss(terms, lambdas, wrong=None):
    """MotionLoss's ``Total Loss`` (synthesis.py:46-58): EVERY term times its lambda, the first included (SynthesisLoss leaves the first
    one unscaled)."""
    total = None
    for i, (t, lam) in enumerate(zip(terms, lambdas)):
        if i == 0:
            total = t if wrong == "first_lambda_ignored" else t * lam
        else:
            total = total + t * lam
    return total


# ---------------------------------------------------------------------------------------------- the 3x3 convolutions of the decoder and of SPADE

def conv3_forward(x, w, b):
    return F.conv2d(x, w, b, padding=1)


def conv3_backward_data(g, w):
    return F.conv_transpose2d(g, w, padding=1)


def conv3_weight_grad(x, g):
    xp = F.pad(x, (1, 1, 1, 1))
    H, W = x.shape[2:]
    dw = x.new_zeros(g.shape[1], x.shape[1], 3, 3)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, xp[:, :, ky:ky + H, kx:kx + W])
    return dw, g.sum((0, 2, 3))


# ---------------------------------------------------------------------------------------------- spectral normalisation

SN_EPS = 1e-12


def _normalize(t):
    return t / t.norm().clamp_min(SN_EPS)


def sn_power_iteration(w, u, v):
    wm = w.reshape(w.shape[0], -1)
    v = _normalize(wm.t() @ u)
    return _normalize(wm @ v), v


def sn_inv_sigma(w, u, v):
    return 1.0 / torch.dot(u, w.reshape(w.shape[0], -1) @ v)


# ---------------------------------------------------------------------------------------------- the network (architectures.py:673-743)

ENC_NORM = {2: "2_0", 3: "4_0", 4: "8_0", 5: "8_1", 6: "8_2", 7: "8_3"}
DEC_NORM = {1: "8_4", 2: "8_5", 3: "8_6", 4: "8_7", 5: "4_1", 6: "2_1", 7: ""}
SN_LAYERS = [f"conv{i}" for i in range(1, 9)] + [f"dconv{i}" for i in range(1, 9)]
SLOPE = 0.2


def param_shapes(nf, cin=6, cout=2):
    """{state-dict key of SPADEUnet4MaskMotion under spectral norm: shape}."""
    enc = [cin, nf, nf * 2, nf * 4, nf * 8, nf * 8, nf * 8, nf * 8, nf * 8]
    dec = [(nf * 8, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 8), (nf * 16, nf * 4), (nf * 8, nf * 2), (nf * 4, nf),
           (nf * 2, cout)]
    shapes = {}

    def sn(name, ci, co, k):
        shapes[f"{name}.bias"], shapes[f"{name}.weight_orig"] = (co,), (co, ci, k, k)
        shapes[f"{name}.weight_u"], shapes[f"{name}.weight_v"] = (co,), (ci * k * k,)
    for i in range(1, 9):
        sn(f"conv{i}", enc[i - 1], enc[i], 4)
        sn(f"dconv{i}", dec[i - 1][0], dec[i - 1][1], 3)
    for C, s in [(enc[i], s) for i, s in ENC_NORM.items()] + [(dec[k - 1][1], s) for k, s in DEC_NORM.items()]:
        p = f"spade_layer{s}."
        shapes[p + "mlp_shared.0.weight"], shapes[p + "mlp_shared.0.bias"] = (128, 6, 3, 3), (128,)
        for h in ("mlp_gamma", "mlp_beta"):
            shapes[p + h + ".weight"], shapes[p + h + ".bias"] = (C, 128, 3, 3), (C,)
    return shapes


def segmap(x, like):
    """SPADE's segmap at ``like``'s size (networks.py:450-455): bilinear, the mask channel nearest."""
    size = like.shape[2:]
    return torch.cat([F.interpolate(x[:, :3], size=size, mode="bilinear", align_corners=False),
                      F.interpolate(x[:, 3:4], size=size, mode="nearest"),
                      F.interpolate(x[:, 4:6], size=size, mode="bilinear", align_corners=False)], 1)


def spade_forward(P, p, y, x):
    seg = segmap(x, y)
    pre = conv3_forward(seg, P[p + "mlp_shared.0.weight"], P[p + "mlp_shared.0.bias"])
    actv = torch.clamp_min(pre, 0)
    gb = torch.cat([conv3_forward(actv, P[p + "mlp_gamma.weight"], P[p + "mlp_gamma.bias"]),
                    conv3_forward(actv, P[p + "mlp_beta.weight"], P[p + "mlp_beta.bias"])], 1)
    out, xh, rstd = instnorm_spade_forward(y, gb)
    return out, dict(seg=seg, pre=pre, actv=actv, gb=gb, xh=xh, rstd=rstd)


def spade_backward(P, p, g, c, grads, wrong=None):
    gy, dgb = instnorm_spade_backward(g, c["gb"], c["xh"], c["rstd"], wrong)
    C = g.shape[1]
    gactv = 0
    for h, d in (("mlp_gamma", dgb[:, :C]), ("mlp_beta", dgb[:, C:])):
        grads[p + h + ".weight"], grads[p + h + ".bias"] = conv3_weight_grad(c["actv"], d)
        gactv = gactv + conv3_backward_data(d, P[p + h + ".weight"])
    gpre = gactv * (c["pre"] > 0).to(g.dtype)
    grads[p + "mlp_shared.0.weight"], grads[p + "mlp_shared.0.bias"] = conv3_weight_grad(c["seg"], gpre)
    return gy


def net_forward(P, x, training):
    """(prediction, cache, state after the forward: in training mode every spectral layer runs one power iteration first)."""
    P = dict(P)
    inv = {}
    for name in SN_LAYERS:
        w, u, v = P[name + ".weight_orig"], P[name + ".weight_u"], P[name + ".weight_v"]
        if training:
            u, v = sn_power_iteration(w, u, v)
            P[name + ".weight_u"], P[name + ".weight_v"] = u, v
        inv[name] = sn_inv_sigma(w, u, v)
    W = {name: P[name + ".weight_orig"] * inv[name] for name in SN_LAYERS}
    c = dict(x=x, inv=inv, W=W, spade={}, cin={}, din={}, dout={})
    e = [conv_forward(x, W["conv1"], P["conv1.bias"], None)]
    for i in range(2, 9):
        c["cin"][i] = e[-1]
        y = conv_forward(e[-1], W[f"conv{i}"], P[f"conv{i}.bias"], SLOPE)
        if i < 8:
            y, c["spade"][f"spade_layer{ENC_NORM[i]}."] = spade_forward(P, f"spade_layer{ENC_NORM[i]}.", y, x)
        e.append(y)
    c["e"] = e
    d = upsample_concat_forward(e[7], None, 3, RELU_BEFORE)
    for k in range(1, 8):
        c["din"][k] = d
        y = conv3_forward(d, W[f"dconv{k}"], P[f"dconv{k}.bias"])
        y, c["spade"][f"spade_layer{DEC_NORM[k]}."] = spade_forward(P, f"spade_layer{DEC_NORM[k]}.", y, x)
        c["dout"][k] = y
        d = upsample_concat_forward(y, e[7 - k], 3, RELU_AFTER)
    c["din"][8] = d
    return conv3_forward(d, W["dconv8"], P["dconv8.bias"]), c, P


def net_backward(P, c, g, wrong=None):
    """{state-dict key: gradient} from g = d prediction; P the state after the forward."""
    grads, W, e = {}, c["W"], c["e"]

    def sn_grad(name, dw, db):
        grads[name + ".bias"] = db
        grads[name + ".weight_orig"] = sn_weight_grad(dw, P[name + ".weight_orig"], P[name + ".weight_u"], P[name + ".weight_v"], c["inv"][name])
    ge = [None] * 8
    sn_grad("dconv8", *conv3_weight_grad(c["din"][8], g))
    gd = conv3_backward_data(g, W["dconv8"])
    for k in range(7, 0, -1):
        gy, ge[7 - k] = upsample_concat_backward(gd, c["din"][k + 1], c["dout"][k], e[7 - k], 3, RELU_AFTER, wrong)
        gy = spade_backward(P, f"spade_layer{DEC_NORM[k]}.", gy, c["spade"][f"spade_layer{DEC_NORM[k]}."], grads, wrong)
        sn_grad(f"dconv{k}", *conv3_weight_grad(c["din"][k], gy))
        gd = conv3_backward_data(gy, W[f"dconv{k}"])
    ge[7], _ = upsample_concat_backward(gd, None, e[7], None, 3, RELU_BEFORE, wrong)
    for i in range(8, 1, -1):
        gy = ge[i - 1]
        if i < 8:
            gy = spade_backward(P, f"spade_layer{ENC_NORM[i]}.", gy, c["spade"][f"spade_layer{ENC_NORM[i]}."], grads, wrong)
        sn_grad(f"conv{i}", *conv_weight_grad(c["cin"][i], gy, SLOPE))
        ge[i - 2] = ge[i - 2] + conv_backward_data(gy, W[f"conv{i}"], c["cin"][i], SLOPE, wrong)
    sn_grad("conv1", *conv_weight_grad(c["x"], ge[0], None))
    return grads


# ---------------------------------------------------------------------------------------------- the model (unet_motion.py:131-173)

def parse_losses(entries):
    lam, names = zip(*[str(e).split("_") for e in entries])
    return [float(v) for v in lam], list(names)


def model_step(P, image, gt_motion, hint, motion_losses_opt, div_flow, training, with_grads=True, wrong=None):
    """SPADEUnetMaskMotion.forward(batch) and the gradient of its Total Loss: (losses, pred_dict, gradients, state after the forward)."""
    bs, _, H, W = image.shape
    speed = (gt_motion[:, 0:1] ** 2 + gt_motion[:, 1:2] ** 2).sqrt()
    mask = 1.0 - (speed < speed.mean([1, 2, 3], True) * 0.1).to(image.dtype)
    pred, cache, P2 = net_forward(P, torch.cat([image, mask, hint], 1), training)
    pm = pred * div_flow
    epe, l1, mse = motion_losses(pm, gt_motion)
    lam, names = parse_losses(motion_losses_opt)
    terms = [epe if n == "EndPointError" else l1 for n in names]
    losses = {n: t for n, t in zip(names, terms)}
    losses["Total Loss"] = total_loss(terms, lam, wrong)
    losses["PSNR_motion"] = (10 * (1 / mse).log10()).mean()
    grads = None
    if with_grads:
        w_epe = sum(v for v, n in zip(lam, names) if n == "EndPointError")
        w_l1 = sum(v for v, n in zip(lam, names) if n == "MotionL1")
        grads = net_backward(P2, cache, motion_losses_grad(pm, gt_motion, w_epe, w_l1, wrong) * div_flow, wrong)
    return losses, dict(PredMotion=pred, GTMotion=gt_motion, InputImg=image, MovingMask=mask, HintMotion=hint), grads, P2
