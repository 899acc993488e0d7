"""The head of the two-layer model (models/animating_softmax_splating_2layers_alpha_seperate.py, the lines given at each step) written out
in torch, callable in float64 and float32: the definition slr_sfs_amd.layers is held to.  Also the analytic backward of both operators as
csrc/layers.hip computes it, written out in torch so that it can be held to autograd of the definition on the host."""
import torch

LOSS_NAMES = ("AlphaMSEloss", "AlphaTV", "Alpha Decoder Consistency Loss", "Moving Region Alpha Decoder Consistency Loss")


def smooth_l1(inp, target, gamma=0.1):                                      # :63-65
    t = torch.abs(inp - target)
    return t + gamma * (2 * torch.sigmoid(5 * t) - 1)


def total_variation(image):                                                 # :67-71
    return torch.mean(torch.abs(image[:, :, :, :-1] - image[:, :, :, 1:])) + \
        torch.mean(torch.abs(image[:, :, :-1, :] - image[:, :, 1:, :]))


def layer_composite(fluid_raw, bg_raw, fluid_alpha_raw, bg_alpha_raw):
    """(pred, fluid, bg, composite_alpha), :372, :598, :608, :616-617, :652, :775, :789."""
    bg = torch.tanh(bg_raw)
    fluid = torch.tanh(fluid_raw)
    af = torch.sigmoid(fluid_alpha_raw)
    ab = torch.sigmoid(bg_alpha_raw)
    n = torch.clamp(af + ab, min=1e-8)
    pred = (af * fluid + ab * bg) / n
    return pred, fluid, bg, torch.sigmoid(fluid_alpha_raw) / torch.clamp(af + ab, min=1e-8)


def alpha_losses(a_start, mask_rock, small_motion_alpha, warped_alpha, norm, fluid_alpha_raw, reweight=True, mutant=None):
    """(dict of the four losses, GTAlpha, c0), :393-397, :420-421, :569, :619-621, :658-666, :694-699, :727-729, :757-765.
    ``mutant`` "tv_sigmoid": the deliberately wrong total variation that sigmoids the fluid plane too (the mutation check)."""
    a_bg_raw, a_fluid = a_start[:, 0:1], a_start[:, 1:2]
    a_bg = torch.sigmoid(a_bg_raw)
    n0 = torch.clamp(torch.sigmoid(a_fluid) + a_bg, min=1e-8)
    c0 = torch.sigmoid(a_fluid) / n0
    sma = small_motion_alpha
    gt = mask_rock * (1.0 - sma) * 0.25 + (1.0 - mask_rock) * (1.0 - sma) * 1 + sma * 0.5
    err = (c0 * (1.0 - sma) - gt * (1.0 - sma)) ** 2                        # nn.MSELoss(reduction='none')
    if reweight:
        pos = mask_rock * (1.0 - sma)
        neg = (1.0 - mask_rock) * (1.0 - sma)
        mse = .5 * ((pos * err).sum() / (1 + pos.sum()) + (neg * err).sum() / (1 + neg.sum()))
    else:
        mse = err.mean()
    tv = total_variation(torch.sigmoid(a_fluid) if mutant == "tv_sigmoid" else a_fluid) + total_variation(a_bg)
    k = (norm > 1e-8).to(norm.dtype)
    S = smooth_l1(warped_alpha.detach() * k, fluid_alpha_raw * k)
    losses = dict(zip(LOSS_NAMES, (mse, tv, S.mean(), (S * (1.0 - sma)).mean())))
    return losses, gt, c0


# ---------------------------------------------------------------------------------------------- the analytic backward of csrc/layers.hip

def _sign(d):                                                               # torch.sign: 0 at 0 and at NaN
    return (d > 0).to(d.dtype) - (d < 0).to(d.dtype)


def layer_composite_backward(fluid_raw, bg_raw, fluid_alpha_raw, bg_alpha_raw, g_pred=None, g_fluid=None, g_bg=None, mutant=None):
    """(d fluid_raw, d bg_raw, d fluid_alpha_raw, d bg_alpha_raw) from the gradients reaching pred, fluid and bg (None: absent).
    ``mutant`` "drop_dn": the deliberately wrong backward without the term through n (the mutation check)."""
    F, B = torch.tanh(fluid_raw), torch.tanh(bg_raw)
    af, ab = torch.sigmoid(fluid_alpha_raw), torch.sigmoid(bg_alpha_raw)
    s = af + ab
    n = torch.clamp(s, min=1e-8)
    zero3 = torch.zeros_like(F)
    GF = zero3 if g_fluid is None else g_fluid
    GB = zero3 if g_bg is None else g_bg
    gaf = gab = gn = torch.zeros_like(af)
    if g_pred is not None:
        gnum = g_pred / n
        gn = (-g_pred * (af * F + ab * B) / (n * n)).sum(1, keepdim=True)
        gaf = (gnum * F).sum(1, keepdim=True)
        gab = (gnum * B).sum(1, keepdim=True)
        GF = GF + gnum * af
        GB = GB + gnum * ab
    gs = torch.where(s >= 1e-8, gn, torch.zeros_like(gn))                   # the clamp's backward: where it bites, nothing flows
    if mutant == "drop_dn":
        gs = torch.zeros_like(gn)
    return GF * (1 - F * F), GB * (1 - B * B), (gaf + gs) * (1 - af) * af, (gab + gs) * (1 - ab) * ab


def _tv_grad(x, kx, ky):
    g = torch.zeros_like(x)
    sx = _sign(x[:, :, :, :-1] - x[:, :, :, 1:]) * kx
    sy = _sign(x[:, :, :-1, :] - x[:, :, 1:, :]) * ky
    g[:, :, :, :-1] += sx
    g[:, :, :, 1:] -= sx
    g[:, :, :-1, :] += sy
    g[:, :, 1:, :] -= sy
    return g


def alpha_losses_backward(a_start, mask_rock, small_motion_alpha, warped_alpha, norm, fluid_alpha_raw, g, reweight=True):
    """(d a_start, d fluid_alpha_raw) from g [4], the gradients reaching the four losses."""
    N, _, H, W = a_start.shape
    a0, a1 = a_start[:, 0:1], a_start[:, 1:2]
    sma, r = small_motion_alpha, mask_rock
    m = 1.0 - sma
    sf, sb = torch.sigmoid(a1), torch.sigmoid(a0)
    s = sf + sb
    n = torch.clamp(s, min=1e-8)
    c0 = sf / n
    gt = r * m * 0.25 + (1.0 - r) * m + sma * 0.5
    e = c0 * m - gt * m
    if reweight:
        gerr = g[0] * 0.5 / (1 + (r * m).sum()) * (r * m) + g[0] * 0.5 / (1 + ((1.0 - r) * m).sum()) * ((1.0 - r) * m)
    else:
        gerr = g[0] / e.numel() * torch.ones_like(e)
    gc0 = gerr * (2 * e) * m
    gn = -gc0 * sf / (n * n)
    gs = torch.where(s >= 1e-8, gn, torch.zeros_like(gn))
    gsf, gsb = gc0 / n + gs, gs
    kx, ky = g[1] / (N * H * (W - 1)), g[1] / (N * (H - 1) * W)
    d1 = gsf * (1 - sf) * sf + _tv_grad(a1, kx, ky)
    d0 = (gsb + _tv_grad(sb, kx, ky)) * (1 - sb) * sb
    k = (norm > 1e-8).to(norm.dtype)
    d = warped_alpha * k - fluid_alpha_raw * k
    t = d.abs()
    sg = torch.sigmoid(5 * t)
    gS = g[2] / d.numel() + g[3] / d.numel() * m
    gt_ = gS + gS * 0.2 * (1 - sg) * sg * 5
    return torch.cat([d0, d1], 1), -(gt_ * _sign(d)) * k


# ---------------------------------------------------------------------------------------------- inputs of the operator tests

def head_inputs(N, H, W, seed=0, dtype=torch.float64, rock="mixed"):
    """Inputs of both operators [N,.,H,W] with the cases the kernels can get wrong: a pixel with both logits at -40 in every alpha pair
    (the 1e-8 clamp bites), constant runs along x and y (TV and S at d = 0), norm <= 1e-8 holes, small_motion_alpha all ones for the last sample
    when N > 1 (else for its first row).  ``rock``: "mixed" (random; with N > 1 sample 0 has no rock pixel and the last is all rock),
    "none" or "all": a whole batch without a rock pixel or of rock alone, so that one of the 1 + sum denominators is 1."""
    g, rock_mode = torch.Generator().manual_seed(seed), rock
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    d = {"fluid_raw": rnd(N, 3, H, W) * 1.5, "bg_raw": rnd(N, 3, H, W) * 1.5, "fluid_alpha_raw": rnd(N, 1, H, W) * 2,
         "a_start": rnd(N, 2, H, W) * 2, "warped_alpha": rnd(N, 1, H, W) * 2}
    d["a_start"][0, :, 1, :] = 0.75                                         # constant runs
    d["a_start"][-1, 1, :, W - 1] = -0.5
    d["fluid_alpha_raw"][0, 0, 1, :] = d["warped_alpha"][0, 0, 1, :]        # S at d = 0
    d["a_start"][0, :, 0, 0] = -40.0
    d["a_start"][-1, :, H - 1, W - 1] = -40.0
    d["fluid_alpha_raw"][0, 0, 0, 0] = -40.0                                # with a_start[0, 0, 0, 0]: the composite's clamp
    rock = (torch.rand(N, 1, H, W, generator=g, dtype=torch.float64) < 0.4).double()
    if rock_mode != "mixed":
        rock[:] = 1.0 if rock_mode == "all" else 0.0
    elif N > 1:
        rock[0] = 0.0
        rock[-1] = 1.0
    sma = (torch.rand(N, 1, H, W, generator=g, dtype=torch.float64) < 0.3).double()
    if N > 1:
        sma[-1] = 1.0
    else:
        sma[0, 0, 0] = 1.0
    norm = torch.rand(N, 1, H, W, generator=g, dtype=torch.float64) + 0.1
    norm[torch.rand(N, 1, H, W, generator=g, dtype=torch.float64) < 0.2] = 0.0
    norm[0, 0, 0, 1] = 1e-9
    d.update(mask_rock=rock, small_motion_alpha=sma, norm=norm, bg_alpha_raw=d["a_start"][:, 0:1].clone())
    return {k: v.to(dtype).contiguous() for k, v in d.items()}


COMPOSITE_ARGS = ("fluid_raw", "bg_raw", "fluid_alpha_raw", "bg_alpha_raw")
ALPHA_ARGS = ("a_start", "mask_rock", "small_motion_alpha", "warped_alpha", "norm", "fluid_alpha_raw")


# ---------------------------------------------------------------------------------------------- the whole forward
# AnimatingSoftmaxSplatingJoint.forward (:256-809) under the options of train_alpha_finetuneBG_finetuneFluid_v2.sh, written out from the
# definitions the pieces are tested against (tests/train_step_f64.py's spectral networks and Euler integration, tests/blend_f64.py,
# tests/loss_f64.py) and the head above; and the reader of tests/golden/two_layer_train_vs_reference.npz
# (tools/make_golden_two_layer_train.py: the reference's own float32 run).

import os  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_layer_train_vs_reference.npz")
ENC_WIDTHS, DEC_WIDTHS = [8, 8, 8, 8, 8, 8, 8], [8, 16, 16, 8, 8, 8, 8]
UPDOWN = [None, "Down", "Down", None, "Up", "Up", None, None]
FEAT = 16
PCONV_FORMS = ["input"] + ["pconv"] * 7
# network -> (blocks' key, plain ResNet_Blocks?, channels, resampling), in the reference's registration order
NETWORKS = {"encoder": ("gblocks", True, [3] + ENC_WIDTHS + [FEAT + 1], [None] * 8),
            "net_bg": ("eblocks", True, [3] + DEC_WIDTHS + [3], UPDOWN),
            "net_alpha_encoder": ("gblocks", True, [3] + ENC_WIDTHS + [2], [None] * 8),
            "net_alpha_decoder": ("eblocks", False, [FEAT + 1] + DEC_WIDTHS + [1], UPDOWN),
            "projector": ("eblocks", False, [FEAT] + DEC_WIDTHS + [3], UPDOWN)}
# the noise layers' calls in the reference's order: the encoder runs four times (the first pair is dropped, :349-350)
NOISE_CALLS = {"start_dropped": ("encoder", 0), "end_dropped": ("encoder", 1), "start": ("encoder", 2), "end": ("encoder", 3),
               "bg": ("net_bg", 0), "alpha_start": ("net_alpha_encoder", 0), "alpha_end": ("net_alpha_encoder", 1),
               "projector": ("projector", 0), "alpha_decoder": ("net_alpha_decoder", 0)}


def unpack(g, group):
    """The arrays tools/make_golden_two_layer_train.py::pack wrote under ``group``: name -> float32 array."""
    names = str(g[group + "_names"]).split("\n") if str(g[group + "_names"]) else []
    out, at = {}, 0
    for k, shape in zip(names, g[group + "_shapes"]):
        shape = tuple(int(s) for s in shape if s >= 0)
        n = int(np.prod(shape)) if shape else 1
        out[k] = g[group + "_data"][at:at + n].reshape(shape)
        at += n
    assert at == g[group + "_data"].size
    return out


def load(path=GOLDEN):
    """The fixture as a dict of numpy arrays, the packed groups under "sd/<key>", "noise/<layer>/<call>" and "after/<key>", the key lists
    as lists of strings."""
    z = np.load(path)
    packed = {f"{group}_{part}" for group in ("sd", "noise", "after") for part in ("names", "shapes", "data")}
    g = {k: z[k] for k in z.files if k not in packed}
    for group in ("sd", "noise", "after"):
        g.update({f"{group}/{k}": v for k, v in unpack(z, group).items()})
    for k in ("loss_keys", "pred_keys", "state_keys", "parameter_order"):
        g[k] = str(g[k]).split("\n")
    return g


def options(**more):
    """The options of the fixture as a Namespace, as far as this package reads them."""
    import losses_fixture as LF
    opt = types.SimpleNamespace(model_type="softmax_splating_2layers_alpha_seperate",
                                refine_model_type="resnet_256W8UpDown64_de_resnet_pconv2_nonorm",
                                alpha_refine_model_type="resnet_256W8UpDown64Layers_de_resnet_pconv2_nonorm",
                                bg_refine_model_type="resnet_256W8UpDown64BG_nonorm", pconv="pconv_pbn_woresbias",
                                norm_G="sync:spectral_batch", normalize_image=True, train_Z=True, use_inverse_depth=True,
                                losses=list(LF.LOSSES), discriminator_losses="0", ndf=8, ngf=FEAT, out_channel=FEAT + 1, W=32, max_z=10.0,
                                min_z=0.5, voxel_size=64, gan_mode="hinge", lambda_feat=10.0, no_ganFeat_loss=False, beta1=0.0, beta2=0.9,
                                lr_g=5e-4, lr_d=2e-3, niter_decay=10, use_gt_depth=False, ATVloss=1.0, AKLloss=0.0, ADCloss=1.0,
                                MRADCloss=1.0, AlphaMSEloss=1000.0, use_reweight_mask_loss=True, train_bg=True, train_alpha=True,
                                MVloss=1.0, RockRegionlosstarget=0.25)
    for k, v in more.items():
        setattr(opt, k, v)
    return opt


def model_kwargs():
    """The narrow widths of the fixture as keyword arguments of ``TwoLayerTrainingModel``."""
    return dict(encoder_widths=ENC_WIDTHS, alpha_encoder_widths=ENC_WIDTHS, decoder_widths=DEC_WIDTHS, decoder_updown=UPDOWN,
                alpha_decoder_widths=DEC_WIDTHS, alpha_decoder_updown=UPDOWN, bg_widths=DEC_WIDTHS, bg_updown=UPDOWN)


def state_dict(g, prefix="model.module."):
    import train_step_f64 as T64
    return T64.state_dict(g, prefix)


def noise_lists(g):
    """NOISE_CALLS' key -> per block the (noise1, noise2) pair the reference's layers drew at that call."""
    out = {}
    for key, (net, call) in NOISE_CALLS.items():
        blocks, plain, _, _ = NETWORKS[net]
        a, b = ("ch_a.0", "ch_a.3") if plain else ("bn_noise1", "bn_noise2")
        out[key] = [(torch.from_numpy(g[f"noise/{net}.{blocks}.{i}.{a}/{call}"]), torch.from_numpy(g[f"noise/{net}.{blocks}.{i}.{b}/{call}"]))
                    for i in range(8)]
    return out


def fixture_inputs(g):
    return {"images": [torch.from_numpy(g["images"][k]) for k in range(3)], "mean_video": [torch.from_numpy(g["mean_video"])],
            "motions": torch.from_numpy(g["motions"]), "mask_rock": torch.from_numpy(g["mask_rock"]), "index": torch.from_numpy(g["index"]),
            "noise": noise_lists(g)}


def generator(g, dtype):
    """network -> {"ps", "uvs": the current u / v lists, "forms", "kinds"}, and "leaves": reference key -> requires_grad leaf."""
    import train_step_f64 as T64
    nets, leaves = {}, {}
    for net, (blocks, plain, ch, kinds) in NETWORKS.items():
        names = T64.ENC_NAMES if plain else T64.DEC_NAMES
        ps, uvs = [], []
        for i in range(8):
            head, p, uv = f"{net}.{blocks}.{i}", {}, {}
            used_b = True if plain else (bool(kinds[i]) or ch[i] != ch[i + 1])
            for name, key in names.items():
                k = f"sd/{head}.{key}.weight_orig"
                if k not in g or (name == "w_b" and not used_b):
                    p[name] = None
                    if name in T64.BIASES:
                        p[T64.BIASES[name]] = None
                    continue
                p[name] = torch.from_numpy(g[k]).to(dtype).requires_grad_(True)
                leaves[f"{head}.{key}.weight_orig"] = p[name]
                uv[name] = (torch.from_numpy(g[f"sd/{head}.{key}.weight_u"]).to(dtype), torch.from_numpy(g[f"sd/{head}.{key}.weight_v"]).to(dtype))
                if name in T64.BIASES:
                    b = f"sd/{head}.{key}.bias"
                    p[T64.BIASES[name]] = torch.from_numpy(g[b]).to(dtype).requires_grad_(True) if b in g else None
                    if b in g:
                        leaves[f"{head}.{key}.bias"] = p[T64.BIASES[name]]
            ps.append(p), uvs.append(uv)
        nets[net] = {"ps": ps, "uvs": uvs, "forms": ["res"] * 8 if plain else PCONV_FORMS, "kinds": kinds}
    nets["leaves"] = leaves
    return nets


def _run(nets, name, x, noise, dtype):
    import spectral_f64 as S64
    import train_step_f64 as T64
    n = nets[name]
    fs, uns, _ = T64.network(n["forms"], x, n["ps"], n["uvs"], n["kinds"], S64.cast(noise, dtype))
    n["uvs"] = uns
    return fs[-1]["y"]


def model_forward(nets, inp, dtype, opts=None, literal_encoder_calls=True):
    """(loss dict, pred dict) on the leaves of ``nets`` (``generator``), whose u / v lists advance; differentiable by autograd."""
    import blend_f64 as BL64
    import loss_f64 as L64
    import losses_fixture as LF
    import spectral_f64 as S64
    import train_step_f64 as T64
    opts = options() if opts is None else opts
    a = lambda t: S64.cast(t, dtype)                                          # noqa: E731
    images, motion, index, nz = a(list(inp["images"])), a(inp["motions"]), inp["index"], inp["noise"]
    mean_img, rock = a(inp["mean_video"][0]), a(inp["mask_rock"])
    start, middle, end = images
    flow = motion if motion.shape[1] == 2 else motion[:, :2] * motion[:, 2:3]
    speed = (flow[:, 0:1] ** 2 + flow[:, 1:2] ** 2).sqrt()                     # :334-339
    sma = (speed < speed.mean([1, 2, 3], True) * 0.1).to(dtype)
    if literal_encoder_calls:                                                  # :349-350
        with torch.no_grad():
            _run(nets, "encoder", start, nz["start_dropped"], dtype)
            _run(nets, "encoder", end, nz["end_dropped"], dtype)
    ys, ye = _run(nets, "encoder", start, nz["start"], dtype), _run(nets, "encoder", end, nz["end"], dtype)
    (start_fs, Z_f), (end_fs, Z_p) = (ys[:, :-1], ys[:, -1:]), (ye[:, :-1], ye[:, -1:])
    bg_raw = _run(nets, "net_bg", start, nz["bg"], dtype)
    a_start = _run(nets, "net_alpha_encoder", start, nz["alpha_start"], dtype)
    a_end = _run(nets, "net_alpha_encoder", end, nz["alpha_end"], dtype)
    s, m, e = index[:, 0], index[:, 1], index[:, 2]
    flow_f, flow_p = T64.euler(flow, m - s), T64.euler(-flow, e + 1 - m)       # :454-455
    alpha = torch.clamp(1.0 - (m - s).to(dtype) / (e - s + 1).to(dtype), min=1.0 / 600.0, max=599.0 / 600.0)      # :459-461
    train_z = bool(getattr(opts, "train_Z", False))
    splat, norm = BL64.blend_f64(torch.cat([start_fs, a_start[:, 1:2]], 1), Z_f if train_z else None, flow_f,
                                 torch.cat([end_fs, a_end[:, 1:2]], 1), Z_p if train_z else None, flow_p, alpha, dtype, return_norm=True)
    fluid_raw = _run(nets, "projector", splat[:, :FEAT], nz["projector"], dtype)
    fluid_alpha_raw = _run(nets, "net_alpha_decoder", splat, nz["alpha_decoder"], dtype)
    pred, fluid, bg, ca = layer_composite(fluid_raw, bg_raw, fluid_alpha_raw, a_start[:, 0:1])
    vgg = LF.vgg19_state_dict()
    loss = L64.synthesis_loss(pred, middle, vgg, tuple(opts.losses), dtype)
    loss.pop("distances", None)
    terms, gt, _ = alpha_losses(a_start, rock, sma, splat[:, FEAT:].detach(), norm.detach(), fluid_alpha_raw,
                                reweight=bool(getattr(opts, "use_reweight_mask_loss", False)))
    for weight, name in (("AlphaMSEloss", LOSS_NAMES[0]), ("ATVloss", LOSS_NAMES[1])):
        if getattr(opts, weight, 0.0) > 0.0:
            loss[name] = terms[name]
            loss["Total Loss"] = loss["Total Loss"] + terms[name] * getattr(opts, weight)
    if getattr(opts, "MVloss", 0.0) > 0.0:
        lb = L64.synthesis_loss(bg, mean_img, vgg, tuple(opts.losses), dtype)
        lb.pop("distances", None)
        for k in lb:
            if "Perceptual" in k or "L1" in k:
                loss[k + "_bg"] = lb[k]
            elif "Total" in k:
                loss[k] = loss[k] + lb[k] * opts.MVloss
    for weight, name in (("ADCloss", LOSS_NAMES[2]), ("MRADCloss", LOSS_NAMES[3])):
        if getattr(opts, weight, 0.0) > 0.0:
            loss[name] = terms[name]
            loss["Total Loss"] = loss["Total Loss"] + terms[name] * getattr(opts, weight)
    with torch.no_grad():
        z = Z_f.detach() if train_z else torch.ones_like(Z_f)
        z = torch.clamp(z - z.max(), min=-20.0, max=20.0)
    pred_dict = {"OutputImg": middle, "PredImg": pred, "BGImg_f": bg, "MeanImg": mean_img, "FluidImg": fluid,
                 "AlphaFluid_f": torch.sigmoid(a_start[:, 1:2]), "AlphaBG_f": torch.sigmoid(a_start[:, 0:1]), "CompositeFluidAlpha": ca,
                 "Z_f": z, "GTMotion": flow, "GTAlpha": gt, "RockMask": rock}
    return loss, pred_dict


def forward(g, dtype=torch.float64, opts=None, literal_encoder_calls=True):
    """The whole forward on the fixture's inputs without gradients: (loss, pred_dict, nets) -- nets with the u / v lists after it."""
    nets = generator(g, dtype)
    with torch.no_grad():
        loss, pred = model_forward(nets, fixture_inputs(g), dtype, opts, literal_encoder_calls)
    return loss, pred, nets
