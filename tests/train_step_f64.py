"""The forward of the reference's training model (models/animating_softmax_splating.py:445-775, the configuration of
train_baseline2_pconv.sh) written out in any dtype from the definitions the pieces are tested against -- TEST INFRASTRUCTURE ONLY (no
tests here): ``spectral_f64.network`` (the encoder on the start and on the end image, two power iterations; the decoder), the Euler
integration written below, ``blend_f64``, ``tanh``, ``loss_f64.synthesis_loss``.  Also the reader of
tests/golden/train_step_vs_reference.npz (tools/make_golden_train_step.py: the reference's own float32 run), which supplies the inputs,
the initial state, the noise and the reference's key lists.  tests/test_train_step_host.py pins the definition to the reference's values.

The same path is differentiable: ``generator`` makes a ``requires_grad`` leaf of every weight_orig, gain, bias and convolution bias under
its reference key, ``generator_forward`` runs encoder twice -> Euler -> blend -> decoder -> tanh on any inputs (the fixture's by default)
and torch autograd supplies the gradients.  The power iteration runs under ``no_grad`` on the detached weight, so u, v and hence the
direction of sigma are constants of the backward, as in torch's spectral_norm and in ``spectral_f64.weight_orig_grad``
(tests/test_train_step_host.py: autograd's leaves ARE ``spectral_f64.network_grads``').  ``chain_gradients`` is the generator alone under a
given gradient at PredImg, ``iteration_gradients`` models/base_model.py:95-163 with ``disc_f64`` for the discriminator.  ``MUTANTS`` are
deliberately wrong compositions of the same pieces, the host tests' evidence that the criterion tells them from float32 rounding."""
import os
import types

import numpy as np
import torch

import blend_f64 as BL64
import conv_train_f64 as C64
import block_train_f64 as B64
import disc_f64 as DI64
import loss_f64 as L64
import losses_fixture as LF
import spectral_f64 as S64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step_vs_reference.npz")
ENC_WIDTHS, DEC_WIDTHS = [8, 8, 8, 16, 16, 16, 16], [16, 24, 24, 16, 16, 16, 8]            # tests/test_gpu_spectral.py's, feat = 16
UPDOWN = [None, "Down", "Down", None, "Up", "Up", None, None]
FEAT, NDF = 16, 8
ENC_NAMES = {"gain1": "ch_a.0.gain", "bias1": "ch_a.0.bias", "w_aa": "ch_a.2", "gain2": "ch_a.3.gain", "bias2": "ch_a.3.bias", "w_ab": "ch_a.5",
             "w_b": "ch_b.0"}
DEC_NAMES = {"gain1": "bn_noise1.gain", "bias1": "bn_noise1.bias", "w_aa": "conv_aa", "gain2": "bn_noise2.gain", "bias2": "bn_noise2.bias",
             "w_ab": "conv_ab", "w_b": "conv_b"}
BIASES = {"w_aa": "b_aa", "w_ab": "b_ab", "w_b": "b_b"}


def load(path=GOLDEN):
    """The fixture as a dict of numpy arrays."""
    g = np.load(path)
    return {k: g[k] for k in g.files}


def options(**more):
    """The training options of the fixture as a Namespace (what the reference's parser made of train_baseline2_pconv.sh's flags, as far
    as this package reads them)."""
    opt = types.SimpleNamespace(model_type="softmax_splating", refine_model_type="resnet_256W8UpDown64_de_resnet_pconv2_nonorm",
                                pconv="pconv_pbn_woresbias", norm_G="sync:spectral_batch", normalize_image=True, train_Z=True,
                                use_softmax_splatter=True, use_inverse_depth=True, losses=list(LF.LOSSES), discriminator_losses="pix2pixHD",
                                ndf=NDF, ngf=FEAT, out_channel=FEAT, W=32, Z_model="encoder", max_z=10.0, min_z=0.5, voxel_size=64,
                                gan_mode="hinge", lambda_feat=10.0, no_ganFeat_loss=False, beta1=0.0, beta2=0.9, lr_g=5e-4, lr_d=2e-3,
                                niter_decay=10, use_gt_depth=False)
    for k, v in more.items():
        setattr(opt, k, v)
    return opt


def state_dict(g, prefix="model.module."):
    """The fixture's initial state as a reference state dict (float32 tensors), the VGG19 of tests/losses_fixture.py under the
    reference's keys."""
    sd = {prefix + k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")}
    for k, v in LF.vgg19_state_dict().items():
        idx = int(k.split(".")[1])
        s = max(i for i, a in enumerate((0, 2, 7, 12, 21)) if a <= idx) + 1
        sd[f"{prefix}loss_function.losses.1.model.slice{s}.{idx}.{k.split('.')[2]}"] = v
    return sd


def noise_lists(g):
    """{"start", "end", "projector"}: per block the (noise1, noise2) pair the reference's layers drew."""
    enc = lambda call: [(torch.from_numpy(g[f"noise/encoder.gblocks.{i}.ch_a.0/{call}"]), torch.from_numpy(g[f"noise/encoder.gblocks.{i}.ch_a.3/{call}"]))  # noqa: E731
                        for i in range(8)]
    dec = [(torch.from_numpy(g[f"noise/projector.eblocks.{i}.bn_noise1/0"]), torch.from_numpy(g[f"noise/projector.eblocks.{i}.bn_noise2/0"]))
           for i in range(8)]
    return {"start": enc(0), "end": enc(1), "projector": dec}


def block_lists(g, dtype):
    """(ps, uvs) of the encoder and of the decoder in spectral_f64's form.  The decoder's conv_b is a parameter of every block there and
    used only where the block resamples or changes its width (blocks.py:243-247)."""
    def one(head, names, used_b):
        p, uv = {}, {}
        for name, key in names.items():
            k = f"sd/{head}.{key}.weight_orig"
            if k not in g or (name == "w_b" and not used_b):
                p[name] = None
                if name in BIASES:
                    p[BIASES[name]] = None
                continue
            p[name] = torch.from_numpy(g[k]).to(dtype)
            uv[name] = (torch.from_numpy(g[f"sd/{head}.{key}.weight_u"]).to(dtype), torch.from_numpy(g[f"sd/{head}.{key}.weight_v"]).to(dtype))
            if name in BIASES:
                b = f"sd/{head}.{key}.bias"
                p[BIASES[name]] = torch.from_numpy(g[b]).to(dtype) if b in g else None
        return p, uv
    ech, dch = [3] + ENC_WIDTHS + [FEAT + 1], [FEAT] + DEC_WIDTHS + [3]
    enc = [one(f"encoder.gblocks.{i}", ENC_NAMES, True) for i in range(8)]
    dec = [one(f"projector.eblocks.{i}", DEC_NAMES, bool(UPDOWN[i]) or dch[i] != dch[i + 1]) for i in range(8)]
    assert all((p["w_b"] is not None) == (ech[i] != ech[i + 1]) for i, (p, _) in enumerate(enc))
    return ([p for p, _ in enc], [u for _, u in enc]), ([p for p, _ in dec], [u for _, u in dec])


def euler(motion, steps):
    """models/projection/euler_integration_manipulator.py:7-56 per sample, in motion's dtype: ``steps[b]`` times the motion at the rounded
    position is added; a pixel that ever leaves the frame gets the displacement max(H, W) + 1 (``steps[b]`` = 0: zeros)."""
    B, _, H, W = motion.shape
    y, x = torch.meshgrid(torch.arange(H, dtype=motion.dtype), torch.arange(W, dtype=motion.dtype), indexing="ij")
    coord = torch.stack([x, y])
    out = torch.zeros_like(motion)
    for b in range(B):
        dest, invalid = coord.clone(), torch.zeros(H, W, dtype=torch.bool)
        for _ in range(int(steps[b])):
            dest = dest + motion[b][:, torch.round(dest[1]).long(), torch.round(dest[0]).long()]
            invalid = invalid | (dest[0] > W - 1) | (dest[0] < 0) | (dest[1] > H - 1) | (dest[1] < 0)
            dest = torch.where(invalid, coord, dest)
            out[b] = torch.where(invalid, torch.full_like(dest, float(max(H, W) + 1)), dest - coord)
    return out


# ------------------------------------------------------------------ inputs

def fixture_inputs(g):
    """The fixture's batch: {"images": [start, middle, end], "motions", "index" [B,3], "noise": noise_lists(g)}, float32."""
    return {"images": [torch.from_numpy(g["images"][k]) for k in range(3)], "motions": torch.from_numpy(g["motions"]),
            "index": torch.from_numpy(g["index"]), "noise": noise_lists(g)}


# What the second batch of an accumulation adds to the middle and to the end index of the first.  The end offset is the first of 5, 4, 3,
# ... at which the float32 run of the definition keeps E_plain32 <= 0.03 on every tensor in every case of the loose level: with 5 the case
# without the discriminator over two batches reaches 3.2e-2 on encoder.gblocks.0.ch_b.0.weight_orig, with 4 its largest is 1.6e-2
# (tests/test_train_step_host.py asserts the condition for all four cases).
SECOND_OFFSETS = (2, 4)


def second_batch(inp):
    """The second batch of an accumulation, as tests/test_gpu_train_step.py::_batches builds it: start and end exchanged, the motion
    reversed, other indices (SECOND_OFFSETS), the noise pairs exchanged."""
    img, nz, index = inp["images"], inp["noise"], inp["index"]
    return {"images": [img[2], img[0], img[1]], "motions": (-inp["motions"]).contiguous(),
            "index": torch.stack([index[:, 0], index[:, 1] + SECOND_OFFSETS[0], index[:, 2] + SECOND_OFFSETS[1]], 1),
            "noise": {"start": nz["end"], "end": nz["start"], "projector": [(b, a) for a, b in nz["projector"]]}}


CLEAN_INDEX = [[0, 2, 5], [1, 4, 6]]
# train_Z -> (the seed of the first batch, the seed of a second accumulated batch): per batch the first seed from 0 at which the smallest
# float64 |pre-activation| over the batch's 48 batch-norm evaluations (2 encoder calls x 16 + 16 in the decoder, kept elements only where
# a mask applies) exceeds MARGIN -- the second batch in the state (u, v) the first one leaves.  The decoder's pre-activations depend on
# train_Z, hence a pair per setting.  Found by ``first_clean_seed``: 14, 52 and 82 within its limit of 200 seeds.  623 is NOT: after
# seed 14 no second batch below 200 is clean (the settled u / v leave the encoder's last blocks smaller pre-activations), so that one
# search went on to 1000 -- DESIGN 3.15 states the deviation.  tests/test_train_step_host.py asserts every margin, and that 14, 52 and 82
# are the first of their searches (the 624 forwards that would show the same of 623 take half a minute and are not repeated there).
CLEAN_SEEDS = {True: (14, 623), False: (52, 82)}
MARGIN = 1e-4


def clean_case(g, seed, W=8):
    """The small case of the tight level: batch 2, W x W, the fixture's weights and noise, images tanh(randn), motions 0.4 randn on a
    grid of 1/64 (every position, rounding and bounds decision of the Euler integration and every splat corner is then exact in float32
    and float64 alike), the index of CLEAN_INDEX, and the gradient at PredImg randn (1 + arange(W) / W) / numel -- all from ONE
    generator seeded with ``seed``.  Returns (inputs, gpred)."""
    gen = torch.Generator().manual_seed(seed)
    images = [torch.tanh(torch.randn(2, 3, W, W, generator=gen)) for _ in range(3)]
    motions = torch.round(0.4 * torch.randn(2, 2, W, W, generator=gen) * 64.0) / 64.0
    gpred = torch.randn(2, 3, W, W, generator=gen) * (1.0 + torch.arange(W) / W) / float(2 * 3 * W * W)
    return {"images": images, "motions": motions, "index": torch.tensor(CLEAN_INDEX), "noise": noise_lists(g)}, gpred


def clean_batches(g, train_z=True, n=1, W=8):
    """([inputs], [gpred]) of the tight level: ``clean_case`` at the first n seeds of CLEAN_SEEDS[train_z]."""
    cases = [clean_case(g, seed, W) for seed in CLEAN_SEEDS[bool(train_z)][:n]]
    return [c[0] for c in cases], [c[1] for c in cases]


def first_clean_seed(g, opts, before=(), limit=200, W=8):
    """(seed, margin): the first seed whose ``clean_case``, run after the batches ``before``, keeps every kept pre-activation MARGIN from
    zero in float64.  None if there is none below ``limit``."""
    base = generator(g, torch.float64)
    with torch.no_grad():
        for inp in before:
            generator_forward(base, inp, torch.float64, opts)
        for seed in range(limit):
            net = dict(base)
            m = margin(generator_forward(net, clean_case(g, seed, W)[0], torch.float64, opts)["pre"])
            if m > MARGIN:
                return seed, m
    return None


# ------------------------------------------------------------------ the criterion

def cancels(key):
    """The bias of a block's first convolution: a batch-statistics batch-norm follows, which removes a constant per channel, so its
    gradient is zero in exact arithmetic (to O(eps / count) under the partial norm) and E, which divides by max|ref|, means nothing."""
    return key.endswith("ch_a.2.bias") or key.endswith("conv_aa.bias")


def figures(got, ref64, plain32, zero_terms=None):
    """{key: (e, e_plain32, bound)} for dicts of tensors under the same keys: e = E(got, ref64) <= bound = 10 E(plain32, ref64) + 1e-6 is
    the project's criterion.  For the keys of ``cancels`` (and of ``zero_terms``: key -> magnitude of the cancelling terms) the three
    are max|got|, max|plain32| and 10 max|plain32| + 1e-6 terms, each divided by terms -- terms: max|gradient of that convolution's
    weight|."""
    out = {}
    for k, r in ref64.items():
        a, p = got[k].detach().cpu().double(), plain32[k].detach().cpu().double()
        terms = None
        if zero_terms is not None and k in zero_terms:
            terms = float(zero_terms[k])
        elif cancels(k):
            terms = float(ref64[k[:-len("bias")] + "weight_orig"].abs().max())
        if terms is None:
            e, ep = C64.E(a, r), C64.E(p, r)
        else:
            e, ep = float(a.abs().max()) / terms, float(p.abs().max()) / terms
        out[k] = (e, ep, 10.0 * ep + 1e-6)
    return out


DISC_SEED = 11              # torch.manual_seed of the discriminator's initialisation, on the host and on the device


def final_bias(key):
    """The bias of a discriminator's final convolution (under disc_f64's key, with or without a prefix)."""
    return key.endswith("model4.0.bias")


def final_bias_terms(grads_D, n_batches):
    """{key: terms} for the bias of each discriminator's final convolution: its gradient in the discriminator step is (open fake
    gates - open real gates) / (num_D numel) (/ weight, summed over the batches), which is exactly zero while every hinge gate is open --
    as with the 0.02 xavier initialisation, whose final maps are ~1e-3.  terms: the sum of the magnitudes of what cancels, 2 / num_D
    per batch / weight = n_batches ** 2."""
    return {k: float(n_batches) ** 2 for k in grads_D if final_bias(k)}


# ------------------------------------------------------------------ the generator with leaves

MUTANTS = ("end_dropped",      # (a) the end image's encoder call does not reach the encoder's gradients
           "through_power",    # (b) the gradient flows through the power iteration
           "first_uv",         # (c) u / v of the FIRST encoder call in the rank-one term of both calls
           "overwrite",        # (d) the second accumulated batch overwrites the first
           "no_gan",           # (e) the GAN + feature-matching term is missing at PredImg
           "no_weight",        # (f) the factor 1 / weight is omitted
           "stale_d_uv")       # (g) the discriminator step runs with the u / v from before the generator step


def generator(g, dtype):
    """{"enc": ps, "dec": ps, "euv", "duv": the current u / v lists, "leaves": reference key -> requires_grad leaf} in ``dtype``."""
    (eps_, euv), (dps, duv) = block_lists(g, dtype)
    leaves = {}
    for head, names, ps in (("encoder.gblocks", ENC_NAMES, eps_), ("projector.eblocks", DEC_NAMES, dps)):
        for i, p in enumerate(ps):
            for name, key in names.items():
                for field, tail in ((name, "weight_orig"), (BIASES.get(name), "bias")):
                    if field is not None and p.get(field) is not None:
                        p[field] = p[field].clone().requires_grad_(True)
                        leaves[f"{head}.{i}.{key}.{tail}"] = p[field]
    return {"enc": eps_, "dec": dps, "euv": euv, "duv": duv, "leaves": leaves}


def network(forms, x, ps, uvs, kinds, noises, through_power=False, sigma_uvs=None):
    """``spectral_f64.network`` in training mode for leaves: ``spectral_f64.power_iteration`` under no_grad on the detached weight, then
    sigma = u^T W v differentiated in W alone.  Same return: (the blocks' dicts with x and mask, the new uvs, the ctxs).
    Mutants: through_power differentiates the iteration as well; sigma_uvs gives sigma its value from this call's (u, v) and its
    derivative from those."""
    fs, uns, ctxs, mask = [], [], [], None
    for i, p in enumerate(ps):
        pe, un, inv = dict(p), {}, {}
        for k in S64.names_of(p):
            if through_power:
                u, v = S64.power_iteration(p[k], *uvs[i][k])
            else:
                with torch.no_grad():
                    u, v = S64.power_iteration(p[k].detach(), *uvs[i][k])
            s = S64.sigma(p[k], u, v)
            if sigma_uvs is not None:
                other = S64.sigma(p[k], *sigma_uvs[i][k])
                s = s.detach() + (other - other.detach())
            un[k], inv[k] = (u.detach(), v.detach()), 1.0 / s
            pe[k] = p[k] * inv[k]
        gains, biases = S64.tables(pe, noises[i])
        fwd = S64.BLOCKS[forms[i]][0]
        f = fwd(x, mask, pe, kinds[i], gains, biases) if forms[i] == "pconv" else fwd(x, pe, kinds[i], gains, biases)
        f["x"], f["mask"] = x, mask
        fs.append(f), uns.append(un), ctxs.append((pe, inv, gains, biases))
        x, mask = f["y"], f.get("um")
    return fs, uns, ctxs


ENC_FORMS, DEC_FORMS = ["res"] * 8, ["input"] + ["pconv"] * 7


def pre_activations(forms, fs, ctxs):
    """[(|y| of the pre-activation, kept) per BN evaluation], detached: two per block.  kept: where the gate reaches anything -- the
    non-zero elements under the per-element mask of the decoder's first block, the mask of a partial block, everything elsewhere."""
    out = []
    with torch.no_grad():
        for form, f, (pe, inv, gains, biases) in zip(forms, fs, ctxs):
            x, mask = f["x"], f["mask"]
            keep1 = (x != 0) if form == "input" else (torch.ones_like(x, dtype=torch.bool) if mask is None else (mask != 0).expand_as(x))
            um1 = f.get("um1")
            keep2 = torch.ones_like(f["o1"], dtype=torch.bool) if um1 is None else (um1 != 0).expand_as(f["o1"])
            for t, mean, var, gain, bias, keep in ((x, f["mean1"], f["var1"], gains[0], biases[0], keep1),
                                                   (f["o1"], f["mean2"], f["var2"], gains[1], biases[1], keep2)):
                scale, shift = B64.bn_tables(mean, var, gain, bias)
                out.append(((t * B64._t(scale) - B64._t(shift)).abs().detach(), keep))
    return out


def margin(pre):
    """The smallest |pre-activation| over the kept elements of every BN evaluation of ``pre_activations``."""
    return min(float(y[k].min()) for y, k in pre if bool(k.any()))


def generator_forward(net, inp, dtype, opts=None, mutants=()):
    """Encoder on the start and on the end image (u and v move at each call), Euler, blend, decoder, tanh -- on the leaves of ``net``,
    whose u / v lists advance.  Returns PredImg, gen_fs (its gradient retained), Z_f, the flows, the (u, v) lists after each encoder call
    and after the decoder, and the BN pre-activations."""
    opts = options() if opts is None else opts
    a = lambda t: S64.cast(t, dtype)                                          # noqa: E731
    images, motion, index, nz = a(list(inp["images"])), a(inp["motions"]), inp["index"], inp["noise"]
    feats, pre, enc_uvs, calls = [], [], [], []
    for call, (img, noise) in enumerate(((images[0], nz["start"]), (images[2], nz["end"]))):      # :486-487
        fs, uns, ctxs = network(ENC_FORMS, img, net["enc"], net["euv"], [None] * 8, a(noise), "through_power" in mutants,
                                enc_uvs[0] if call == 1 and "first_uv" in mutants else None)
        net["euv"] = uns
        enc_uvs.append(uns)
        calls.append((fs, uns, ctxs, a(noise)))
        pre += pre_activations(ENC_FORMS, fs, ctxs)
        y = fs[-1]["y"]
        if call == 1 and "end_dropped" in mutants:
            y = y.detach()
        feats.append((y[:, :-1], y[:, -1:]))
    (start_fs, Z_f), (end_fs, Z_p) = feats
    if "relu" in str(getattr(opts, "Z_model", "encoder")):                      # :488-490
        Z_f, Z_p = torch.relu(Z_f), torch.relu(Z_p)
    s, m, e = index[:, 0], index[:, 1], index[:, 2]
    flow_f, flow_p = euler(motion, m - s), euler(-motion, e + 1 - m)           # :579-580
    alpha = (1.0 - (m - s).to(dtype) / (e - s + 1).to(dtype))                  # :585
    train_z = bool(getattr(opts, "train_Z", False))
    gen_fs = BL64.blend_f64(start_fs, Z_f if train_z else None, flow_f, end_fs, Z_p if train_z else None, flow_p, alpha, dtype)
    if gen_fs.requires_grad:
        gen_fs.retain_grad()
    fs, duv, ctxs = network(DEC_FORMS, gen_fs, net["dec"], net["duv"], UPDOWN, a(nz["projector"]), "through_power" in mutants)
    net["duv"] = duv
    pre += pre_activations(DEC_FORMS, fs, ctxs)
    pred = torch.tanh(fs[-1]["y"])
    with torch.no_grad():
        z = Z_f.detach() if train_z else torch.ones_like(Z_f)
        z = torch.clamp(z - z.max(), min=-20.0, max=20.0)                      # :601-605
    return {"PredImg": pred, "Z_f": z, "gen_fs": gen_fs, "flow_f": flow_f, "flow_p": flow_p, "encoder_uvs": enc_uvs,
            "encoder_uv": enc_uvs[1], "decoder_uv": duv, "pre": pre, "encoder_calls": calls, "decoder": (fs, duv, ctxs, a(nz["projector"])), "middle": images[1]}


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def chain_gradients(inputs, gpred, dtype=torch.float64, opts=None, mutants=(), g=None):
    """The generator alone: per batch of ``inputs`` (one dict, or a list for an accumulation) the forward and
    ``PredImg.backward(gpred)``; the leaves' gradients add up and u / v move on.  Returns {"grads": reference key -> gradient, "gen_fs":
    [the gradient at gen_fs per batch], "PredImg": [...], "pre": [the BN pre-activations per batch], "margin": the smallest of them,
    "encoder_uvs": [per batch the (u, v) lists after the start and after the end call], "decoder_uv": [...], "flows": [...]}."""
    net = generator(load() if g is None else g, dtype)
    out = {"gen_fs": [], "PredImg": [], "pre": [], "encoder_uvs": [], "decoder_uv": [], "flows": [], "holes": []}
    for n, (inp, gp) in enumerate(zip(_as_list(inputs), _as_list(gpred))):
        if n and "overwrite" in mutants:
            for t in net["leaves"].values():
                t.grad = None
        f = generator_forward(net, inp, dtype, opts, mutants)
        f["PredImg"].backward(gp.to(dtype))
        out["gen_fs"].append(f["gen_fs"].grad.detach()), out["PredImg"].append(f["PredImg"].detach()), out["pre"].append(f["pre"])
        out["encoder_uvs"].append(f["encoder_uvs"]), out["decoder_uv"].append(f["decoder_uv"])
        out["flows"].append((f["flow_f"], f["flow_p"])), out["holes"].append(int((f["gen_fs"].detach() == 0).sum()))
    out["grads"] = {k: (torch.zeros_like(t) if t.grad is None else t.grad.detach().clone()) for k, t in net["leaves"].items()}
    out["margin"] = min(margin(p) for p in out["pre"])
    return out


def iteration_gradients(inputs_list, P_disc=None, dtype=torch.float64, use_d=True, opts=None, mutants=(), g=None):
    """models/base_model.py:95-163 in ``dtype``.  Per batch the generator's backward is of (synthesis Total + GAN Total) / weight, weight
    = 1 / len(inputs_list): ``loss_f64.synthesis_loss`` through autograd, ``disc_f64.generator_step`` for the GAN and feature-matching
    losses, their gradient to the fake image and the u / v it leaves; then ``disc_f64.discriminator_step`` on the detached predictions
    with those u / v.  P_disc: the discriminator's initial state under disc_f64's keys.  Returns {"grads_G": reference key -> gradient
    in front of the generator's optimiser step, "grads_D": disc_f64 key -> gradient in front of the discriminator's, "losses": what the
    trainer returns, "PredImg": the last batch's}."""
    opts = options() if opts is None else opts
    net = generator(load() if g is None else g, dtype)
    vgg, lam = LF.vgg19_state_dict(), float(getattr(opts, "lambda_feat", 10.0))
    batches = _as_list(inputs_list)
    scale = 1.0 if "no_weight" in mutants else float(len(batches))            # 1 / weight
    P0 = P = None if not use_d else {k: v.to(dtype) for k, v in P_disc.items()}
    kept, losses = [], {}
    for n, inp in enumerate(batches):
        if n and "overwrite" in mutants:
            for t in net["leaves"].values():
                t.grad = None
        f = generator_forward(net, inp, dtype, opts, mutants)
        pred, middle = f["PredImg"], f["middle"]
        t_losses = L64.synthesis_loss(pred, middle, vgg, tuple(opts.losses), dtype)
        roots, seeds = [t_losses["Total Loss"] * scale], [None]
        if use_d:
            g_losses, _, dg, P = DI64.generator_step(P, pred.detach(), middle, lam)
            if "no_gan" not in mutants:
                roots.append(pred), seeds.append(dg["fake"] * scale)
        torch.autograd.backward(roots, seeds)
        kept.append((pred.detach(), middle))
    losses.update({k: v.detach() for k, v in t_losses.items() if k != "distances"})
    out = {"grads_G": {k: (torch.zeros_like(t) if t.grad is None else t.grad.detach().clone()) for k, t in net["leaves"].items()},
           "PredImg": kept[-1][0], "encoder_uv": net["euv"], "decoder_uv": net["duv"]}
    if use_d:
        if "stale_d_uv" in mutants:
            P = P0
        grads_D = None
        for pred, middle in kept:
            d_losses, dd, P = DI64.discriminator_step(P, pred, middle)
            grads_D = {k: v * scale for k, v in dd.items()} if grads_D is None else {k: grads_D[k] + v * scale for k, v in dd.items()}
        out["grads_D"], out["P"] = grads_D, P
        losses.update({k: v.detach() for d in (g_losses, d_losses) for k, v in d.items() if k != "Total Loss"})
    out["losses"] = losses
    return out


def forward(g, dtype=torch.float64, inputs=None, opts=None):
    """The training model's forward (u and v move, the statistics are the batch's) on the fixture's inputs (or ``inputs``) in
    ``dtype``: {"loss": {...}, "PredImg", "Z_f", "gen_fs", the new (u, v) lists}.  No gradients are kept."""
    opts = options() if opts is None else opts
    with torch.no_grad():
        f = generator_forward(generator(g, dtype), fixture_inputs(g) if inputs is None else inputs, dtype, opts)
        loss = L64.synthesis_loss(f["PredImg"], f["middle"], LF.vgg19_state_dict(), tuple(opts.losses), dtype)
    return {"loss": loss, "PredImg": f["PredImg"], "Z_f": f["Z_f"], "gen_fs": f["gen_fs"], "flow_f": f["flow_f"], "flow_p": f["flow_p"],
            "encoder_uv": f["encoder_uv"], "decoder_uv": f["decoder_uv"]}
