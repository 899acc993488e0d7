"""The forward of the reference's training model (models/animating_softmax_splating.py:445-775, the configuration of
train_baseline2_pconv.sh) written out in any dtype from the definitions the pieces are tested against -- TEST INFRASTRUCTURE ONLY (no
tests here): ``spectral_f64.network`` (the encoder on the start and on the end image, two power iterations; the decoder), the Euler
integration written below, ``blend_f64``, ``tanh``, ``loss_f64.synthesis_loss``.  Also the reader of
tests/golden/train_step_vs_reference.npz (tools/make_golden_train_step.py: the reference's own float32 run), which supplies the inputs,
the initial state, the noise and the reference's key lists.  tests/test_train_step_host.py pins the definition to the reference's values."""
import os
import types

import numpy as np
import torch

import blend_f64 as BL64
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


def forward(g, dtype=torch.float64, training=True):
    """The forward on the fixture's inputs in ``dtype``: {"loss": {...}, "PredImg", "Z_f", "gen_fs", the new (u, v) lists}."""
    a = lambda t: S64.cast(t, dtype)                                          # noqa: E731
    (eps_, euv), (dps, duv) = block_lists(g, dtype)
    nz = noise_lists(g)
    images, motion, index = a(torch.from_numpy(g["images"])), a(torch.from_numpy(g["motions"])), torch.from_numpy(g["index"])
    feats = []
    for img, noise in ((images[0], nz["start"]), (images[2], nz["end"])):      # :486-487: u and v move at each call
        fs, euv, _ = S64.network(["res"] * 8, img, eps_, euv, [None] * 8, a(noise), training)
        y = fs[-1]["y"]
        feats.append((y[:, :-1], y[:, -1:]))
    (start_fs, Z_f), (end_fs, Z_p) = feats
    s, m, e = index[:, 0], index[:, 1], index[:, 2]
    flow_f, flow_p = euler(motion, m - s), euler(-motion, e + 1 - m)           # :579-580
    alpha = (1.0 - (m - s).to(dtype) / (e - s + 1).to(dtype))                  # :585
    gen_fs = BL64.blend_f64(start_fs, Z_f, flow_f, end_fs, Z_p, flow_p, alpha, dtype)
    fs, duv, _ = S64.network(["input"] + ["pconv"] * 7, gen_fs, dps, duv, UPDOWN, a(nz["projector"]), training)
    pred = torch.tanh(fs[-1]["y"])
    loss = L64.synthesis_loss(pred, images[1], LF.vgg19_state_dict(), tuple(LF.LOSSES), dtype)
    z = torch.clamp(Z_f - Z_f.max(), min=-20.0, max=20.0)                      # :601-605
    return {"loss": loss, "PredImg": pred, "Z_f": z, "gen_fs": gen_fs, "flow_f": flow_f, "flow_p": flow_p, "encoder_uv": euv, "decoder_uv": duv}
