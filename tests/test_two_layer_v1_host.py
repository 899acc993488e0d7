"""Host-side checks of the v1 two-layer model (``blend_alpha0``, ``TwoLayerAlpha0TrainingModel``; csrc/layers.hip, ABI 25), none of which
needs a GPU: the entry points and their refusals, the operator's argument checks, the analytic backward the kernel computes
(tests/two_layer_v1_f64.py) against float64 autograd of the definition, the written-out forward in float64 against the reference's own
run under the v1 script's options (tests/golden/two_layer_v1_train_vs_reference.npz) -- and two near misses of v1 that must fall outside
the same bound --, the v1 script's option line, and every refused flag."""
import argparse
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import two_layer_f64 as D
import two_layer_v1_f64 as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("slr_blend_alpha0_ws_bytes", "slr_blend_alpha0_forward", "slr_blend_alpha0_backward")
P = 0x7F0000100000                                                           # a 16-byte aligned address that is never dereferenced
SHAPES = [(1, 1, 1), (2, 3, 3), (1, 16, 32), (1, 19, 27), (3, 37, 41)]
# the model options of train_animating_scripts/train_alpha_finetuneBG_finetuneFluid_v1.sh, as the script passes them
V1_OPTION_LINE = ("--use_inverse_depth --accumulation 'wsum' --bg_refine_model_type 'resnet_256W8UpDown64BG_nonorm' "
                  "--alpha_refine_model_type 'resnet_256W8UpDown64Layers_de_resnet_pconv2_nonorm' "
                  "--model_type 'softmax_splating_2layers_alpha_seperate' --refine_model_type 'resnet_256W8UpDown64_de_resnet_pconv2_nonorm' "
                  "--pconv \"pconv_pbn_woresbias\" --out_channel 65 --ngf 64 --norm_G 'sync:spectral_batch' --normalize_image --lr 0.0001 "
                  "--train_Z --lr_g 0.00025 --lr_d 0.001 --W 256 --ATVloss 0.3 --AKLloss 0.0 --ADCloss 1.0 --FluidRegionloss 3 "
                  "--balanced_weight 10 --RockRegionloss 30 --RockRegionlossDecay 20 --train_bg --train_alpha --MVloss 1.0 --niter 2 "
                  "--niter_decay 20 --RockRegionlosstarget 0.25 --use_alpha0_as_blending_weight")


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def test_entry_points_are_declared_and_abi_is_25(L):
    import slr_sfs_amd
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.ABI_VERSION >= 25 and L.slr_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["slr_blend_alpha0_forward"][1]) == 12 and len(_lib.SIGNATURES["slr_blend_alpha0_backward"][1]) == 11
    assert slr_sfs_amd.blend_alpha0 is slr_sfs_amd.layers.blend_alpha0
    assert slr_sfs_amd.TwoLayerAlpha0TrainingModel is slr_sfs_amd.layers.TwoLayerAlpha0TrainingModel
    assert issubclass(slr_sfs_amd.TwoLayerAlpha0TrainingModel, slr_sfs_amd.TwoLayerTrainingModel)


def test_workspace_bytes(L):
    for N, H, W in SHAPES + [(2, 256, 256), (16, 256, 256)]:
        blocks = -(-N * H * W // 512)                                       # a workgroup's share: 128 threads of 4 pixels
        assert L.slr_blend_alpha0_ws_bytes(N, H, W) == -(-blocks * 2 * 8 // 256) * 256
    for N, H, W in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1 << 20, 1 << 10, 1 << 10)]:
        assert L.slr_blend_alpha0_ws_bytes(N, H, W) == 0


def test_entry_points_refuse_before_launching(L):
    """Argument errors return before anything is launched: no device is needed to see them."""
    p = [ctypes.c_void_p(P + 4096 * k) for k in range(8)]
    refused = lambda rc, code, *words: rc == code and all(w in L.slr_last_error() for w in words)      # noqa: E731
    fw, bw = L.slr_blend_alpha0_forward, L.slr_blend_alpha0_backward
    need = L.slr_blend_alpha0_ws_bytes(2, 5, 7)
    for k in range(5):
        args = [None if j == k else p[j] for j in range(5)]
        assert refused(fw(*args, 0.25, 2, 5, 7, p[5], need, None), -1, b"slr_blend_alpha0_forward", b"null")
    for shape in [(0, 5, 7), (2, 0, 7), (2, 5, 0), (1 << 20, 1 << 10, 1 << 10)]:
        assert refused(fw(*p[:5], 0.25, *shape, p[5], need, None), -1, b"sizes")
        assert refused(bw(*p[:6], 0.25, *shape, None), -1, b"sizes")
    assert refused(fw(*p[:5], 0.25, 2, 5, 7, None, need, None), -2, b"workspace")
    assert refused(fw(*p[:5], 0.25, 2, 5, 7, p[5], need - 1, None), -2, b"workspace")
    assert refused(fw(*p[:5], 0.25, 2, 5, 7, ctypes.c_void_p(P + 4), need, None), -2, b"workspace")
    assert refused(bw(None, *p[1:6], 0.25, 2, 5, 7, None), -1, b"slr_blend_alpha0_backward", b"null")
    assert refused(bw(*p[:5], None, 0.25, 2, 5, 7, None), -1, b"null")
    assert refused(bw(*p[:3], None, None, p[5], 0.25, 2, 5, 7, None), -1, b"no gradient")


def test_operator_checks_its_arguments_before_the_device():
    from slr_sfs_amd import layers
    x = list(V.alpha0_inputs(2, 5, 7, dtype=torch.float32))
    for k in range(3):
        with pytest.raises(TypeError, match="tensors required"):
            layers.blend_alpha0(*[None if j == k else t for j, t in enumerate(x)])
    with pytest.raises(NotImplementedError, match="no CPU path"):           # CPU tensors: there is no fallback
        layers.blend_alpha0(*x)
    import unittest.mock as mock
    meta = lambda t: torch.empty_like(t, device="meta")                     # noqa: E731
    with mock.patch.object(torch.Tensor, "is_cuda", property(lambda self: True)), \
            mock.patch.object(layers._lib, "lib", side_effect=AssertionError("the library was called")), \
            mock.patch.object(layers._lib, "call", side_effect=AssertionError("the library was called")):
        with pytest.raises(TypeError, match="float32"):
            layers.blend_alpha0(meta(x[0]), meta(x[1]).double(), meta(x[2]))
        with pytest.raises(ValueError, match="mask_rock"):
            layers.blend_alpha0(meta(x[0]), meta(x[0]), meta(x[2]))
        with pytest.raises(ValueError, match="a_start"):
            layers.blend_alpha0(meta(x[0])[:, :1], meta(x[1]), meta(x[2]))
        with pytest.raises(ValueError, match="a_start"):
            layers.blend_alpha0(meta(x[0])[0], meta(x[1]), meta(x[2]))
        with pytest.raises(ValueError, match="small_motion_alpha"):
            layers.blend_alpha0(meta(x[0]), meta(x[1]), meta(x[2])[:, :, :4])
        with pytest.raises(ValueError, match="not contiguous"):
            layers.blend_alpha0(torch.empty(2, 2, 7, 5, device="meta").transpose(2, 3), meta(x[1]), meta(x[2]))


def _same(got, ref, tol=1e-12):
    err = float((got - ref).abs().max())
    assert err <= tol * float(ref.abs().max()), (err, float(ref.abs().max()))     # relative to the tensor's largest element


@pytest.mark.parametrize("present", [("c0", "values"), ("c0",), ("values",)], ids=["both", "c0-only", "losses-only"])
@pytest.mark.parametrize("rock,sma", [("mixed", "mixed"), ("all", "mixed"), ("none", "mixed"), ("mixed", "all")])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_formula_is_autograd_of_the_definition(shape, rock, sma, present):
    a, r, s = V.alpha0_inputs(*shape, seed=sum(shape), rock=rock, sma=sma, clamp=True)
    a = a.requires_grad_(True)
    c0, losses = V.blend_alpha0(a, r, s, 0.3)
    gen = torch.Generator().manual_seed(5)
    g_c0 = torch.randn(c0.shape, generator=gen, dtype=torch.float64) if "c0" in present else None
    g_vals = torch.tensor([0.7, -1.3], dtype=torch.float64) if "values" in present else None
    total = (c0 * g_c0).sum() if g_c0 is not None else 0.0
    if g_vals is not None:
        total = total + losses["FluidRegionLoss"] * g_vals[0] + losses["RockRegionLoss"] * g_vals[1]
    ref, = torch.autograd.grad(total, a)
    got = V.blend_alpha0_backward(a.detach(), r, s, g_c0, g_vals, 0.3)
    _same(got, ref)
    # where the clamp bites the value is sigmoid(a1) / 1e-8, and nothing flows through the sum: a0 receives nothing
    sig = torch.sigmoid(a.detach()[0, :, 0, 0])
    assert float(sig.sum()) < 1e-8 and float(c0.detach()[0, 0, 0, 0]) == float(sig[1] / 1e-8)
    assert float(got[0, 0, 0, 0]) == 0.0
    if sma == "all" and g_c0 is None:                                        # no moving pixel: both losses and their gradient are exactly 0
        assert all(float(v.detach()) == 0.0 for v in losses.values()) and float(got.abs().max()) == 0.0


def test_region_losses_are_the_references_lines():
    a, r, s = V.alpha0_inputs(2, 5, 7, seed=3)
    c0, losses = V.blend_alpha0(a, r, s, 0.25)
    m = 1.0 - s
    assert float(losses["FluidRegionLoss"]) == float(D.smooth_l1(c0 * (1 - r) * m, (1 - r) * m).mean())
    assert float(losses["RockRegionLoss"]) == float(D.smooth_l1(c0 * r * m, 0.25 * r * m).mean())
    assert torch.equal(c0, D.alpha_losses(a, r, s, r, r, r)[2])              # the c0 that alpha_losses shows


# ---------------------------------------------------------------------------------------------- the model against the reference's run

@functools.lru_cache(maxsize=None)
def _fixture():
    return V.load()


@functools.lru_cache(maxsize=None)
def _definition(dtype, mutant=None):
    return V.forward(_fixture(), dtype, mutant=mutant)


def _E(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def test_definition_is_the_references_run():
    """tests/two_layer_v1_f64.py in float64 against the reference's own float32 run: every loss entry and every pred_dict entry inside
    10 E(def32) + 1e-6, E(def32) the same definition in float32 against float64 (tests/test_two_layer_host.py's rule)."""
    g = _fixture()
    (l64, p64, _), (l32, p32, _) = _definition(torch.float64), _definition(torch.float32)
    assert sorted(l64) == sorted(g["loss_keys"]) and list(p64) == g["pred_keys"]
    assert "FluidRegionLoss" in l64 and "RockRegionLoss" in l64 and "AlphaMSEloss" not in l64
    tail = [k for k in g["loss_keys"] if k in ("L1_bg", "Perceptual_bg") + V.REGION_LOSS_NAMES + D.LOSS_NAMES]
    assert tail[-4:] == list(V.REGION_LOSS_NAMES + D.LOSS_NAMES[2:]) and set(tail[1:3]) == {"L1_bg", "Perceptual_bg"}
    for kind, ref64, ref32 in (("loss", l64, l32), ("pred", p64, p32)):
        for k in ref64:
            e_ref, e_32 = _E(torch.from_numpy(g[f"{kind}/{k}"]), ref64[k]), _E(ref32[k], ref64[k])
            print(f"{kind} {k}: E(reference) {e_ref:.3e}  E(def32) {e_32:.3e}")
            assert e_ref <= 10 * e_32 + 1e-6, (k, e_ref, e_32)
            assert e_32 <= 0.03, (k, e_32)


def test_changed_buffers_after_the_forward_are_the_references():
    """u and v after the forward against the reference's run.  They depend on the weights alone, so they are the v2 run's; what the v1
    run changes among the buffers is the batch statistics of the alpha decoder, whose input's last plane is another one (the device test
    holds the model to those)."""
    import train_step_f64 as T64
    g, v2 = _fixture(), D.load()
    nets = _definition(torch.float64)[2]
    n = 0
    for net, (blocks, plain, _, _) in D.NETWORKS.items():
        names = T64.ENC_NAMES if plain else T64.DEC_NAMES
        for i, uv in enumerate(nets[net]["uvs"]):
            for name, (u, v) in uv.items():
                for t, tail in ((u, "weight_u"), (v, "weight_v")):
                    key = f"{net}.{blocks}.{i}.{names[name]}.{tail}"
                    ref = torch.from_numpy(g.get("after/" + key, g["sd/" + key])).double()
                    assert float((t - ref).abs().max()) <= 1e-5, (net, i, name, tail)
                    n += 1
    assert n > 100
    after = sorted(k for k in g if k.startswith("after/"))
    assert after == sorted(k for k in v2 if k.startswith("after/")) and len(after) > 600
    differs = [k for k in after if not np.array_equal(g[k], v2[k])]
    assert len(differs) == 32 and all(k.startswith("after/net_alpha_decoder.") and "stored_" in k for k in differs)


@pytest.mark.parametrize("mutant", ["end_c0", "feature_norm"])
def test_the_fixture_tells_v1_from_its_near_misses(mutant):
    """The end direction weighted by the END image's c0, and the alpha plane divided by the features' normaliser, both in float64, fall
    OUTSIDE the bound the definition is held to, on PredImg and on the consistency loss at least."""
    g = _fixture()
    (l64, p64, _), (l32, p32, _) = _definition(torch.float64), _definition(torch.float32)
    lm, pm, _ = _definition(torch.float64, mutant)
    for kind, k, mut, r64, r32 in (("pred", "PredImg", pm, p64, p32), ("loss", D.LOSS_NAMES[2], lm, l64, l32)):
        e_mut, bnd = _E(torch.from_numpy(g[f"{kind}/{k}"]), mut[k]), 10 * _E(r32[k], r64[k]) + 1e-6
        print(f"{mutant}: {k} E(reference against the mutant) {e_mut:.3e}  bound {bnd:.3e}")
        assert e_mut > bnd, (mutant, k, e_mut, bnd)


def test_fixture_is_data_only_and_small():
    z = np.load(V.GOLDEN, allow_pickle=False)
    assert os.path.getsize(V.GOLDEN) < 1 << 20
    assert all(z[k].dtype.kind in "fiubU" for k in z.files)
    assert "--use_alpha0_as_blending_weight" in str(z["options"]) and "--MRADCloss 1.0" in str(z["options"])


# ---------------------------------------------------------------------------------------------- options

def _parse(line):
    """An option line the way argparse reads it into a Namespace: ``--name value`` (numbers as numbers) and ``--flag`` (True)."""
    out, tokens, i = argparse.Namespace(), line.split(), 0
    while i < len(tokens):
        name = tokens[i][2:]
        assert tokens[i].startswith("--"), tokens[i]
        if i + 1 < len(tokens) and not tokens[i + 1].startswith("--"):
            v = tokens[i + 1].strip("'\"")
            try:
                v = float(v) if any(c in v for c in ".e") else int(v)
            except ValueError:
                pass
            setattr(out, name, v)
            i += 2
        else:
            setattr(out, name, True)
            i += 1
    return out


def test_the_v1_scripts_option_line_is_accepted_and_the_v2_check_refuses_it():
    from slr_sfs_amd import layers
    opts = _parse(V1_OPTION_LINE)
    assert opts.use_alpha0_as_blending_weight is True and opts.FluidRegionloss == 3 and opts.RockRegionloss == 30
    assert opts.RockRegionlosstarget == 0.25 and opts.ngf == 64 and not hasattr(opts, "AlphaMSEloss")
    layers.check_two_layer_alpha0_options(opts)
    layers.check_two_layer_alpha0_options(V.options())
    with pytest.raises(NotImplementedError, match="use_alpha0_as_blending_weight.*TwoLayerAlpha0TrainingModel"):
        layers.check_two_layer_options(opts)


def test_every_refused_flag_raises_naming_itself():
    import slr_sfs_amd as S
    from slr_sfs_amd import layers
    allowed = ("use_alpha0_as_blending_weight", "RockRegionloss", "FluidRegionloss")
    flags = tuple(n for n in layers._REFUSED_FLAGS if n not in allowed) + ("use_softmax_splatter_v2", "use_3d_splatter", "random_ff_mask",
                                                                           "train_motion", "use_rgb_features")
    assert len(flags) == len(layers._REFUSED_FLAGS) - 1 + 5
    for name in flags + ("use_alpha_tau", "use_fluid_alpha_only", "use_bg_alpha_only", "use_reweight_mask_loss2", "use_static_moving_loss"):
        with pytest.raises(NotImplementedError, match=name):
            layers.check_two_layer_alpha0_options(V.options(**{name: True}))
    for name in layers._REFUSED_POSITIVE:
        if name in allowed:
            layers.check_two_layer_alpha0_options(V.options(**{name: 0.5}))
        else:
            with pytest.raises(NotImplementedError, match=name):
                layers.check_two_layer_alpha0_options(V.options(**{name: 0.5}))
        layers.check_two_layer_alpha0_options(V.options(**{name: 0.0}))
    for name in ("AlphaL1loss", "clamp_alpha", "use_alpha_softmax"):
        assert name in layers._REFUSED_POSITIVE
    for value in ("resnet_256W8UpDown64Layers_decouple_de_resnet_pconv2_nonorm", "resnet_256W8UpDown64Layers_image_de_resnet_pconv2_nonorm"):
        with pytest.raises(NotImplementedError, match="alpha_refine_model_type"):
            layers.check_two_layer_alpha0_options(V.options(alpha_refine_model_type=value))
    for name in ("train_bg", "train_alpha"):
        with pytest.raises(NotImplementedError, match=name):
            layers.check_two_layer_alpha0_options(V.options(**{name: False}))
    with pytest.raises(NotImplementedError, match="TwoLayerAlpha0TrainingModel.*use_alpha_tau"):
        S.TwoLayerAlpha0TrainingModel(V.options(use_alpha_tau=True))
    # without the flag the new class refuses and points to the parent; the parent keeps refusing the flag and both weights
    for opts in (D.options(), V.options(use_alpha0_as_blending_weight=False)):
        with pytest.raises(NotImplementedError, match="use_alpha0_as_blending_weight.*TwoLayerTrainingModel"):
            S.TwoLayerAlpha0TrainingModel(opts)
    for name, value in (("use_alpha0_as_blending_weight", True), ("FluidRegionloss", 3.0), ("RockRegionloss", 30.0)):
        with pytest.raises(NotImplementedError, match=name):
            S.TwoLayerTrainingModel(D.options(**{name: value}))


def test_model_keys_shapes_and_parameter_order_are_the_parents():
    import slr_sfs_amd as S
    g = _fixture()
    with torch.device("meta"):
        model = S.TwoLayerAlpha0TrainingModel(V.options(), S.VGG19Features(), **D.model_kwargs())
        parent = S.TwoLayerTrainingModel(D.options(), S.VGG19Features(), **D.model_kwargs())
    sd, theirs = model.reference_state_dict("model."), parent.reference_state_dict("model.")
    assert list(sd) == list(theirs) and all(sd[k].shape == theirs[k].shape for k in sd) and len(sd) > 1000
    assert [k for k, _, _ in model.reference_parameters()] == g["parameter_order"]
    assert model.literal_encoder_calls is True and type(model).forward is S.TwoLayerTrainingModel.forward
