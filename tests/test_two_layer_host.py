"""Host-side checks of the two-layer model (slr_sfs_amd.layers, csrc/layers.hip, ABI 24), none of which needs a GPU: the entry points and
their refusals, the operators' argument checks, and the analytic backward the kernels compute (tests/two_layer_f64.py) against float64
autograd of the definition -- on inputs where the 1e-8 clamp bites, on constant runs, with absent output gradients, in both reweight
forms, and with a NaN in one input pixel (the same elements NaN, the others equal).  Then the model: the written-out forward in float64
against the reference's own run (tests/golden/two_layer_train_vs_reference.npz), u and v after the forward with the literal encoder
calls, the key set, shapes and parameter order of a ``TwoLayerTrainingModel`` built on the meta device, and every refused flag."""
import ctypes
import os
import re

import pytest
import torch

import two_layer_f64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("slr_layer_composite_forward", "slr_layer_composite_backward", "slr_alpha_losses_ws_bytes", "slr_alpha_losses_forward",
           "slr_alpha_losses_backward")
P = 0x7F0000100000                                                           # a 16-byte aligned address that is never dereferenced
SHAPES = [(2, 5, 7), (1, 33, 31), (3, 2, 2), (2, 6, 8)]


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def test_entry_points_are_declared_and_abi_is_24(L):
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.ABI_VERSION >= 24 and L.slr_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION
    import slr_sfs_amd
    assert slr_sfs_amd.layer_composite is slr_sfs_amd.layers.layer_composite
    assert slr_sfs_amd.alpha_losses is slr_sfs_amd.layers.alpha_losses


def test_workspace_bytes(L):
    for N, H, W in SHAPES + [(2, 256, 256), (16, 256, 256)]:
        blocks = -(-N * H * W // 512)                                       # a workgroup's share: 128 threads of 4 pixels
        assert L.slr_alpha_losses_ws_bytes(N, H, W) == -(-blocks * 11 * 8 // 256) * 256
    for N, H, W in [(0, 4, 4), (1, 1, 4), (1, 4, 1), (-1, 4, 4), (1 << 20, 1 << 10, 1 << 10)]:
        assert L.slr_alpha_losses_ws_bytes(N, H, W) == 0


def test_entry_points_refuse_before_launching(L):
    """Argument errors return before anything is launched: no device is needed to see them."""
    p = [ctypes.c_void_p(P + 4096 * k) for k in range(12)]
    refused = lambda rc, code, *words: rc == code and all(w in L.slr_last_error() for w in words)      # noqa: E731
    cf, cb, af, ab = (getattr(L, n) for n in (ENTRIES[0], ENTRIES[1], ENTRIES[3], ENTRIES[4]))
    assert refused(cf(*p[:7], None, 1, 4, 4, None), -1, b"slr_layer_composite_forward", b"null")
    assert refused(cf(None, *p[:7], 1, 4, 4, None), -1, b"null")
    for shape in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1 << 20, 1 << 10, 1 << 10)]:
        assert refused(cf(*p[:8], *shape, None), -1, b"sizes")
        assert refused(cb(*p[:11], *shape, None), -1, b"sizes")
    assert refused(cb(None, *p[:10], 1, 4, 4, None), -1, b"null")
    assert refused(cb(*p[:7], None, None, None, None, 1, 4, 4, None), -1, b"no gradient")
    need = L.slr_alpha_losses_ws_bytes(2, 5, 7)
    assert refused(af(*p[:8], None, 1, 2, 5, 7, p[9], need, None), -1, b"slr_alpha_losses_forward", b"null")
    for shape in [(2, 1, 7), (2, 5, 1), (0, 5, 7)]:
        assert refused(af(*p[:9], 1, *shape, p[9], need, None), -1, b"sizes")
        assert refused(ab(*p[:10], 1, *shape, None), -1, b"sizes")
    assert refused(af(*p[:9], 1, 2, 5, 7, None, need, None), -2, b"workspace")
    assert refused(af(*p[:9], 1, 2, 5, 7, p[9], need - 1, None), -2, b"workspace")
    assert refused(af(*p[:9], 1, 2, 5, 7, ctypes.c_void_p(P + 4), need, None), -2, b"workspace")
    assert refused(ab(*p[:7], None, p[8], p[9], 1, 2, 5, 7, None), -1, b"null")
    assert refused(ab(*p[:8], None, None, 1, 2, 5, 7, None), -1, b"no gradient")


def test_operators_check_their_arguments_before_the_device():
    from slr_sfs_amd import layers
    d = D.head_inputs(2, 5, 7, dtype=torch.float32)
    comp = [d[k] for k in D.COMPOSITE_ARGS]
    alph = [d[k] for k in D.ALPHA_ARGS]
    for k in range(4):
        with pytest.raises(TypeError, match="tensors required"):
            layers.layer_composite(*[None if j == k else t for j, t in enumerate(comp)])
    for k in range(6):
        with pytest.raises(TypeError, match="tensors required"):
            layers.alpha_losses(*[1.0 if j == k else t for j, t in enumerate(alph)])
    with pytest.raises(NotImplementedError, match="no CPU path"):           # CPU tensors: there is no fallback
        layers.layer_composite(*comp)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        layers.alpha_losses(*alph)
    # the checks behind the device check, on tensors that claim a device but own no memory
    meta = lambda t: torch.empty_like(t, device="meta")                     # noqa: E731
    planes = lambda ts, names, cs: tuple((n, meta(t), c) for n, t, c in zip(names, ts, cs))             # noqa: E731
    import unittest.mock as mock
    with mock.patch.object(torch.Tensor, "is_cuda", property(lambda self: True)):
        ok = planes(alph, D.ALPHA_ARGS, (2, 1, 1, 1, 1, 1))
        assert layers._check_planes("alpha_losses", ok, 2) == (2, 5, 7)
        with pytest.raises(TypeError, match="float32"):
            layers._check_planes("alpha_losses", ok[:1] + (("mask_rock", meta(alph[1]).double(), 1),) + ok[2:], 2)
        with pytest.raises(ValueError, match="mask_rock"):
            layers._check_planes("alpha_losses", ok[:1] + (("mask_rock", meta(alph[0]), 1),) + ok[2:], 2)
        with pytest.raises(ValueError, match="a_start"):
            layers._check_planes("alpha_losses", (("a_start", meta(alph[0])[0], 2),) + ok[1:], 2)
        for H, W in [(1, 7), (5, 1)]:
            tiny = tuple((n, torch.empty(2, c, H, W, device="meta"), c) for n, _, c in ok)
            with pytest.raises(ValueError, match="H, W >= 2"):
                layers._check_planes("alpha_losses", tiny, 2)
        with pytest.raises(ValueError, match="not contiguous"):
            layers._check_planes("alpha_losses", (("a_start", torch.empty(2, 2, 7, 5, device="meta").transpose(2, 3), 2),) + ok[1:], 2)


def _leaves(d, names):
    return [d[k].clone().requires_grad_(k in ("fluid_raw", "bg_raw", "fluid_alpha_raw", "bg_alpha_raw", "a_start")) for k in names]


def _same(got, ref, tol=1e-10):
    """Equal to tol where ref is a number, NaN exactly where ref is NaN."""
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), (int(torch.isnan(got).sum()), int(nan.sum()))
    if (~nan).any():
        err = float((got[~nan] - ref[~nan]).abs().max())
        assert err <= tol * max(1.0, float(ref[~nan].abs().max())), err


@pytest.mark.parametrize("absent", [(), ("fluid", "bg"), ("pred", "fluid"), ("bg",)])
@pytest.mark.parametrize("shape", SHAPES)
def test_composite_backward_formula_is_autograd_of_the_definition(shape, absent):
    d = D.head_inputs(*shape, seed=3)
    x = _leaves(d, D.COMPOSITE_ARGS)
    pred, fluid, bg, ca = D.layer_composite(*x)
    g = torch.Generator().manual_seed(5)
    grads = {k: None if k in absent else torch.randn(t.shape, generator=g, dtype=torch.float64)
             for k, t in (("pred", pred), ("fluid", fluid), ("bg", bg))}
    total = sum((t * grads[k]).sum() for k, t in (("pred", pred), ("fluid", fluid), ("bg", bg)) if grads[k] is not None)
    ref = torch.autograd.grad(total, x, allow_unused=True)
    got = D.layer_composite_backward(*[t.detach() for t in x], grads["pred"], grads["fluid"], grads["bg"])
    for r, o in zip(ref, got):
        _same(o, torch.zeros_like(o) if r is None else r)
    # where the clamp bites the value is (af F + ab B) / 1e-8 and nothing flows through n
    af, ab = torch.sigmoid(x[2].detach()[0, 0, 0, 0]), torch.sigmoid(x[3].detach()[0, 0, 0, 0])
    assert float(af + ab) < 1e-8 and float(ca.detach()[0, 0, 0, 0]) == float(af / 1e-8)


@pytest.mark.parametrize("rock", ["mixed", "none", "all"])
@pytest.mark.parametrize("reweight", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_alpha_losses_backward_formula_is_autograd_of_the_definition(shape, reweight, rock):
    d = D.head_inputs(*shape, seed=4, rock=rock)
    x = _leaves(d, D.ALPHA_ARGS)
    losses, gt, c0 = D.alpha_losses(*x, reweight=reweight)
    g = torch.tensor([0.7, -1.3, 2.1, 0.4], dtype=torch.float64)
    total = sum(losses[n] * g[k] for k, n in enumerate(D.LOSS_NAMES))
    ra, rf = torch.autograd.grad(total, (x[0], x[5]))
    ga, gf = D.alpha_losses_backward(*[t.detach() for t in x], g, reweight=reweight)
    _same(ga, ra)
    _same(gf, rf)
    if rock != "mixed" and reweight:                                        # one denominator is exactly 1 + 0
        m = 1.0 - d["small_motion_alpha"]
        err = (c0.detach() * m - gt * m) ** 2
        other = (m * err).sum() / (1 + m.sum())
        assert abs(float(losses["AlphaMSEloss"]) - 0.5 * float(other)) < 1e-15


def test_total_variation_takes_the_raw_fluid_logit_and_the_sigmoided_background():
    d = D.head_inputs(2, 5, 7, seed=6)
    losses, _, _ = D.alpha_losses(*[d[k] for k in D.ALPHA_ARGS])
    a = d["a_start"]
    assert float(losses["AlphaTV"]) == float(D.total_variation(a[:, 1:2]) + D.total_variation(torch.sigmoid(a[:, 0:1])))
    assert float(losses["AlphaTV"]) != float(D.total_variation(torch.sigmoid(a[:, 1:2])) + D.total_variation(torch.sigmoid(a[:, 0:1])))


@pytest.mark.parametrize("where", ["fluid_raw", "bg_raw", "fluid_alpha_raw", "bg_alpha_raw"])
def test_composite_backward_formula_on_a_nan_pixel(where):
    d = D.head_inputs(2, 5, 7, seed=7)
    d[where][1, 0, 2, 3] = float("nan")
    x = _leaves(d, D.COMPOSITE_ARGS)
    pred, fluid, bg, _ = D.layer_composite(*x)
    ref = torch.autograd.grad(pred.sum() * 0.5 + (fluid * 0.25).sum() + (bg * 2).sum(), x)
    got = D.layer_composite_backward(*[t.detach() for t in x], torch.full_like(pred, 0.5), torch.full_like(pred, 0.25),
                                     torch.full_like(pred, 2.0))
    for r, o in zip(ref, got):
        _same(o, r)
    assert sum(int(torch.isnan(r).sum()) for r in ref) >= 1


@pytest.mark.parametrize("where,channel", [("a_start", 0), ("a_start", 1), ("fluid_alpha_raw", 0), ("warped_alpha", 0), ("norm", 0)])
def test_alpha_losses_backward_formula_on_a_nan_pixel(where, channel):
    d = D.head_inputs(2, 5, 7, seed=8)
    d[where][1, channel, 2, 3] = float("nan")
    d["small_motion_alpha"][1] = d["small_motion_alpha"][0]                 # (the NaN's sample takes part in the moving region)
    x = _leaves(d, D.ALPHA_ARGS)
    losses, _, _ = D.alpha_losses(*x)
    # the gradients reaching the losses are numbers even where a loss is NaN, as they are in a training step
    g = torch.tensor([0.7, -1.3, 2.1, 0.4], dtype=torch.float64)
    ra, rf = torch.autograd.grad(sum(losses[n] * g[k] for k, n in enumerate(D.LOSS_NAMES)), (x[0], x[5]))
    ga, gf = D.alpha_losses_backward(*[t.detach() for t in x], g)
    _same(ga, ra)
    _same(gf, rf)


# ---------------------------------------------------------------------------------------------- the model against the reference's run

import functools  # noqa: E402

import numpy as np  # noqa: E402


@functools.lru_cache(maxsize=None)
def _fixture():
    return D.load()


@functools.lru_cache(maxsize=None)
def _definition(dtype):
    return D.forward(_fixture(), dtype)


def _E(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def test_definition_is_the_references_run():
    """tests/two_layer_f64.py in float64 against the reference's own float32 run: every loss entry and every pred_dict entry inside
    10 E(def32) + 1e-6, E(def32) the same definition in float32 against float64 (tests/test_train_step_host.py's rule)."""
    g = _fixture()
    (l64, p64, _), (l32, p32, _) = _definition(torch.float64), _definition(torch.float32)
    assert list(l64) != [] and sorted(l64) == sorted(g["loss_keys"]) and list(p64) == g["pred_keys"]
    for kind, ref64, ref32 in (("loss", l64, l32), ("pred", p64, p32)):
        for k in ref64:
            e_ref, e_32 = _E(torch.from_numpy(g[f"{kind}/{k}"]), ref64[k]), _E(ref32[k], ref64[k])
            print(f"{kind} {k}: E(reference) {e_ref:.3e}  E(def32) {e_32:.3e}")
            assert e_ref <= 10 * e_32 + 1e-6, (k, e_ref, e_32)
            assert e_32 <= 0.03, (k, e_32)                                   # the cap of tests/train_step_f64.py


def test_u_and_v_after_the_forward_are_the_references_with_the_literal_calls():
    g = _fixture()
    nets = _definition(torch.float64)[2]
    skipped = D.forward(g, torch.float64, literal_encoder_calls=False)[2]
    n, moved = 0, 0
    for net, (blocks, plain, _, _) in D.NETWORKS.items():
        import train_step_f64 as T64
        names = T64.ENC_NAMES if plain else T64.DEC_NAMES
        for i, uv in enumerate(nets[net]["uvs"]):
            for name, (u, v) in uv.items():
                for t, tail, other in ((u, "weight_u", skipped[net]["uvs"][i][name][0]), (v, "weight_v", skipped[net]["uvs"][i][name][1])):
                    key = f"{net}.{blocks}.{i}.{names[name]}.{tail}"          # (the fixture records the buffers that changed; the others stand as they were)
                    ref = torch.from_numpy(g.get("after/" + key, g["sd/" + key])).double()
                    assert float((t - ref).abs().max()) <= 1e-5, (net, i, name, tail)
                    if net == "encoder":
                        moved += float((other - ref).abs().max()) > 1e-4
                    n += 1
    assert n > 100 and moved > 10                                            # without the dropped pair the encoder's u / v are other vectors


@functools.lru_cache(maxsize=None)
def _meta_model():
    import slr_sfs_amd as S
    with torch.device("meta"):
        return S.TwoLayerTrainingModel(D.options(), S.VGG19Features(), **D.model_kwargs())


def test_model_keys_shapes_and_parameter_order_are_the_references():
    g = _fixture()
    model = _meta_model()
    sd = model.reference_state_dict("model.")                              # (BaseModel on the host: no DataParallel, so no "module.")
    theirs = {k: shape for k, shape in zip(g["state_keys"], g["state_shapes"]) if k.startswith("model.")}
    assert sorted(sd) == sorted(theirs) and len(sd) > 1000
    for k, shape in theirs.items():
        assert tuple(sd[k].shape) == tuple(int(s) for s in shape if s >= 0), k
    rows = model.reference_parameters()
    assert [k for k, _, _ in rows] == g["parameter_order"]
    learns = {k: l for k, _, l in rows}
    for k, l in zip(g["parameter_order"], g["parameter_learns"]):
        if not k.endswith("conv_b.weight_orig"):                            # (the decoders' unused conv_b never gets a gradient there)
            assert learns[k] == bool(l), k
    listed = {id(t) for _, t, l in rows if l}
    assert not [n for n, p in model.named_parameters() if p.requires_grad and id(p) not in listed]      # what Trainer.optimizers asks


def test_every_refused_flag_raises_naming_itself():
    import slr_sfs_amd as S
    from slr_sfs_amd import layers
    flags = layers._REFUSED_FLAGS + ("use_softmax_splatter_v2", "use_3d_splatter", "random_ff_mask", "train_motion", "use_rgb_features")
    assert "use_alpha0_as_blending_weight" in flags
    for name in flags:
        with pytest.raises(NotImplementedError, match=name):
            layers.check_two_layer_options(D.options(**{name: True}))
    for name in layers._REFUSED_POSITIVE:
        with pytest.raises(NotImplementedError, match=name):
            layers.check_two_layer_options(D.options(**{name: 0.5}))
        layers.check_two_layer_options(D.options(**{name: 0.0}))
    for value in ("resnet_256W8UpDown64Layers_decouple_de_resnet_pconv2_nonorm", "resnet_256W8UpDown64Layers_image_de_resnet_pconv2_nonorm"):
        with pytest.raises(NotImplementedError, match="alpha_refine_model_type"):
            layers.check_two_layer_options(D.options(alpha_refine_model_type=value))
    for name in ("train_bg", "train_alpha"):
        with pytest.raises(NotImplementedError, match=name):
            layers.check_two_layer_options(D.options(**{name: False}))
    with pytest.raises(NotImplementedError, match="use_alpha0_as_blending_weight"):
        S.TwoLayerTrainingModel(D.options(use_alpha0_as_blending_weight=True))
    layers.check_two_layer_options(D.options())


def test_fixture_is_data_only_and_small():
    z = np.load(D.GOLDEN, allow_pickle=False)
    assert os.path.getsize(D.GOLDEN) < 1 << 20
    assert all(z[k].dtype.kind in "fiubU" for k in z.files)
