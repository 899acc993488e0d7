"""Host checks of the motion-training operators (slr_sfs_amd.motion_training, ABI 23): the written-out definitions of
tests/motion_train_f64.py against torch autograd in float64, the ABI number in header, binding and library, the argument checks that run
before a device is touched, and the NON-VACUITY of the device tests' criterion: each deliberately wrong variant of the definitions
(motion_train_f64.WRONG) lies outside E <= 10 * E_plain32 + 1e-6 at the device tests' own inputs (tests/test_gpu_motion_train.py), by
the printed factor (run with -s)."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import motion_train_f64 as M64
import motion_train_fixture as TF
import test_gpu_motion_train as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def close(name, got, want):
    err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
    print(f"{name}: {err:.2e}")
    assert err <= TOL, (name, err)


# ------------------------------------------------------------------ the definitions are torch's

@pytest.mark.parametrize("shape", G.CONV_SHAPES[:5], ids=G._id)
def test_convolution_definition_is_torch_autograd(shape):
    c = G._conv_case(shape)
    for slope in (None, G.SLOPE):
        x, w, b = (c[k].double().requires_grad_() for k in ("x", "w", "b"))
        out = F.conv2d(x if slope is None else F.leaky_relu(x, slope), w, b, stride=2, padding=1)
        out.backward(c["g"].double())
        close("out", M64.conv_forward(x.detach(), w.detach(), b.detach(), slope), out.detach())
        close("dx", M64.conv_backward_data(c["g"].double(), w.detach(), x.detach(), slope), x.grad)
        dw, db = M64.conv_weight_grad(x.detach(), c["g"].double(), slope)
        close("dw", dw, w.grad)
        close("db", db, b.grad)


def test_spectral_weight_gradient_definition_is_torch_autograd():
    c = G._conv_case((2, 33, 31, 8, 8))
    w, u, v = c["w"].double().requires_grad_(), c["u"].double(), c["v"].double()
    sigma = u @ w.reshape(w.shape[0], -1) @ v
    out = F.conv2d(c["x"].double(), w / sigma, None, stride=2, padding=1)
    out.backward(c["g"].double())
    dw, _ = M64.conv_weight_grad(c["x"].double(), c["g"].double(), None)
    close("d weight_orig", M64.sn_weight_grad(dw, w.detach(), u, v, 1.0 / sigma.detach()), w.grad)


@pytest.mark.parametrize("shape", G.NORM_SHAPES[:5], ids=G._id)
def test_instnorm_spade_definition_is_torch_autograd(shape):
    c = G._norm_case(shape)
    x, gb = c["x"].double().requires_grad_(), c["gb"].double().requires_grad_()
    C = x.shape[1]
    out = F.instance_norm(x, eps=M64.EPS) * (1 + gb[:, :C]) + gb[:, C:]
    out.backward(c["g"].double())
    close("out", c["r64"]["out"], out.detach())
    close("gx", c["r64"]["gx"], x.grad)
    close("dgb", c["r64"]["dgb"], gb.grad)


def _torch_up(a, b, q, relu):
    def up(x):
        if relu == M64.RELU_BEFORE:
            x = F.relu(x)
        if q < 0:
            return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        parts = [(x[:, :q], "bilinear"), (x[:, q:q + 1], "nearest"), (x[:, q + 1:], "bilinear")]
        return torch.cat([F.interpolate(t, scale_factor=2, mode=m, **({"align_corners": False} if m == "bilinear" else {}))
                          for t, m in parts if t.shape[1]], 1)
    y = up(a) if b is None else torch.cat([up(a), up(b)], 1)
    return F.relu(y) if relu == M64.RELU_AFTER else y


@pytest.mark.parametrize("size", G.UP_SIZES[:5], ids=G._id)
def test_upsample_concat_definition_is_torch_autograd(size):
    for channels in G.UP_CHANNELS:
        for relu in (M64.RELU_NONE, M64.RELU_BEFORE, M64.RELU_AFTER):
            c = G._up_case(size, channels, relu)
            a = c["a"].double().requires_grad_()
            b = None if c["b"] is None else c["b"].double().requires_grad_()
            out = _torch_up(a, b, channels[2], relu)
            out.backward(c["g"].double())
            assert torch.equal(c["r64"]["out"], out.detach())
            close("ga", c["r64"]["ga"], a.grad)
            if b is not None:
                close("gb", c["r64"]["gb"], b.grad)


@pytest.mark.parametrize("shape", G.LOSS_SHAPES[1:2], ids=G._id)
def test_motion_losses_definition_is_the_reference_expression(shape):
    """torch.norm(pred - gt, 2, 1).mean(), nn.L1Loss, (pred - gt).pow(2).sum(1).view(bs, -1).mean(1) and their autograd gradient."""
    c = G._loss_case(shape)
    pred, gt = c["pred"].double().requires_grad_(), c["gt"].double()
    epe, l1 = torch.norm(pred - gt, 2, 1).mean(), torch.nn.L1Loss()(pred, gt)
    mse = (pred - gt).pow(2).sum(dim=1).view(shape[0], -1).mean(dim=1)
    (10.0 * epe + 3.0 * l1).backward()
    close("epe", c["r64"]["epe"], epe.detach())
    close("l1", c["r64"]["l1"], l1.detach())
    close("mse", c["r64"]["mse"], mse.detach())
    close("grad", c["r64"]["g_both"], pred.grad)
    assert float(pred.grad[(pred - gt).detach() == 0].abs().max()) == 0.0


# ------------------------------------------------------------------ the whole definition is the reference

@pytest.fixture(scope="module")
def golden(golden_dir):
    import numpy as np
    return np.load(os.path.join(golden_dir, "motion_train_vs_reference.npz"))


def test_whole_definition_in_float64_is_the_reference(golden):
    """Every loss entry, PredMotion, every parameter gradient and u / v after the forward of the reference's own SPADEUnetMaskMotion
    (train() mode, float64, N = 2, 256 x 256, num_filters = 8) within 1e-10."""
    g = golden
    losses, pred, grads, after = TF.definition("float64", True)
    assert [str(k) for k in g["loss_keys"]] == ["EndPointError", "Total Loss", "PSNR_motion"] and float(g["div_flow"]) == TF.DIV_FLOW
    for k in g["loss_keys"]:
        close(f"loss {k}", losses[str(k)].reshape(1), torch.tensor([float(g["loss/" + str(k)])], dtype=torch.float64))
    assert float(pred["MovingMask"].sum()) == float(g["MovingMask#sum"])

    def digest(name, t, scale=None):
        flat = t.double().reshape(-1)
        scale = float(g[name + "#max_abs"]) if scale is None else scale
        err = float((flat[TF.positions(name, flat.numel())] - torch.from_numpy(g[name + "#samples"])).abs().max()) / scale
        assert err <= TOL and (name[5:] in TF.ZERO_GRAD_BIASES or abs(float(flat.abs().max()) - scale) <= TOL * scale), (name, err)
        return err
    print("PredMotion", digest("PredMotion", pred["PredMotion"]))
    names = sorted(k[5:-8] for k in g.files if k.startswith("grad/") and k.endswith("#samples"))
    assert names == sorted(grads) and len(names) == 110
    print("gradients", max(digest("grad/" + k, grads[k], TF.grad_scale(grads, k) if k in TF.ZERO_GRAD_BIASES else None) for k in names))
    for k in TF.ZERO_GRAD_BIASES:                                           # exactly zero but for rounding, in the reference too
        assert float(g["grad/" + k + "#max_abs"]) <= TOL * TF.grad_scale(grads, k)
    uv = [k[6:] for k in g.files if k.startswith("after/")]
    assert len(uv) == 32
    for k in uv:
        close("after " + k, after[k], torch.from_numpy(g["after/" + k]))
        assert not torch.equal(after[k], TF.initial_state()[k].double())   # (the power iteration moved it)


def test_key_set_and_shapes_at_32_filters_are_the_reference(golden):
    import slr_sfs_amd as S
    want = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(golden["keys_nf32"], golden["shapes_nf32"])}
    assert want == {k: tuple(s) for k, s in M64.param_shapes(32).items()}
    net = S.TrainableSPADEUnet4MaskMotion(nf=32)
    sd = net.reference_state_dict(TF.PREFIX)
    assert {k[len(TF.PREFIX):]: tuple(v.shape) for k, v in sd.items()} == want and all(k.startswith(TF.PREFIX) for k in sd)
    net.load_reference_state_dict(sd, TF.PREFIX)
    S.nets.load_motion_state_dict(S.nets.SPADEUnet4MaskMotion(nf=32), sd, TF.PREFIX)     # the inference class reads what is written
    # strict in both directions, checked before anything is copied
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for bad in (dict(sd, **{TF.PREFIX + "extra.weight": torch.zeros(1)}), {k: v for k, v in sd.items() if not k.endswith("dconv8.bias")},
                dict(sd, **{TF.PREFIX + "dconv8.bias": torch.zeros(3)})):
        bad = {k: (v + 1.0 if v.dtype.is_floating_point else v) for k, v in bad.items()}
        with pytest.raises((KeyError, ValueError)):
            net.load_reference_state_dict(bad, TF.PREFIX)
        assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    with pytest.raises(KeyError):
        net.load_reference_state_dict(sd, "other.")


def test_model_options_that_are_not_built_name_the_flag():
    import slr_sfs_amd as S
    ok = dict(use_mask_as_motion_input=True, use_hint_as_motion_input=True, motion_norm_G="sync:spectral_instance", div_flow=1.0, W=256,
              motion_losses=["10.0_EndPointError"])
    S.MotionTrainingModel(types.SimpleNamespace(**ok), nf=8)
    for change, flag in ((dict(use_mask_as_motion_input=False), "use_mask_as_motion_input"),
                         (dict(use_hint_as_motion_input=False), "use_hint_as_motion_input"), (dict(motion_norm_G="sync:spectral_batch"), "motion_norm_G")):
        with pytest.raises(NotImplementedError, match=flag):
            S.MotionTrainingModel(types.SimpleNamespace(**dict(ok, **change)), nf=8)


# ------------------------------------------------------------------ ABI and argument checks

def test_abi_23_in_header_binding_and_library():
    import slr_sfs_amd
    L = slr_sfs_amd._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    assert L.slr_abi_version() == slr_sfs_amd._lib.ABI_VERSION == int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 23
    for name in ("slr_conv4x4s2_backward_data", "slr_conv4x4s2_grad_ws_bytes", "slr_conv4x4s2_weight_grad", "slr_instnorm_spade_train_forward",
                 "slr_instnorm_spade_backward", "slr_upsample2x_concat_backward", "slr_motion_loss_ws_bytes", "slr_motion_loss",
                 "slr_motion_loss_grad"):
        assert name in slr_sfs_amd._lib.SIGNATURES and re.search(rf"\b{name}\(", hdr), name
        getattr(L, name)


def test_entry_points_refuse_bad_arguments_before_the_device():
    import slr_sfs_amd
    L = slr_sfs_amd._lib.lib()
    p = ctypes.c_void_p(256)                                                # (never dereferenced: every call below is refused first)
    assert L.slr_conv4x4s2_grad_ws_bytes(1, 4, 4, 1, 8, 0) == 0             # H < 2
    assert L.slr_conv4x4s2_grad_ws_bytes(1, 4, 4, 8, 8, -1) == 0
    assert L.slr_conv4x4s2_grad_ws_bytes(2, 33, 31, 9, 8, 3) >= 3 * 16 * 33 * 31 * 4
    assert L.slr_motion_loss_ws_bytes(0, 4, 4) == 0 and L.slr_motion_loss_ws_bytes(2, 256, 256) >= 2 * 16 * 3 * 8
    assert L.slr_conv4x4s2_backward_data(None, None, p, p, 1, 4, 4, 8, 8, 0.2, None) == -1
    assert L.slr_conv4x4s2_backward_data(p, None, p, p, 1, 4, 4, 1, 8, 0.2, None) == -1
    assert b"H, W >= 2" in L.slr_last_error()
    assert L.slr_conv4x4s2_weight_grad(p, p, p, None, 1, 4, 4, 8, 8, 1, 0.2, 0, None, 0, None) != 0          # no workspace
    assert L.slr_instnorm_spade_train_forward(p, p, p, p, p, 1, 4, 1, 3, 1e-5, None) == -1                     # plane of 3 elements
    assert L.slr_instnorm_spade_backward(p, p, p, p, p, p, None, 1, 4, 4, 4, None) == -1
    assert L.slr_upsample2x_concat_backward(p, None, p, 4, None, 0, p, None, 1, 4, 4, 3, 2, None) == -1         # relu = 2 without fwd
    assert L.slr_upsample2x_concat_backward(p, None, None, 4, None, 0, p, None, 1, 4, 4, 3, 1, None) == -1      # relu = 1 without a
    assert L.slr_upsample2x_concat_backward(p, None, None, 4, None, 4, p, None, 1, 4, 4, 3, 0, None) == -1      # Cb without gb
    assert L.slr_motion_loss(p, p, p, 1, 4, 4, None, 0, None) != 0
    assert L.slr_motion_loss_grad(p, p, None, None, None, 1, 4, 4, None) == -1


def test_operators_refuse_cpu_tensors_and_wrong_types():
    import slr_sfs_amd as S
    x, w = torch.zeros(1, 3, 4, 4), torch.zeros(5, 3, 4, 4)
    for call in (lambda: S.conv4x4s2(x, w), lambda: S.instnorm_spade_train(x, torch.zeros(1, 6, 4, 4)),
                 lambda: S.upsample2x_concat_train(x, x, 3, S.motion_training.RELU_AFTER),
                 lambda: S.motion_losses(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: S.conv4x4s2(x, [1.0]), lambda: S.instnorm_spade_train(None, x), lambda: S.upsample2x_concat_train(x, 3),
                 lambda: S.motion_losses(x, 1.0)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(NotImplementedError, match="Reconstruction"):
        S.MotionLoss(types.SimpleNamespace(motion_losses=["1.0_Reconstruction"]))
    with pytest.raises(ValueError):
        S.MotionLoss(types.SimpleNamespace(motion_losses=["EndPointError"]))
    assert S.MotionLoss(types.SimpleNamespace(motion_losses=["10.0_EndPointError"])).lambdas == [10.0]


# ------------------------------------------------------------------ the criterion rejects the wrong variants

def _outside(name, wrong64, right64, plain32):
    """True if the float64 WRONG variant misses the device tests' bound; None where the variant changes nothing (a degenerate shape)."""
    if torch.equal(wrong64, right64):
        return None
    e_wrong, b = G.E(wrong64, right64), G.bound(G.E(plain32, right64))
    print(f"{name}: E_wrong {e_wrong:.3e}  bound {b:.3e}  factor {e_wrong / b:.3g}")
    return not (e_wrong <= b)                                               # (a NaN is outside)


def _all_outside(results):
    seen = [r for r in results if r is not None]
    assert seen and all(seen), results


def test_criterion_rejects_instance_norm_backward_without_the_xhat_term():
    res = []
    for shape in G.NORM_SHAPES:
        c = G._norm_case(shape)
        _, xh, rstd = M64.instnorm_spade_forward(c["x"].double(), c["gb"].double())
        gx, _ = M64.instnorm_spade_backward(c["g"].double(), c["gb"].double(), xh, rstd, wrong="norm_no_xhat_term")
        res.append(_outside(f"gx {shape}", gx, c["r64"]["gx"], c["r32"]["gx"]))
    _all_outside(res)


def test_criterion_rejects_bilinear_up_sampling_of_the_nearest_channel():
    res = []
    for size in G.UP_SIZES:
        for channels in G.UP_CHANNELS[:4]:
            for relu in (M64.RELU_NONE, M64.RELU_BEFORE, M64.RELU_AFTER):
                c = G._up_case(size, channels, relu)
                a, b = c["a"].double(), None if c["b"] is None else c["b"].double()
                ga, _ = M64.upsample_concat_backward(c["g"].double(), c["r64"]["out"], a, b, 3, relu, wrong="nearest_channel_bilinear")
                res.append(_outside(f"ga {size} {channels} relu {relu}", ga, c["r64"]["ga"], c["r32"]["ga"]))
    assert res.count(None) == 3 * 4                                          # a 1 x 1 source: nearest and bilinear are the same
    _all_outside(res)


@pytest.mark.parametrize("wrong", ["no_leaky_gate", "padding2_taps"])
def test_criterion_rejects_wrong_convolution_data_gradients(wrong):
    res = []
    for shape in G.CONV_SHAPES:
        c = G._conv_case(shape)
        r64, r32 = c["refs"][(torch.float64, G.SLOPE, False)], c["refs"][(torch.float32, G.SLOPE, False)]
        dx = M64.conv_backward_data(c["g"].double(), c["w"].double(), c["x"].double(), G.SLOPE, wrong=wrong)
        res.append(_outside(f"dx {shape}", dx, r64["dx"], r32["dx"]))
    _all_outside(res)


def test_criterion_rejects_an_endpoint_error_gradient_that_is_not_zeroed():
    res = []
    for shape in G.LOSS_SHAPES:
        c = G._loss_case(shape)
        g = M64.motion_losses_grad(c["pred"].double(), c["gt"].double(), 1.0, 0.0, wrong="epe_grad_not_zeroed")
        assert torch.isnan(g).any()
        if shape == (1, 1, 1):                                              # (the right gradient is all zero here: nothing to scale E by)
            continue
        res.append(_outside(f"g_epe {shape}", g, c["r64"]["g_epe"], c["r32"]["g_epe"]))
    _all_outside(res)


def test_criterion_rejects_an_ignored_first_lambda():
    c = G._loss_case((2, 3, 5))
    lam = [10.0, 3.0]
    right = M64.total_loss([c["r64"]["epe"], c["r64"]["l1"]], lam)
    plain = M64.total_loss([c["r32"]["epe"], c["r32"]["l1"]], lam)
    wrong = M64.total_loss([c["r64"]["epe"], c["r64"]["l1"]], lam, wrong="first_lambda_ignored")
    _all_outside([_outside("Total Loss", wrong, right, plain)])
