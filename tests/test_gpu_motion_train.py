"""The operators that train the SPADE motion U-Net on the device (slr_sfs_amd.motion_training; csrc/motion_grad.hip, the padding-1 modes of
csrc/conv4x4.hip and csrc/disc.hip) against the float64 definitions of tests/motion_train_f64.py.

Criterion (tests/test_gpu_conv_train.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the
same written-out definition evaluated by torch in float32 on the CPU against float64, computed in the test from the test's inputs and
never from the kernels.  Inputs are gate-clean: whatever a sign or a comparison is taken of is either exactly zero in every arithmetic or
well away from zero.  Every run is repeated once and compared bit for bit.  Every test prints its figures (run with -s)."""
import functools
import types

import pytest
import torch

import motion_train_f64 as M64

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOPE = 0.2
# N, Cin, Cout, H, W: the smallest image, odd sizes, channel counts off 32, several channel tiles (K split over waves at 256), the
# network's first levels' size
CONV_SHAPES = ((1, 1, 1, 2, 2), (1, 7, 5, 2, 6), (1, 3, 33, 5, 9), (2, 6, 32, 4, 4), (2, 33, 31, 8, 8), (2, 256, 256, 2, 2), (1, 32, 64, 64, 64))
ZEROS_SHAPE = (2, 33, 31, 8, 8)                                             # this case has exact zeros in x
NORM_SHAPES = ((1, 1, 2, 2), (2, 3, 2, 2), (1, 5, 3, 7), (3, 33, 5, 4), (2, 8, 16, 16), (1, 2, 128, 128))
UP_SIZES = ((1, 1), (1, 2), (2, 1), (3, 5), (16, 16), (64, 64))
UP_CHANNELS = ((8, 0, 3), (8, 8, 3), (4, 4, 3), (5, 3, 3), (1, 0, -1))      # Ca, Cb, nearest_channel
LOSS_SHAPES = ((1, 1, 1), (2, 3, 5), (2, 256, 256))
_id = lambda s: "x".join(map(str, s))                                       # noqa: E731


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def E(got, ref):
    return float((got.detach().cpu().double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def bound(e_plain):
    return 10.0 * e_plain + 1e-6


def held(name, got, ref64, plain32):
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    e_gpu, e_plain = E(got, ref64), E(plain32, ref64)
    print(f"{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    assert e_gpu <= bound(e_plain), (name, e_gpu, e_plain)


def same_bits(first, again, tag):
    for a, b in zip(first, again):
        assert (a is None and b is None) or torch.equal(a, b), tag


# ------------------------------------------------------------------ 1. the encoder convolution

@functools.lru_cache(maxsize=None)
def _conv_case(shape):
    """Seeded float32 inputs and the written-out definition in float64 and float32, computed once.  x keeps 1e-3 from zero (the LeakyReLU
    gate), except the planted exact zeros of ZEROS_SHAPE, whose gate (slope) every arithmetic takes alike."""
    N, cin, cout, H, W = shape
    gen = torch.Generator().manual_seed(cin * 1000 + cout * 10 + H)
    r = lambda *sh: torch.randn(*sh, generator=gen)                        # noqa: E731
    OH, OW = M64.out_size(H), M64.out_size(W)
    x, w, b, g = r(N, cin, H, W), r(cout, cin, 4, 4) / (4.0 * cin ** 0.5), r(cout), r(N, cout, OH, OW)
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 1e-3), x)
    if shape == ZEROS_SHAPE:
        x[:, ::3, ::2, 1::3] = 0.0
        x[:, :, 0, 0] = 0.0
    g = g * (1.0 + torch.arange(OW) / OW)                                   # (an incoming gradient that is not constant in any direction)
    u, v = r(cout), r(cin * 16)
    u, v = u / u.norm(), v / v.norm()
    scale = (1.0 / (u.double() @ w.double().reshape(cout, -1) @ v.double())).float().reshape(1)

    def ref(dt, slope, scaled):
        a = lambda t: t.to(dt)                                             # noqa: E731
        we = a(w) * a(scale) if scaled else a(w)
        dw, db = M64.conv_weight_grad(a(x), a(g), slope)
        out = dict(out=M64.conv_forward(a(x), we, a(b), slope), out0=M64.conv_forward(a(x), we, None, slope),
                   dx=M64.conv_backward_data(a(g), we, a(x), slope), db=db)
        out["dw"] = dw * a(scale) if scaled else dw
        out["dw_sn"] = M64.sn_weight_grad(dw, a(w), a(u), a(v), a(scale)) if scaled else None
        return out
    refs = {(dt, slope, scaled): ref(dt, slope, scaled) for dt in (torch.float64, torch.float32) for slope in (None, SLOPE)
            for scaled in (False, True)}
    return dict(x=x, w=w, b=b, g=g, u=u, v=v, scale=scale, refs=refs)


def _run_conv(S, c, bias, slope, scaled, spectral, splits=0):
    x, w = c["x"].to(DEV).requires_grad_(), c["w"].to(DEV).requires_grad_()
    b = c["b"].to(DEV).requires_grad_() if bias else None
    kw = {}
    if scaled:
        kw["weight_scale"] = c["scale"].to(DEV)
    if spectral:
        kw["spectral"] = (c["u"].to(DEV), c["v"].to(DEV))
    out = S.conv4x4s2(x, w, b, leaky=slope, _splits=splits, **kw)
    out.backward(c["g"].to(DEV))
    return out.detach(), x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_id)
def test_conv4x4s2_forward_backward_data_weight_gradient(S, shape):
    c = _conv_case(shape)
    if shape == ZEROS_SHAPE:
        assert int((c["x"] == 0).sum()) > 50
    # bias, LeakyReLU, weight_scale, spectral=(u, v), splits of the weight gradient
    for bias, slope, scaled, spectral, splits in ((True, SLOPE, False, False, 0), (False, None, False, False, 0), (True, None, True, False, 1),
                                                  (False, SLOPE, True, True, 3), (True, SLOPE, True, True, 0)):
        r64, r32 = c["refs"][(torch.float64, slope, scaled)], c["refs"][(torch.float32, slope, scaled)]
        tag = f"bias {int(bias)} slope {slope} scaled {int(scaled)} spectral {int(spectral)} splits {splits}"
        out, dx, dw, db = _run_conv(S, c, bias, slope, scaled, spectral, splits)
        ko, kw = "out" if bias else "out0", "dw_sn" if spectral else "dw"
        held(f"out {tag}", out, r64[ko], r32[ko])
        held(f"dx {tag}", dx, r64["dx"], r32["dx"])
        held(f"dw {tag}", dw, r64[kw], r32[kw])
        if bias:
            held(f"db {tag}", db, r64["db"], r32["db"])
        same_bits((out, dx, dw, db), _run_conv(S, c, bias, slope, scaled, spectral, splits), tag)


def test_conv4x4s2_forward_is_the_inference_kernel(S):
    """The training forward is slr_conv4x4s2_forward on the same fragments: bit-equal to nets.Conv4x4s2."""
    c = _conv_case((2, 33, 31, 8, 8))
    layer = S.nets.Conv4x4s2(33, 31).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(c["w"])
        layer.bias.copy_(c["b"])
        want = layer(c["x"].to(DEV), leaky=SLOPE)
    got = S.conv4x4s2(c["x"].to(DEV), c["w"].to(DEV), c["b"].to(DEV), leaky=SLOPE)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 2. SPADE instance norm

@functools.lru_cache(maxsize=None)
def _norm_case(shape):
    """One constant plane (16 x 16 of 0.75: every partial sum is exact, so the variance is exactly 0 in every arithmetic) and one plane
    with mean 100 and deviation 0.01 (128 x 128)."""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(C * 100 + H * 10 + W)
    r = lambda *sh: torch.randn(*sh, generator=gen)                        # noqa: E731
    x, gb, g = r(N, C, H, W) * 1.5 + 0.3, r(N, 2 * C, H, W) * 0.5, r(N, C, H, W)
    if shape == (2, 8, 16, 16):
        x[1, 2] = 0.75
    if shape == (1, 2, 128, 128):
        x[0, 1] = 100.0 + 0.01 * r(H, W)

    def ref(dt):
        out, xh, rstd = M64.instnorm_spade_forward(x.to(dt), gb.to(dt))
        gx, dgb = M64.instnorm_spade_backward(g.to(dt), gb.to(dt), xh, rstd)
        return dict(out=out, gx=gx, dgb=dgb)
    return dict(x=x, gb=gb, g=g, r64=ref(torch.float64), r32=ref(torch.float32))


def _run_norm(S, c):
    x, gb = c["x"].to(DEV).requires_grad_(), c["gb"].to(DEV).requires_grad_()
    out = S.instnorm_spade_train(x, gb)
    out.backward(c["g"].to(DEV))
    return out.detach(), x.grad, gb.grad


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_id)
def test_instnorm_spade_train(S, shape):
    c = _norm_case(shape)
    first = _run_norm(S, c)
    for name, got in zip(("out", "gx", "dgb"), first):
        held(name, got, c["r64"][name], c["r32"][name])
    same_bits(first, _run_norm(S, c), shape)
    # the forward is the inference kernel's own code
    assert torch.equal(first[0], S.nets.instnorm_spade(c["x"].to(DEV), c["gb"].to(DEV)))
    if shape == (2, 8, 16, 16):                                             # the constant plane: x-hat = 0, out = beta, d gamma = 0
        assert torch.equal(first[0][1, 2].cpu(), c["gb"][1, 8 + 2])
        assert float(first[2][1, 2].abs().max()) == 0.0


# ------------------------------------------------------------------ 3. up-sampling + concatenation

@functools.lru_cache(maxsize=None)
def _up_case(size, channels, relu):
    """Sources of small integers / 4: with the weights 1/4 and 3/4 every up-sampled value is exact in float32, so the result's sign (the
    RELU_AFTER gate) is the same in every arithmetic; zeros are planted in the sources (RELU_BEFORE) and, through an all-zero block, in the
    result (RELU_AFTER)."""
    H, W = size
    Ca, Cb, q = channels
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + Ca + Cb + relu)
    src = lambda C: torch.randint(-8, 9, (2, C, H, W), generator=gen).float() / 4.0       # noqa: E731
    a, b = src(Ca), (src(Cb) if Cb else None)
    for t in (a,) if b is None else (a, b):
        t[:, :, : (H + 1) // 2, : (W + 1) // 2] *= (torch.arange(t.shape[1]) % 2).view(1, -1, 1, 1).float()   # zero blocks in the even channels
    g = torch.randn(2, Ca + Cb, 2 * H, 2 * W, generator=gen)

    def ref(dt):
        a_, b_ = a.to(dt), None if b is None else b.to(dt)
        out = M64.upsample_concat_forward(a_, b_, q, relu)
        ga, gb = M64.upsample_concat_backward(g.to(dt), out, a_, b_, q, relu)
        return dict(out=out, ga=ga, gb=gb)
    return dict(a=a, b=b, g=g, r64=ref(torch.float64), r32=ref(torch.float32))


def _run_up(S, c, q, relu):
    a = c["a"].to(DEV).requires_grad_()
    b = None if c["b"] is None else c["b"].to(DEV).requires_grad_()
    out = S.upsample2x_concat_train(a, b, q, relu)
    out.backward(c["g"].to(DEV))
    return out.detach(), a.grad, None if b is None else b.grad


@pytest.mark.parametrize("size", UP_SIZES, ids=_id)
def test_upsample2x_concat_train(S, size):
    for channels in UP_CHANNELS:
        for relu in (M64.RELU_NONE, M64.RELU_BEFORE, M64.RELU_AFTER):
            c = _up_case(size, channels, relu)
            tag = f"{size} {channels} relu {relu}"
            first = _run_up(S, c, channels[2], relu)
            assert torch.equal(first[0].cpu(), c["r64"]["out"].float()), tag            # (exact by construction)
            if relu == M64.RELU_AFTER and size[0] * size[1] > 1:
                assert int((first[0] == 0).sum()) > 0, tag
            held(f"ga {tag}", first[1], c["r64"]["ga"], c["r32"]["ga"])
            if channels[1]:
                held(f"gb {tag}", first[2], c["r64"]["gb"], c["r32"]["gb"])
            same_bits(first, _run_up(S, c, channels[2], relu), tag)


# ------------------------------------------------------------------ 4. the motion losses

@functools.lru_cache(maxsize=None)
def _loss_case(shape):
    N, H, W = shape
    gen = torch.Generator().manual_seed(N * 100 + H + W)
    pred, gt = torch.randn(N, 2, H, W, generator=gen) * 2.0, torch.randn(N, 2, H, W, generator=gen) * 2.0
    if H * W > 1:
        same = torch.rand(N, 1, H, W, generator=gen) < 0.25                 # pixels with pred == gt exactly
        same[0, 0, 0, 0] = True
        gt = torch.where(same, pred, gt)
        gt[:, 1, H // 2] = pred[:, 1, H // 2]                               # ... and one channel equal: sign(0) = 0 in the L1 part
    else:
        gt = pred.clone()                                                   # the one pixel has d = 0

    def ref(dt):
        epe, l1, mse = M64.motion_losses(pred.to(dt), gt.to(dt))
        return dict(epe=epe, l1=l1, mse=mse, g_epe=M64.motion_losses_grad(pred.to(dt), gt.to(dt), 1.0, 0.0),
                    g_l1=M64.motion_losses_grad(pred.to(dt), gt.to(dt), 0.0, 1.0),
                    g_both=M64.motion_losses_grad(pred.to(dt), gt.to(dt), 10.0, 3.0))
    return dict(pred=pred, gt=gt, r64=ref(torch.float64), r32=ref(torch.float32))


def _run_losses(S, c, w_epe, w_l1):
    pred = c["pred"].to(DEV).requires_grad_()
    epe, l1, mse = S.motion_losses(pred, c["gt"].to(DEV))
    (epe * w_epe + l1 * w_l1).backward()
    return epe.detach(), l1.detach(), mse.detach(), pred.grad


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=_id)
def test_motion_losses_values_and_gradient(S, shape):
    c = _loss_case(shape)
    r64, r32 = c["r64"], c["r32"]
    for key, w_epe, w_l1 in (("g_epe", 1.0, 0.0), ("g_l1", 0.0, 1.0), ("g_both", 10.0, 3.0)):
        first = _run_losses(S, c, w_epe, w_l1)
        for name, got in zip(("epe", "l1", "mse"), first[:3]):
            if float(r64[name].abs().max()) == 0.0:                         # (the one-pixel case: d = 0, every sum exactly 0)
                assert float(got.abs().max()) == 0.0, name
            else:
                held(name, got, r64[name], r32[name])
        assert torch.isfinite(first[3]).all()
        if float(r64[key].abs().max()) == 0.0:
            assert float(first[3].abs().max()) == 0.0, key
        else:
            held(key, first[3], r64[key], r32[key])
        # exactly 0 where pred == gt: no 0 / 0
        d = c["pred"] - c["gt"]
        assert float(first[3].cpu()[d == 0].abs().max()) == 0.0
        same_bits(first, _run_losses(S, c, w_epe, w_l1), key)


def test_motion_loss_dictionary(S):
    """MotionLoss: the reference's keys in its order, every term unscaled, Total Loss = sum of lambda * term with the FIRST lambda
    applied, and the gradient of Total Loss."""
    c = _loss_case((2, 3, 5))
    loss = S.MotionLoss(types.SimpleNamespace(motion_losses=["10.0_EndPointError", "3.0_MotionL1"]))
    pred = c["pred"].to(DEV).requires_grad_()
    out = loss(pred, c["gt"].to(DEV))
    assert list(out) == ["MotionL1", "Total Loss", "EndPointError"]          # dict(l, **loss_dir): the later term's keys come first
    out["Total Loss"].backward()
    r64, r32 = c["r64"], c["r32"]
    held("EndPointError", out["EndPointError"], r64["epe"], r32["epe"])
    held("MotionL1", out["MotionL1"], r64["l1"], r32["l1"])
    held("Total Loss", out["Total Loss"], M64.total_loss([r64["epe"], r64["l1"]], [10.0, 3.0]), M64.total_loss([r32["epe"], r32["l1"]], [10.0, 3.0]))
    held("d Total Loss", pred.grad, r64["g_both"], r32["g_both"])
    held("mse_err", loss.last_mse_err, r64["mse"], r32["mse"])


# ------------------------------------------------------------------ 5. the whole network, the round trip, one composed iteration

import motion_train_fixture as TF  # noqa: E402

# E_plain32 measured on the CPU for def32 against def64 on the fixture's state and batch (the largest over PredMotion, the losses, u / v
# and the 110 gradients): 9.7e-06 in train() mode, 1.2e-05 in eval().  The cap is three times the larger one -- far below the 0.03 of
# tests/test_gpu_train_step.py: no gate of this input flips in float32 (motion_train_fixture.SEED; one flip costs 1e-4 ... 1e-2).
E_PLAIN32_CAP = 3.6e-5
OPTS = dict(use_mask_as_motion_input=True, use_hint_as_motion_input=True, motion_norm_G="sync:spectral_instance", div_flow=TF.DIV_FLOW,
            W=TF.SIZE, motionH=TF.SIZE, motionW=TF.SIZE, motion_losses=TF.MOTION_LOSSES)


def _model(S, training):
    model = S.MotionTrainingModel(types.SimpleNamespace(**OPTS), nf=TF.NF)
    model.motion_predictor.load_reference_state_dict(TF.initial_state())
    return model.to(DEV).train(training)


def _batch():
    b = TF.batch()
    return {"images": [b["images"][0].to(DEV)], "motions": b["motions"].to(DEV), "hints": b["hints"].to(DEV)}


def _step(S, training):
    """One forward + backward: (losses, PredMotion, {reference key: gradient}, {reference key: u / v after the forward})."""
    model, b = _model(S, training), _batch()
    with _no_sync():
        losses, pred = model(b)
        losses["Total Loss"].backward()
    net = model.motion_predictor
    grads, after = {}, {}
    for key, t, sl in net._reference_entries():
        if key.endswith(("weight_u", "weight_v")):
            after[key] = t.detach().clone()
        else:
            grads[key] = (t.grad if sl is None else t.grad[sl]).clone()
    return {k: v.detach() for k, v in losses.items()}, pred["PredMotion"].detach(), grads, after, pred


class _no_sync:
    """Inside: anything that synchronises the host with the device raises."""

    def __enter__(self):
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


def held_capped(name, got, ref64, plain32, scale=None, missed=None):
    """``held`` with the error relative to ``scale`` (default max|ref64|) and E_plain32 <= E_PLAIN32_CAP, so the bound cannot go slack.
    ``missed``: a list that collects the tensors outside the bound instead of stopping at the first (every figure is printed)."""
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    scale = float(ref64.double().abs().max()) if scale is None else scale
    e_gpu = float((got.detach().cpu().double() - ref64.double()).abs().max()) / scale
    e_plain = float((plain32.double() - ref64.double()).abs().max()) / scale
    print(f"{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    if missed is not None:
        if not (e_plain <= E_PLAIN32_CAP and e_gpu <= bound(e_plain)):
            missed.append((name, e_gpu, e_plain))
        return
    assert e_plain <= E_PLAIN32_CAP, (name, e_plain)
    assert e_gpu <= bound(e_plain), (name, e_gpu, e_plain)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_whole_network_losses_prediction_gradients_and_power_iteration(S, training):
    """MotionTrainingModel at nf = 8, N = 2, 256 x 256 on the fixture's state: every loss entry, PredMotion, every parameter gradient and
    u / v after the forward.  Measured E_plain32 (CPU, def32 against def64): at most 9.7e-06 (train) / 1.2e-05 (eval); cap 3.6e-05.
    Measured on the device: max E_gpu 6.0e-06 (train) / 3.7e-06 (eval)."""
    l64, p64, g64, a64 = TF.definition("float64", training)
    l32, p32, g32, a32 = TF.definition("float32", training)
    losses, pred, grads, after, pred_dict = _step(S, training)
    assert list(losses) == ["EndPointError", "Total Loss", "PSNR_motion"] and sorted(grads) == sorted(g64)
    assert list(pred_dict) == ["PredMotion", "GTMotion", "InputImg", "MovingMask", "HintMotion"]
    assert torch.equal(pred_dict["MovingMask"].cpu(), p64["MovingMask"].float())
    missed = []
    for k in losses:
        held_capped(f"loss {k}", losses[k].reshape(1), l64[k].reshape(1), l32[k].reshape(1), None, missed)
    held_capped("PredMotion", pred, p64["PredMotion"], p32["PredMotion"], None, missed)
    for k in sorted(grads):
        held_capped(f"grad {k}", grads[k], g64[k], g32[k], TF.grad_scale(g64, k), missed)
    for k in sorted(after):
        if training:
            held_capped(f"after {k}", after[k], a64[k], a32[k], None, missed)
        else:
            assert torch.equal(after[k].cpu(), TF.initial_state()[k]), k        # eval(): no power iteration
    assert not missed, missed
    again = _step(S, training)
    assert all(torch.equal(losses[k], again[0][k]) for k in losses) and torch.equal(pred, again[1])
    assert all(torch.equal(grads[k], again[2][k]) for k in grads) and all(torch.equal(after[k], again[3][k]) for k in after)


def test_reference_state_dict_round_trip_into_the_inference_network(S):
    """reference_state_dict -> nets.load_motion_state_dict -> nets.SPADEUnet4MaskMotion gives the trainable network's eval() output."""
    _, p64, _, _ = TF.definition("float64", False)
    _, p32, _, _ = TF.definition("float32", False)
    model = _model(S, False)
    b = _batch()
    sd = model.motion_predictor.reference_state_dict(TF.PREFIX)
    inference = S.nets.load_motion_state_dict(S.nets.SPADEUnet4MaskMotion(nf=TF.NF).to(DEV), sd, TF.PREFIX)
    x = torch.cat([b["images"][0], p64["MovingMask"].float().to(DEV), b["hints"]], 1)
    with torch.no_grad():
        trained = model.forward_flow(b["images"][0], p64["MovingMask"].float().to(DEV), b["hints"])["PredMotion"]
        served = inference(x) * TF.DIV_FLOW
    held_capped("trainable eval()", trained, p64["PredMotion"] * TF.DIV_FLOW, p32["PredMotion"] * TF.DIV_FLOW)
    held_capped("inference network", served, p64["PredMotion"] * TF.DIV_FLOW, p32["PredMotion"] * TF.DIV_FLOW)


def _iteration(S):
    """models/base_model_motion.py:122-178 with num_steps = 1: generator step (motion losses + adversarial), then discriminator step."""
    torch.manual_seed(7)
    model = _model(S, True)
    netD = S.DiscriminatorLoss(output_nc=2, ndf=8).to(DEV).train()
    opt_g = S.optim.Adam(model.parameters(), lr=5e-4, betas=(0.0, 0.9))
    opt_d = S.optim.Adam(netD.parameters(), lr=2e-3, betas=(0.0, 0.9))
    opt_g.zero_grad()
    t_losses, out = model(_batch())
    g_losses = netD.run_generator_one_step(out["PredMotion"], out["GTMotion"])
    (g_losses["Total Loss"] + t_losses["Total Loss"]).mean().backward()
    opt_g.step()
    opt_d.zero_grad()
    d_losses = netD.run_discriminator_one_step(out["PredMotion"], out["GTMotion"])
    d_losses["Total Loss"].mean().backward()
    opt_d.step()
    state = {"G/" + k: v.detach().clone() for k, v in model.state_dict().items()}
    state.update({"D/" + k: v.detach().clone() for k, v in netD.state_dict().items()})
    for tag, opt in (("optG", opt_g), ("optD", opt_d)):
        for i, st in opt.state_dict()["state"].items():
            state.update({f"{tag}/{i}/{k}": v.detach().clone() for k, v in st.items() if torch.is_tensor(v)})
    state.update({"loss/" + k: v.detach().clone() for k, v in {**t_losses, **g_losses, **d_losses}.items()})
    return state


def test_one_composed_iteration_has_the_same_bits_twice(S):
    first, again = _iteration(S), _iteration(S)
    assert sorted(first) == sorted(again) and len(first) > 200
    moved = sum(1 for k in first if k.startswith("G/") and "weight_orig" in k)
    assert moved == 16
    for k in first:
        assert torch.equal(first[k], again[k]), k
    init = TF.initial_state()
    assert not torch.equal(first["G/motion_predictor.conv1.weight_orig"].cpu(), init["conv1.weight_orig"])      # (the step moved the weights)
    assert all(torch.isfinite(v).all() for v in first.values() if v.is_floating_point())
