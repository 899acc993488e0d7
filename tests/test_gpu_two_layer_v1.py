"""The v1 two-layer model on the device (``blend_alpha0``, ``TwoLayerAlpha0TrainingModel``; csrc/layers.hip, ABI 25) against the float64
definition of tests/two_layer_v1_f64.py: the operator (forward and every gradient, rock masks, the exact zero without a moving pixel, the
1e-8 clamp, absent gradients, run-to-run bits, refusals), the alpha plane's splat as the model makes it -- a second ``splat_blend`` call
at C = 1 whose logits tensor is shared by both directions --, the same pair of calls against the inference path
(``ClipSynthesizer(use_alpha0=True)``), and the whole model at the fixture's shape: every loss, image and gradient, the buffers after the
forward against the reference's own v1 run, one iteration through ``Trainer`` bit for bit against the same iteration written out from
the public pieces, two deterministic iterations, the checkpoint, and the region losses' weights.

Criterion (tests/test_gpu_two_layer.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the
same written-out definition evaluated by torch in float32 on the CPU against float64, computed in the test from the test's inputs.  Every
test prints its figures (run with -s).

Shapes of the operator [N,H,W]: (1,1,1); (2,3,3): a sample boundary inside a thread's four pixels; (1,16,32): exactly one workgroup of
512 pixels; (1,19,27): 513 pixels, a tail and a second workgroup; (3,37,41): 4551 pixels, nine partial sums for the finish kernel."""
import functools

import numpy as np
import pytest
import torch

import blend_f64 as B64
import two_layer_f64 as D
import two_layer_v1_f64 as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = ((1, 1, 1), (2, 3, 3), (1, 16, 32), (1, 19, 27), (3, 37, 41))
BIG = (3, 37, 41)
GRAD = (0.7, -1.3)                                                          # the gradients reaching the two region losses
TARGET = 0.25
_id = lambda s: "x".join(map(str, s))                                       # noqa: E731


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def E(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaNs in other places than the definition's"
    if nan.all():
        return 0.0
    return float((got[~nan] - ref[~nan]).abs().max()) / max(float(ref[~nan].abs().max()), 1e-300)


def bound(e_plain):
    return 10.0 * e_plain + 1e-6


def held(name, got, ref64, plain32):
    e_gpu, e_plain = E(got, ref64), E(plain32, ref64)
    print(f"{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    assert e_gpu <= bound(e_plain), (name, e_gpu, e_plain)
    return e_gpu


# ------------------------------------------------------------------ blend_alpha0

@functools.lru_cache(maxsize=None)
def _case(shape, rock="mixed", sma="mixed", clamp=False, present=("c0", "values")):
    """Float32 inputs (CPU), the cotangent of c0, and the definition's outputs and gradient in float64 and float32, computed once."""
    a, r, s = V.alpha0_inputs(*shape, seed=sum(shape), dtype=torch.float32, rock=rock, sma=sma, clamp=clamp, target=TARGET)
    go = torch.randn(r.shape, generator=torch.Generator().manual_seed(13))

    def run(dt):
        x = a.to(dt).clone().requires_grad_(True)
        c0, losses = V.blend_alpha0(x, r.to(dt), s.to(dt), TARGET)
        total = (c0 * go.to(dt)).sum() if "c0" in present else 0.0
        if "values" in present:
            total = total + sum(losses[n] * g for n, g in zip(V.REGION_LOSS_NAMES, GRAD))
        return c0.detach(), {k: v.detach() for k, v in losses.items()}, torch.autograd.grad(total, x)[0]
    return (a, r, s), go, run(torch.float64), run(torch.float32)


def _device(S, inputs, go, present=("c0", "values"), need=True):
    a, r, s = (t.to(DEV) for t in inputs)
    a.requires_grad_(need)
    c0, losses = S.blend_alpha0(a, r, s, TARGET)
    if need:
        total = (c0 * go.to(DEV)).sum() if "c0" in present else 0.0
        if "values" in present:
            total = total + sum(losses[n] * g for n, g in zip(V.REGION_LOSS_NAMES, GRAD))
        total.backward()
    return c0, losses, a.grad


def _gate_clean(inputs, clamp=False):
    """Logits in [-4, 4] and |c0 - target| > 1e-3 on the rock region, in the float32 the device gets: the sign at the kink of the rock
    term is a decision, not a rounding (the fluid term's x - y = (c0 - 1) (1 - r) m is negative or exactly 0)."""
    a, r, s = inputs
    if clamp:                                                               # (the clamped pixels lie outside the gate on purpose)
        a = a.clone()
        a[0, :, 0, 0] = 0.0
        a[-1, :, -1, -1] = 0.0
    c0 = V.blend_alpha0(a.double(), r.double(), s.double(), TARGET)[0]
    assert float(a.abs().max()) <= 4.0
    assert bool((((c0 - TARGET).abs() > 1e-3) | (r == 0)).all())
    assert float(c0.max()) < 0.99


def _check(S, shape, **kw):
    inputs, go, (c64, l64, g64), (c32, l32, g32) = _case(shape, **kw)
    _gate_clean(inputs, kw.get("clamp", False))
    c0, losses, grad = _device(S, inputs, go, kw.get("present", ("c0", "values")))
    assert list(losses) == list(V.REGION_LOSS_NAMES) and all(v.dim() == 0 for v in losses.values())
    tag = f"{_id(shape)} {kw}"
    held(f"{tag} c0", c0, c64, c32)
    for n in V.REGION_LOSS_NAMES:
        held(f"{tag} {n}", losses[n], l64[n], l32[n])
    held(f"{tag} d a_start", grad, g64, g32)
    return inputs, c0, losses, grad


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_blend_alpha0_forward_and_every_gradient(S, shape):
    _check(S, shape)


@pytest.mark.parametrize("shape", [(2, 3, 3), BIG], ids=_id)
@pytest.mark.parametrize("rock", ["all", "none"])
def test_blend_alpha0_rock_masks(S, shape, rock):
    _check(S, shape, rock=rock)


@pytest.mark.parametrize("shape", [(2, 3, 3), BIG], ids=_id)
def test_blend_alpha0_without_a_moving_pixel_is_exactly_zero(S, shape):
    inputs, _, losses, grad = _check(S, shape, sma="all", present=("values",))
    assert all(float(v.detach()) == 0.0 for v in losses.values())
    assert float(grad.abs().max()) == 0.0
    _check(S, shape, sma="all")                                             # (with a gradient reaching c0: that one alone)


@pytest.mark.parametrize("shape", [(2, 3, 3), (1, 16, 32), BIG], ids=_id)
def test_blend_alpha0_where_the_clamp_bites(S, shape):
    """Both logits at -25: sigmoid(a1) + sigmoid(a0) < 1e-8, c0 = sigmoid(a1) / 1e-8 and nothing flows through the sum -- the definition
    (torch.clamp and its backward) takes the same decision in float64 and float32, so the criterion compares at that decision."""
    inputs, c0, _, grad = _check(S, shape, clamp=True)
    a = inputs[0].double()
    for n, y, x in ((0, 0, 0), (-1, -1, -1)):
        assert float(torch.sigmoid(a[n, :, y, x]).sum()) < 1e-8
        want = float(V.c0_clamped(a)[n, 0, y, x])
        assert abs(float(c0.detach()[n, 0, y, x]) - want) <= 1e-5 * want
        assert float(grad[n, 0, y, x]) == 0.0                               # the background logit is reached through the sum alone


def test_blend_alpha0_needs_input_grad_and_absent_gradients(S, monkeypatch):
    inputs, go, _, _ = _case(BIG)
    c0, losses, grad = _device(S, inputs, go, need=False)
    assert grad is None and not c0.requires_grad and not any(v.requires_grad for v in losses.values())
    calls = []
    real = S.layers._lib.call
    monkeypatch.setattr(S.layers._lib, "call", lambda name, dev, *args: (calls.append((name, args)), real(name, dev, *args))[1])
    full = _device(S, inputs, go)[2]
    assert [n for n, _ in calls] == ["slr_blend_alpha0_forward", "slr_blend_alpha0_backward"]      # one forward call, one backward call
    assert calls[1][1][3] is not None and calls[1][1][4] is not None
    for present, absent in ((("c0",), 4), (("values",), 3)):
        calls.clear()
        _check(S, BIG, present=present)
        assert calls[1][0] == "slr_blend_alpha0_backward" and calls[1][1][absent] is None and calls[1][1][7 - absent] is not None
    assert full is not None and full.shape == inputs[0].shape


def test_blend_alpha0_two_runs_have_the_same_bits(S):
    inputs, go, _, _ = _case(BIG)
    a, b = (_device(S, inputs, go) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[1][n], b[1][n]) for n in V.REGION_LOSS_NAMES)


def test_blend_alpha0_refuses_bad_arguments_on_the_device(S):
    a, r, s = (t.to(DEV) for t in _case((2, 3, 3))[0])
    with pytest.raises(ValueError, match="not contiguous"):
        S.blend_alpha0(torch.zeros(2, 2, 3, 3, device=DEV).transpose(2, 3), r, s)
    with pytest.raises(TypeError, match="float32"):
        S.blend_alpha0(a.double(), r, s)
    with pytest.raises(ValueError, match="a_start"):
        S.blend_alpha0(a[:, :1].contiguous(), r, s)
    with pytest.raises(ValueError, match="mask_rock"):
        S.blend_alpha0(a, r[:, :, :2].contiguous(), s)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        S.blend_alpha0(a, r.cpu(), s)
    with pytest.raises(TypeError, match="tensors required"):
        S.blend_alpha0(a, r, 0.0)


# ------------------------------------------------------------------ the second splat call as the model makes it
# C = 1, one logits tensor for both directions (values in (0, 1): a c0), clamp_z=None, subtract_max=False, at [2,1,40,72]: more than one
# tile each way, with partial tiles.  Flows: Euler-integrated smooth motion (it converges: pile-ups) and the families of
# tests/test_gpu_splat_blend.py.

SPLAT_SHAPE = (2, 1, 40, 72)
FLOWS = ("euler", "uniform3", "integer", "collapse", "nan")
SPLAT_NAMES = ("a_start", "a_end", "c0", "flow_f", "flow_p")


@functools.lru_cache(maxsize=None)
def _splat_case(kind):
    import test_gpu_splat_blend as SB
    from oracle import oracle as o
    o.build()
    c = SB.euler_case(o, SPLAT_SHAPE) if kind == "euler" else SB.family(o, kind, SPLAT_SHAPE, 4100 + FLOWS.index(kind), 1.0)
    rng = np.random.default_rng(77)
    t = dict(a_start=torch.from_numpy(c["start_fs"]), a_end=torch.from_numpy(c["end_fs"]),
             c0=torch.from_numpy(rng.uniform(0.02, 0.98, (2, 1, 40, 72)).astype(np.float32)),
             flow_f=torch.from_numpy(c["flow_f"]), flow_p=torch.from_numpy(c["flow_p"]))
    alpha, go = torch.from_numpy(c["alpha"]), torch.from_numpy(c["go"])

    def run(dt, cot=None):
        x = {k: v.to(dt).clone().requires_grad_(True) for k, v in t.items()}
        out, norm = B64.blend_f64(x["a_start"], x["c0"], x["flow_f"], x["a_end"], x["c0"], x["flow_p"], alpha, dt, clamp_z=None,
                                  subtract_max=False, return_norm=True)
        if cot is None:
            cot = (go.double() * norm.detach().clamp(max=1.0)).float()      # (tests/test_gpu_splat_blend.py's cotangent)
        return out.detach(), norm.detach(), dict(zip(SPLAT_NAMES, torch.autograd.grad(out, [x[k] for k in SPLAT_NAMES], cot.to(dt)))), cot
    r64 = run(torch.float64)
    return t, alpha, r64, run(torch.float32, r64[3])


def _splat_device(S, t, alpha, cot, deterministic):
    x = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    out, norm = S.splat_blend(x["a_start"], x["c0"], x["flow_f"], x["a_end"], x["c0"], x["flow_p"], alpha.to(DEV), clamp_z=None,
                              subtract_max=False, return_norm=True, **({"deterministic": True} if deterministic else {}))
    out.backward(cot.to(DEV))
    return out.detach(), norm, {k: x[k].grad for k in SPLAT_NAMES}


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("front", ["scan", "rows"])
@pytest.mark.parametrize("kind", FLOWS)
def test_alpha_plane_splat_call_against_float64(S, kind, front, deterministic):
    import test_gpu_splat_blend_deterministic as DT
    t, alpha, (o64, n64, g64, cot), (o32, n32, g32, _) = _splat_case(kind)
    with DT._front_end(S, front):
        out, norm, grads = _splat_device(S, t, alpha, cot, deterministic)
        tag = f"{kind} {front} {'det' if deterministic else 'default'}"
        held(f"{tag} out", out, o64, o32)
        held(f"{tag} norm", norm, n64, n32)
        for k in SPLAT_NAMES:                                               # c0: the sum over both directions
            held(f"{tag} d {k}", grads[k], g64[k], g32[k])
        if deterministic:
            again = _splat_device(S, t, alpha, cot, True)
            assert torch.equal(out, again[0]) and torch.equal(norm, again[1])
            assert all(torch.equal(grads[k], again[2][k]) for k in SPLAT_NAMES)
            assert int(S.training.splat_blend_fallback_count(torch.empty(SPLAT_SHAPE, device=DEV)).item()) == 0


def test_the_pair_of_splat_calls_is_the_inference_path(S):
    """start == end, batch 1, indices (0, t, N - 1): what the model computes is what ``ClipSynthesizer(use_alpha0=True).features(t)``
    renders from a v1 checkpoint, to the tolerance tests/test_gpu_parity.py holds those two outputs to."""
    import test_gpu_gradients as TG
    C, H, W, N, t = 8, 40, 72, 12, 5
    g = torch.Generator().manual_seed(31)
    fs, Z = torch.randn(1, C, H, W, generator=g).to(DEV), (0.7 * torch.randn(1, 1, H, W, generator=g)).to(DEV)
    a = (torch.rand(1, 2, H, W, generator=g) * 8 - 4).to(DEV)
    motion = torch.from_numpy(TG.smooth_motion(H, W, 5, amp=2.0)).to(DEV)
    assert float((Z - Z.max()).min()) >= -20.0                              # the training path clamps there, the inference path does not
    rock, sma = torch.zeros(1, 1, H, W, device=DEV), torch.zeros(1, 1, H, W, device=DEV)
    c0, _ = S.blend_alpha0(a, rock, sma)
    euler = S.EulerIntegration(None)
    s, m, e = (torch.tensor([v], device=DEV) for v in (0, t, N - 1))
    flow_f, flow_p = euler(motion, m.long() - s.long()), euler(-motion, e.long() + 1 - m.long())
    alpha = torch.clamp(1.0 - (m.float() - s.float()) / (e.float() - s.float() + 1), min=1.0 / 600.0, max=599.0 / 600.0)
    gen = S.splat_blend(fs, Z, flow_f, fs, Z, flow_p, alpha)
    plane = a[:, 1:2].contiguous()
    afl = S.splat_blend(plane, c0, flow_f, plane, c0, flow_p, alpha, clamp_z=None, subtract_max=False)
    clip = S.synthesis.ClipSynthesizer(fs, Z, motion, N, alpha_fluid_logit=plane, alpha_bg=torch.sigmoid(a[:, 0:1]), use_alpha0=True)
    ref_gen, ref_afl = clip.features(t)
    np.testing.assert_allclose(gen.cpu().numpy(), ref_gen.cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(afl.cpu().numpy(), ref_afl.cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert float(afl.abs().max()) > 0.5 and float(gen.abs().max()) > 0.5


# ------------------------------------------------------------------ the whole model at the fixture's shape
# batch 2, 32 x 32, ngf 16, the narrow widths of tests/two_layer_f64.py; the state, the batch and the noise of every network call are the
# reference's run's (tests/golden/two_layer_train_vs_reference.npz), the results its v1 run's (two_layer_v1_train_vs_reference.npz).

import train_step_f64 as T64  # noqa: E402

PLAIN_CAP = 0.03                                                            # the cap of tests/train_step_f64.py on E_plain32


@functools.lru_cache(maxsize=None)
def _fixture():
    g = V.load()
    return g, D.state_dict(g)


def _T2():
    import test_gpu_two_layer as T2                                         # its fixture helpers: the batch and the seeded VGG19
    return T2


def _model(S, deterministic=False, **more):
    model = S.TwoLayerAlpha0TrainingModel(V.options(**more), _T2()._vgg(S), deterministic=deterministic, **D.model_kwargs())
    return model.to(DEV).train().load_reference_state_dict(_fixture()[1])


@functools.lru_cache(maxsize=None)
def _reference(dtype):
    nets = D.generator(_fixture()[0], dtype)
    loss, pred = V.model_forward_v1(nets, D.fixture_inputs(_fixture()[0]), dtype)
    loss["Total Loss"].backward()
    return ({k: v.detach() for k, v in loss.items()}, {k: v.detach() for k, v in pred.items()},
            {k: t.grad for k, t in nets["leaves"].items()})


def test_model_against_float64_and_the_references_buffers(S):
    g = _fixture()[0]
    model = _model(S)
    loss, pred = model(_T2()._batch())
    loss["Total Loss"].backward()
    (l64, p64, g64), (l32, p32, g32) = _reference(torch.float64), _reference(torch.float32)
    assert list(loss) == g["loss_keys"] and list(pred) == g["pred_keys"]    # the reference's keys, in its order
    worst = 0.0
    for kind, got, r64, r32 in (("loss", loss, l64, l32), ("pred", pred, p64, p32)):
        for k in got:
            assert E(r32[k], r64[k]) <= PLAIN_CAP, k
            worst = max(worst, held(f"{kind} {k}", got[k], r64[k], r32[k]))
    rows = {k: t for k, t, learns in model.reference_parameters() if learns and not k.startswith("loss_function")}
    assert set(g64) <= set(rows)
    for k, t in rows.items():
        if k not in g64:                                                    # (a decoder's conv_b that no block uses)
            assert t.grad is None or float(t.grad.abs().max()) == 0.0, k
    for k, (e, e_plain, bnd) in T64.figures({k: rows[k].grad for k in g64}, g64, g32).items():
        print(f"d {k}: E_gpu {e:.3e}  E_plain32 {e_plain:.3e}  bound {bnd:.3e}")
        assert e_plain <= PLAIN_CAP, (k, e_plain)
        assert e <= bnd, (k, e, e_plain)
        worst = max(worst, e)
    print(f"largest E_gpu {worst:.3e}")
    # the buffers after the forward are the reference's v1 run's: u, v, and the batch statistics -- the alpha decoder's differ from v2's
    sd, n = model.reference_state_dict("model."), 0
    for k in g:
        if k.startswith("after/"):
            got, ref = sd["model." + k[6:]].double().cpu(), torch.from_numpy(g[k]).double()
            assert float((got - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max())), k
            n += 1
    assert n > 600


def _through_trainer(S, use_d, cls=None):
    opts = V.options(discriminator_losses="pix2pixHD" if use_d else "0")
    model = (cls or S.TwoLayerAlpha0TrainingModel)(opts, _T2()._vgg(S), deterministic=True, **D.model_kwargs())
    torch.manual_seed(11)
    trainer = S.Trainer(model, opts).to(DEV).train()
    model.load_reference_state_dict(_fixture()[1])
    losses, images = trainer(iter([_T2()._batch()]))
    snap = _T2()._snapshot
    return trainer, {"losses": snap(losses.items()), "tensors": snap(trainer.reference_state_dict().items()),
                     "pred": images["PredImg"].detach().clone()}


def _by_hand(S, use_d):
    """base_model.py:95-163 on the v1 forward, written out from the public pieces (the deterministic splat on both sides, so that the
    bits can be compared)."""
    from slr_sfs_amd import spectral
    opts, sd, b = V.options(discriminator_losses="pix2pixHD" if use_d else "0"), _fixture()[1], _T2()._batch()
    kw = D.model_kwargs()
    nets = {"encoder": S.TrainableEncoderWithZ(cin=3, feat=D.FEAT, widths=kw["encoder_widths"], spectral=True),
            "net_bg": S.TrainableBGDecoder(cin=3, cout=3, widths=kw["bg_widths"], updown=kw["bg_updown"], spectral=True),
            "net_alpha_encoder": S.TrainableEncoder(cin=3, cout=2, widths=kw["alpha_encoder_widths"], spectral=True),
            "net_alpha_decoder": S.TrainableDecoderPconv2(cin=D.FEAT + 1, cout=1, widths=kw["alpha_decoder_widths"],
                                                          updown=kw["alpha_decoder_updown"], spectral=True),
            "projector": S.TrainableDecoderPconv2(cin=D.FEAT, cout=3, widths=kw["decoder_widths"], updown=kw["decoder_updown"], spectral=True)}
    for name, net in nets.items():
        net.to(DEV).train()
        spectral.load_spectral_state_dict(net, sd, f"model.module.{name}.")
    loss_fn, euler = S.losses.SynthesisLoss(opts, _T2()._vgg(S)), S.EulerIntegration(opts)
    params = [p for net in nets.values() for p in net.parameters() if p.requires_grad]
    betas = (opts.beta1, opts.beta2) if use_d else (0.99, opts.beta2)
    opt_g = S.optim.Adam(params, lr=opts.lr_g, betas=betas)
    if use_d:
        torch.manual_seed(11)
        netD = S.DiscriminatorLoss(gan_mode="hinge", lambda_feat=10.0, no_ganFeat_loss=False, ndf=8, output_nc=3).to(DEV).train()
        opt_d = S.optim.Adam(list(netD.parameters()), lr=opts.lr_d, betas=betas)
    start, middle, end = b["images"]
    nz, flow, index = b["noise"], b["motions"], b["index"]
    speed = (flow[:, 0:1] ** 2 + flow[:, 1:2] ** 2).sqrt()
    sma = (speed < speed.mean([1, 2, 3], True) * 0.1).float()
    with torch.no_grad():
        nets["encoder"](start, noise=nz["start_dropped"])
        nets["encoder"](end, noise=nz["end_dropped"])
    s_fs, z_f = nets["encoder"](start, noise=nz["start"])
    e_fs, z_p = nets["encoder"](end, noise=nz["end"])
    bg_raw = nets["net_bg"](start, noise=nz["bg"])
    a_s, a_e = nets["net_alpha_encoder"](start, noise=nz["alpha_start"]), nets["net_alpha_encoder"](end, noise=nz["alpha_end"])
    s, m, e = index[:, 0], index[:, 1], index[:, 2]
    flow_f, flow_p = euler(flow, m.long() - s.long()), euler(-flow, e.long() + 1 - m.long())
    alpha = torch.clamp(1.0 - (m.float() - s.float()) / (e.float() - s.float() + 1), min=1.0 / 600.0, max=599.0 / 600.0).contiguous()
    c0, region = S.blend_alpha0(a_s, b["mask_rock"], sma, rock_target=opts.RockRegionlosstarget)
    gen_fs, norm = S.splat_blend(s_fs.contiguous(), z_f, flow_f, e_fs.contiguous(), z_p, flow_p, alpha, return_norm=True, deterministic=True)
    afl = S.splat_blend(a_s[:, 1:2].contiguous(), c0, flow_f, a_e[:, 1:2].contiguous(), c0, flow_p, alpha, clamp_z=None, subtract_max=False,
                        deterministic=True)
    fluid_raw = nets["projector"](gen_fs, noise=nz["projector"])
    far = nets["net_alpha_decoder"](torch.cat([gen_fs, afl], 1), noise=nz["alpha_decoder"])
    pred, _, bg, _ = S.layer_composite(fluid_raw, bg_raw, far, a_s[:, 0:1].contiguous())
    loss = loss_fn(pred, middle)
    terms, _, _ = S.alpha_losses(a_s, b["mask_rock"], sma, afl.detach(), norm.detach().contiguous(), far, reweight=False)
    total = loss["Total Loss"] + terms["AlphaTV"] * opts.ATVloss
    lb = loss_fn(bg, b["mean_video"][0])
    total = total + lb["Total Loss"] * opts.MVloss
    total = total + region["FluidRegionLoss"] * opts.FluidRegionloss
    total = total + region["RockRegionLoss"] * opts.RockRegionloss
    total = total + terms["Alpha Decoder Consistency Loss"] * opts.ADCloss
    total = total + terms["Moving Region Alpha Decoder Consistency Loss"] * opts.MRADCloss
    opt_g.zero_grad()
    if use_d:
        g_losses = netD.run_generator_one_step(pred, middle)
        (g_losses["Total Loss"] / 1.0 + total / 1.0).mean().backward()
    else:
        (total / 1.0).mean().backward()
    opt_g.step()
    tensors = {f"model.module.{name}.{k}": t for name, net in nets.items() for k, t in spectral._entries(net).items()}
    if use_d:
        opt_d.zero_grad()
        d_losses = netD.run_discriminator_one_step(pred, middle)
        (d_losses["Total Loss"] / 1.0).mean().backward()
        opt_d.step()
        tensors.update({"netD." + k: t for k, t in netD.state_dict().items()})
    return {"total": total.detach().clone(), "tensors": _T2()._snapshot(tensors.items()), "pred": (0.5 * pred + 0.5).detach().clone()}


@pytest.mark.parametrize("use_d", [True, False], ids=["with-D", "without-D"])
def test_one_iteration_through_trainer_has_the_bits_of_the_hand_written_one(S, use_d):
    """``Trainer`` takes the v1 model as it takes the others: one iteration, both optimiser steps."""
    _, got = _through_trainer(S, use_d)
    hand = _by_hand(S, use_d)
    assert torch.equal(got["losses"]["Total Loss"], hand["total"])
    assert torch.equal(got["pred"], hand["pred"])
    moved = 0
    for k, t in hand["tensors"].items():
        assert torch.equal(got["tensors"][k], t), k
        moved += not torch.equal(t.cpu(), _fixture()[1][k]) if k in _fixture()[1] else 0
    assert moved > 300                                                      # the parameters of all five networks took the step


def test_two_deterministic_iterations_have_the_same_bits(S):
    (_, a), (_, b) = _through_trainer(S, True), _through_trainer(S, True)
    _T2()._same_bits(a, b, "iteration")
    for C in (D.FEAT, 1):                                                   # the workspaces of both splat calls
        assert int(S.training.splat_blend_fallback_count(torch.empty(2, C, 32, 32, device=DEV)).item()) == 0


def test_checkpoint_round_trips_and_loads_into_the_v2_model(S):
    snap, same = _T2()._snapshot, _T2()._same_bits
    a, _ = _through_trainer(S, True)
    ckpt = a.reference_checkpoint()
    g = _fixture()[0]
    assert ckpt["optimizerG"]["param_groups"][0]["params"] == list(range(len(g["parameter_order"])))
    for cls, opts in ((S.TwoLayerAlpha0TrainingModel, V.options(discriminator_losses="pix2pixHD")),
                      (S.TwoLayerTrainingModel, D.options(discriminator_losses="pix2pixHD"))):      # the same keys: a v1 checkpoint loads into either
        b = S.Trainer(cls(opts, _T2()._vgg(S), deterministic=True, **D.model_kwargs()), opts).to(DEV).train()
        b.load_reference_checkpoint(ckpt)
        back = b.reference_checkpoint()
        same(snap(ckpt["state_dict"].items()), snap(back["state_dict"].items()), "state_dict")
        for name in ("optimizerG", "optimizerD"):
            assert back[name]["param_groups"] == ckpt[name]["param_groups"]
            same({k: snap(st.items()) for k, st in ckpt[name]["state"].items()},
                 {k: snap(st.items()) for k, st in back[name]["state"].items()}, name)
    sd = dict(_fixture()[1])
    model = a.model
    for bad in ({k: v for k, v in sd.items() if not k.endswith("net_bg.eblocks.0.ch_a.2.weight_u")}, dict(sd, **{"model.module.extra": sd["model.module.min_z"]})):
        with pytest.raises(KeyError):
            model.load_reference_state_dict(bad)


def test_a_weight_of_zero_skips_a_region_term_and_the_weights_are_read_at_each_forward(S):
    model = _model(S, deterministic=True)
    full, _ = model(_T2()._batch())
    model = _model(S, deterministic=True)
    model.opt.FluidRegionloss, model.opt.RockRegionloss = 0.0, 28.5          # (the training script decays both weights every epoch)
    less, _ = model(_T2()._batch())
    assert "FluidRegionLoss" not in less and torch.equal(less["RockRegionLoss"], full["RockRegionLoss"])
    model = _model(S, deterministic=True)
    model.opt.RockRegionloss = 0.0
    none, _ = model(_T2()._batch())
    assert "RockRegionLoss" not in none and "FluidRegionLoss" in none
    full, less, none = ({k: float(v.detach()) for k, v in d.items()} for d in (full, less, none))
    want = full["Total Loss"] - 3.0 * full["FluidRegionLoss"] - 1.5 * full["RockRegionLoss"]
    assert abs(less["Total Loss"] - want) <= 1e-5 * abs(want)
    want = full["Total Loss"] - 30.0 * full["RockRegionLoss"]
    assert abs(none["Total Loss"] - want) <= 1e-5 * abs(want)
