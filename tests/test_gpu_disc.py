"""The adversarial loss on the device (slr_sfs_amd.adversarial, csrc/disc.hip) against the float64 definitions of tests/disc_f64.py.

Criterion (tests/test_gpu_conv_train.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the
same written-out definition evaluated by torch in float32 on the CPU against float64, computed in the test from the test's inputs and
never from the kernels.  Every result must have the same bits in two runs.  Every test prints its figures (run with -s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import disc_f64 as D64

pytestmark = pytest.mark.gpu

DEV = "cuda"
# N, Cin, Cout, H, W, stride: odd sizes, both parities at stride 2, channel counts off 32 and 64, Cout = 1, a one-pixel image
CONV_SHAPES = ((1, 3, 8, 5, 7, 2), (2, 3, 64, 33, 20, 2), (2, 40, 72, 33, 20, 1), (4, 64, 128, 37, 51, 2), (1, 128, 256, 16, 24, 1),
               (2, 72, 1, 9, 11, 1), (1, 8, 8, 1, 1, 2))
NORM_SHAPES = ((1, 8, 2, 2), (2, 24, 33, 20), (4, 130, 5, 4), (2, 16, 65, 65))
WHOLE = {"d16": (2, 16, 16), "d21": (2, 21, 19)}
NDF = 8
_id = lambda s: "x".join(map(str, s))                                     # noqa: E731


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


class _no_sync:
    """Inside: anything that synchronises the host with the device raises."""

    def __enter__(self):
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


# ------------------------------------------------------------------ 1. the convolutions alone

@functools.lru_cache(maxsize=None)
def _conv_case(shape):
    """Seeded float32 inputs and the written-out definition in float64 and float32, computed once.  Dense normal values: the border rows
    and columns are non-zero, which is where a wrong halo shows."""
    N, cin, cout, H, W, s = shape
    gen = torch.Generator().manual_seed(cin * 1000 + cout * 10 + H)
    r = lambda *sh: torch.randn(*sh, generator=gen)                        # noqa: E731
    OH, OW = D64.out_size(H, s), D64.out_size(W, s)
    x, w, b, g = r(N, cin, H, W), r(cout, cin, 4, 4) / (4.0 * cin ** 0.5), r(cout), r(N, cout, OH, OW)
    g = g * (1.0 + torch.arange(OW) / OW)                                   # (an incoming gradient that is not constant in any direction)

    def ref(dt):
        a = lambda t: t.to(dt)                                             # noqa: E731
        dw, db = D64.conv_weight_grad(a(x), a(g), s)
        return dict(out=D64.conv_forward(a(x), a(w), a(b), s), out0=D64.conv_forward(a(x), a(w), None, s),
                    dx=D64.conv_backward_data(a(g), a(w), s, H, W), dw=dw, db=db)
    return dict(x=x, w=w, b=b, g=g, r64=ref(torch.float64), r32=ref(torch.float32))


def _run_conv(S, c, s, bias, splits, leaky=False):
    x, w = c["x"].to(DEV).requires_grad_(), c["w"].to(DEV).requires_grad_()
    b = c["b"].to(DEV).requires_grad_() if bias else None
    out = S.conv4x4(x, w, b, stride=s, leaky=leaky, _splits=splits)
    out.backward(c["g"].to(DEV))
    return out.detach(), x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_id)
def test_convolution_forward_backward_data_weight_gradient(S, shape):
    s = shape[5]
    c = _conv_case(shape)
    r64, r32 = c["r64"], c["r32"]
    seen = {}
    for bias in (True, False):
        for splits in (0, 1, 3):
            out, dx, dw, db = _run_conv(S, c, s, bias, splits)
            tag = f"bias {int(bias)} splits {splits}"
            held(f"out {tag}", out, r64["out" if bias else "out0"], r32["out" if bias else "out0"])
            held(f"dx {tag}", dx, r64["dx"], r32["dx"])
            held(f"dw {tag}", dw, r64["dw"], r32["dw"])
            if bias:
                held(f"db {tag}", db, r64["db"], r32["db"])
            again = _run_conv(S, c, s, bias, splits)
            for a, b2 in zip((out, dx, dw, db), again):
                assert (a is None and b2 is None) or torch.equal(a, b2), tag
            # the split changes the weight gradient's order of addition only; nothing else depends on it or on the bias
            first = seen.setdefault("dx", dx)
            assert torch.equal(dx, first), tag
            if bias:
                assert torch.equal(db, seen.setdefault("db", db)), tag


# The launch rule of csrc/conv4x4.hip (c4_launch) takes 2 or 4 tiles of 32 produced channels per workgroup once the launch has 512
# workgroups; the shapes above are all below that.  One cheap shape per mode and tile count: the forward produces Cout, the backward-data
# Cin; the pixel tiles are those of the output (forward), of the input (stride-1 backward) or of its largest parity class (stride 2).
PATH_SHAPES = {(1, 8, 128, 128, 128, 1): ("forward", 4), (1, 8, 64, 128, 128, 1): ("forward", 2), (1, 128, 8, 128, 128, 1): ("backward", 4),
               (1, 64, 8, 128, 128, 1): ("backward", 2), (1, 8, 128, 254, 254, 2): ("forward", 4), (1, 8, 64, 254, 254, 2): ("forward", 2),
               (1, 128, 8, 128, 128, 2): ("backward", 4), (1, 64, 8, 128, 128, 2): ("backward", 2)}


def _channel_tiles_per_workgroup(shape, direction):
    N, cin, cout, H, W, s = shape
    if direction == "forward":
        produced, pixels, classes = cout, N * D64.out_size(H, s) * D64.out_size(W, s), 1
    else:
        produced, pixels, classes = (cin, N * H * W, 1) if s == 1 else (cin, N * ((H + 1) // 2) * ((W + 1) // 2), 4)
    ntile, ptiles = (produced + 31) // 32, (pixels + 31) // 32
    ct = 4 if ntile % 4 == 0 else 2 if ntile % 2 == 0 else 1
    return 1 if ptiles * classes * (ntile // ct) < 512 else ct


@pytest.mark.parametrize("shape", sorted(PATH_SHAPES), ids=_id)
def test_convolution_with_several_channel_tiles_per_workgroup(S, shape):
    direction, ct = PATH_SHAPES[shape]
    assert _channel_tiles_per_workgroup(shape, direction) == ct
    assert all(_channel_tiles_per_workgroup(sh, d) == 1 for sh in CONV_SHAPES for d in ("forward", "backward"))
    c = _conv_case(shape)
    out, dx, dw, db = _run_conv(S, c, shape[5], True, 0)
    for name, got in (("out", out), ("dx", dx), ("dw", dw), ("db", db)):
        held(name, got, c["r64"][name], c["r32"][name])
    again = _run_conv(S, c, shape[5], True, 0)
    assert all(torch.equal(a, b) for a, b in zip((out, dx, dw, db), again))


def test_fused_leaky_relu_is_the_unfused_output_gated(S):
    """model0: LeakyReLU(0.2) of the output inside the kernel is bit-equal to leaky_relu of the unfused output."""
    shape = (2, 3, 64, 33, 20, 2)
    c = _conv_case(shape)
    x, w, b = c["x"].to(DEV), c["w"].to(DEV), c["b"].to(DEV)
    plain = S.conv4x4(x, w, b, stride=2)
    fused = S.conv4x4(x, w, b, stride=2, leaky=True)
    assert torch.equal(fused, F.leaky_relu(plain, 0.2)) and bool((plain < 0).any()) and bool((plain > 0).any())


# ------------------------------------------------------------------ 2. instance norm + LeakyReLU

@functools.lru_cache(maxsize=None)
def _norm_case(shape):
    gen = torch.Generator().manual_seed(shape[1] * 100 + shape[2])
    x = D64.nudged(torch.randn(*shape, generator=gen) * 1.5 + 0.3)
    g = torch.randn(*shape, generator=gen)

    def ref(dt):
        y, xh, rstd = D64.instnorm_lrelu_forward(x.to(dt))
        return dict(y=y, gx=D64.instnorm_lrelu_backward(g.to(dt), xh, rstd))
    return dict(x=x, g=g, r64=ref(torch.float64), r32=ref(torch.float32))


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=_id)
def test_instance_norm_lrelu(S, shape):
    c = _norm_case(shape)
    margin = D64.instnorm_margin(c["x"])
    print(f"gate margin {margin:.3e}")
    assert margin >= 1e-4

    def run():
        x = c["x"].to(DEV).requires_grad_()
        y = S.instnorm_lrelu(x)
        y.backward(c["g"].to(DEV))
        return y.detach(), x.grad
    y, gx = run()
    held("y", y, c["r64"]["y"], c["r32"]["y"])
    held("gx", gx, c["r64"]["gx"], c["r32"]["gx"])
    y2, gx2 = run()
    assert torch.equal(y, y2) and torch.equal(gx, gx2)


# ------------------------------------------------------------------ 3. the spectral weight

@pytest.mark.parametrize("shape", [(16, 8, 4, 4), (128, 64, 4, 4)], ids=_id)
def test_spectral_weight(S, shape):
    cout, cin = shape[:2]
    w = D64.fixture_param("sn", "model1.0.0.weight_orig", shape)
    u0, v0 = D64.fixture_param("sn", "weight_u", (cout,)), D64.fixture_param("sn", "weight_v", (cin * 16,))
    x, g = D64.fixture_param("sn", "x", (2, cin, 9, 7)), D64.fixture_param("sn", "g", (2, cout, 5, 4))

    def ref(dt):
        wd, u, v = w.to(dt), u0.to(dt), v0.to(dt)
        for _ in range(2):
            u, v = D64.sn_power_iteration(wd, u, v)
        sigma = D64.sn_sigma(wd, u, v)
        dW, _ = D64.conv_weight_grad(x.to(dt), g.to(dt), 2)
        return dict(u=u, v=v, inv=(1.0 / sigma).reshape(1), out=D64.conv_forward(x.to(dt), wd / sigma, None, 2), gw=D64.sn_weight_grad(dW, wd, u, v))
    r64, r32 = ref(torch.float64), ref(torch.float32)

    def run():
        wd, u, v = w.to(DEV).requires_grad_(), u0.to(DEV), v0.to(DEV)
        S.spectral_weight(wd, u, v, True)
        inv = S.spectral_weight(wd, u, v, True)          # two forwards: u and v move twice
        out = S.conv4x4(x.to(DEV), wd, None, stride=2, weight_scale=inv)
        out.backward(g.to(DEV))
        u_eval, v_eval = u.clone(), v.clone()
        inv_eval = S.spectral_weight(wd, u_eval, v_eval, False)
        assert torch.equal(u_eval, u) and torch.equal(v_eval, v) and torch.equal(inv_eval, inv)
        return dict(u=u, v=v, inv=inv.detach(), out=out.detach(), gw=wd.grad)
    got = run()
    for k in ("u", "v", "inv", "out", "gw"):
        held(k, got[k], r64[k], r32[k])
    again = run()
    assert all(torch.equal(got[k], again[k]) for k in got)


# ------------------------------------------------------------------ 4. the wholes

@functools.lru_cache(maxsize=None)
def _whole_case(case):
    N, H, W = WHOLE[case]
    seed, P, fake, real = D64.first_clean_seed(case, NDF, N, H, W)
    margin = D64.gate_margin(P, fake, real)
    print(f"{case}: seed {seed}, gate margin {margin:.3e}")
    assert seed < 1000 and margin >= 1e-4

    def ref(dt, lr=0.05):
        Pd, fk, rl = {k: v.to(dt) for k, v in P.items()}, fake.to(dt), real.to(dt)
        gl, _, gg, P2 = D64.generator_step(Pd, fk, rl)
        dl, dg, P3 = D64.discriminator_step(P2, fk, rl)
        P4 = {k: (v - lr * dg[k] if k in dg else v) for k, v in P3.items()}       # one hand-made SGD step on the discriminator
        gl2, _, _, P5 = D64.generator_step(P4, fk, rl, with_grads=False)
        dl2, _, P6 = D64.discriminator_step(P5, fk, rl, with_grads=False)
        out = {f"g/{k}": v for k, v in gl.items()}
        out.update({f"g/grad/{k}": v for k, v in gg.items()})
        out.update({f"d/{k}": v.reshape(-1) for k, v in dl.items()})
        out.update({f"d/grad/{k}": v for k, v in dg.items()})
        out.update({f"uv/{k}": v for k, v in P3.items() if k.endswith(("_u", "_v"))})
        out.update({f"g2/{k}": v for k, v in gl2.items()})
        out.update({f"d2/{k}": v.reshape(-1) for k, v in dl2.items()})
        return out
    return dict(P=P, fake=fake, real=real, r64=ref(torch.float64), r32=ref(torch.float32))


def _run_whole(S, c, lr=0.05, no_sync=False):
    loss = S.DiscriminatorLoss(ndf=NDF)
    loss.load_state_dict({"netD.netD." + k: v for k, v in c["P"].items()})
    loss = loss.to(DEV).train()
    params = {k[len("netD.netD."):]: p for k, p in loss.named_parameters()}
    fake, real = c["fake"].to(DEV).requires_grad_(), c["real"].to(DEV)
    out = {}
    torch.cuda.synchronize()
    guard = _no_sync() if no_sync else torch.enable_grad()
    with guard:
        gl = loss.run_generator_one_step(fake, real)
        gl["Total Loss"].backward()
        out.update({f"g/{k}": v.detach() for k, v in gl.items()})
        out["g/grad/fake"] = fake.grad
        for k, p in params.items():
            out[f"g/grad/{k}"] = p.grad
            p.grad = None
        dl = loss.run_discriminator_one_step(fake, real)
        dl["Total Loss"].backward()
        out.update({f"d/{k}": v.detach().reshape(-1) for k, v in dl.items()})
        out.update({f"d/grad/{k}": p.grad for k, p in params.items()})
        out.update({f"uv/{k[len('netD.netD.'):]}": b.clone() for k, b in loss.named_buffers()})
        with torch.no_grad():
            for p in params.values():
                p.sub_(lr * p.grad)
        gl2 = loss.run_generator_one_step(fake, real)
        dl2 = loss.run_discriminator_one_step(fake, real)
        out.update({f"g2/{k}": v.detach() for k, v in gl2.items()})
        out.update({f"d2/{k}": v.detach().reshape(-1) for k, v in dl2.items()})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", sorted(WHOLE))
def test_both_steps_of_the_whole_loss(S, case):
    """Both steps' loss dictionaries, the gradient to the fake image, every parameter gradient, u / v after the two forwards, and the
    losses after one hand-made SGD step on the discriminator."""
    c = _whole_case(case)
    got = _run_whole(S, c)
    assert sorted(got) == sorted(c["r64"]) and len([k for k in got if "/grad/" in k]) == 1 + 14 + 14
    assert got["g/GAN"].shape == (1,) and got["g/GAN_Feat"].shape == (1,) and got["g/Total Loss"].shape == ()
    for k in sorted(got):
        held(k, got[k], c["r64"][k], c["r32"][k])
    again = _run_whole(S, c)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_a_training_step_does_not_synchronise(S):
    c = _whole_case("d16")
    _run_whole(S, c)                                     # (first launches load code objects)
    got = _run_whole(S, c, no_sync=True)
    assert bool(torch.isfinite(got["g/Total Loss"]).all()) and bool(torch.isfinite(got["d2/Total Loss"]).all())
