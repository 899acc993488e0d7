"""tests/disc_f64.py (the adversarial loss written out without autograd) against float64 torch autograd of the same operators (1e-12) and
against the reference's own DiscriminatorLoss in float64 (tests/golden/disc_vs_reference.npz, made by tools/make_golden_disc.py; 1e-10);
the state-dict names and the u / v bookkeeping of the new classes; the host-side argument checks of csrc/disc.hip.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_f64 as D64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disc_vs_reference.npz")
CASES = {"d16": (2, 16, 16), "d21": (2, 21, 19)}
NDF = 8


def E(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("shape", [(1, 3, 8, 5, 7, 2), (2, 3, 6, 9, 4, 1), (2, 5, 4, 1, 1, 2), (1, 4, 1, 6, 6, 1), (2, 2, 3, 8, 8, 2)])
def test_convolution_against_autograd(shape):
    N, cin, cout, H, W, s = shape
    x, w, b = rnd(N, cin, H, W, seed=1).requires_grad_(), rnd(cout, cin, 4, 4, seed=2).requires_grad_(), rnd(cout, seed=3).requires_grad_()
    y = F.conv2d(x, w, b, stride=s, padding=2)
    assert tuple(y.shape[2:]) == (D64.out_size(H, s), D64.out_size(W, s))
    g = rnd(*y.shape, seed=4)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), g)
    xd, wd = x.detach(), w.detach()
    dw, db = D64.conv_weight_grad(xd, g, s)
    for name, got, ref in (("forward", D64.conv_forward(xd, wd, b.detach(), s), y.detach()), ("backward-data", D64.conv_backward_data(g, wd, s, H, W), gx),
                           ("weight-gradient", dw, gw), ("bias-gradient", db, gb)):
        assert E(got, ref) <= 1e-12, (name, E(got, ref))


@pytest.mark.parametrize("shape", [(1, 8, 2, 2), (2, 5, 7, 4), (2, 3, 9, 9)])
def test_instance_norm_against_autograd(shape):
    x = rnd(*shape, seed=5).requires_grad_()
    y = F.leaky_relu(F.instance_norm(x, eps=1e-5), 0.2)
    g = rnd(*shape, seed=6)
    gx, = torch.autograd.grad(y, x, g)
    got, xh, rstd = D64.instnorm_lrelu_forward(x.detach())
    assert E(got, y.detach()) <= 1e-12 and E(D64.instnorm_lrelu_backward(g, xh, rstd), gx) <= 1e-12
    xn = D64.nudged(torch.zeros(1, 2, 4, 4).float() + torch.arange(16.0).view(1, 1, 4, 4) - 7.5)
    assert D64.instnorm_margin(xn) >= 1e-4


def test_spectral_norm_against_torch():
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(6, 10, 4, 2, 2, bias=False)).double().train()
    w, u, v = conv.weight_orig.detach().clone(), conv.weight_u.clone(), conv.weight_v.clone()
    x, g = rnd(2, 6, 7, 5, seed=7), None
    for _ in range(2):                                   # two forwards: u and v move twice
        y = conv(x)
        u, v = D64.sn_power_iteration(w, u, v)
        assert E(u, conv.weight_u) <= 1e-12 and E(v, conv.weight_v) <= 1e-12
    g = rnd(*y.shape, seed=8)
    ref, = torch.autograd.grad(y, conv.weight_orig, g)
    W = w / D64.sn_sigma(w, u, v)
    assert E(D64.conv_forward(x, W, None, 2), y.detach()) <= 1e-12
    assert E(D64.sn_weight_grad(D64.conv_weight_grad(x, g, 2)[0], w, u, v), ref) <= 1e-12
    conv.eval()
    conv(x)
    assert torch.equal(conv.weight_u, u.to(conv.weight_u.dtype)) or E(u, conv.weight_u) <= 1e-12


@pytest.mark.parametrize("hw", [(16, 16), (21, 19), (1, 5), (2, 2)])
def test_counted_average_pool_against_autograd(hw):
    x = rnd(2, 3, *hw, seed=9).requires_grad_()
    y = F.avg_pool2d(x, 3, stride=2, padding=[1, 1], count_include_pad=False)
    g = rnd(*y.shape, seed=10)
    gx, = torch.autograd.grad(y, x, g)
    assert E(D64.avgpool_forward(x.detach()), y.detach()) <= 1e-12 and E(D64.avgpool_backward(g, *hw), gx) <= 1e-12


def autograd_features(P, x):
    """MultiscaleDiscriminator.forward from torch's own operators, u and v taken as they are (constants)."""
    feats = []
    for d in range(2):
        p = f"discriminator_{d}."
        f = [F.leaky_relu(F.conv2d(x, P[p + "model0.0.weight"], P[p + "model0.0.bias"], stride=2, padding=2), 0.2)]
        for j in (1, 2, 3):
            k = p + f"model{j}.0.0.weight"
            W = P[k + "_orig"] / D64.sn_sigma(P[k + "_orig"], P[k + "_u"], P[k + "_v"])
            f.append(F.leaky_relu(F.instance_norm(F.conv2d(f[-1], W, None, stride=D64.STRIDES[j], padding=2), eps=1e-5), 0.2))
        f.append(F.conv2d(f[-1], P[p + "model4.0.weight"], P[p + "model4.0.bias"], stride=1, padding=2))
        feats.append(f)
        x = F.avg_pool2d(x, 3, stride=2, padding=[1, 1], count_include_pad=False)
    return feats


@pytest.mark.parametrize("case", sorted(CASES))
def test_both_steps_against_autograd(case):
    N, H, W = CASES[case]
    P = D64.fixture_state(case, NDF)
    fake, real = D64.fixture_param(case, "fake", (N, 3, H, W)).double(), D64.fixture_param(case, "real", (N, 3, H, W)).double()
    losses, terms, grads, P2 = D64.generator_step(P, fake, real)
    leaves = {k: v.clone().requires_grad_() for k, v in P2.items() if not k.endswith(("_u", "_v"))}
    fk = fake.clone().requires_grad_()
    feats = autograd_features({**P2, **leaves}, torch.cat([fk, real]))
    gan = sum(-f[4][:N].mean() for f in feats) / 2
    feat = sum(F.l1_loss(f[j][:N], f[j][N:].detach()) * 10.0 / 2 for f in feats for j in range(4))
    assert E(losses["GAN"], gan.detach()) <= 1e-12 and E(losses["GAN_Feat"], feat.detach()) <= 1e-12
    assert losses["GAN"].shape == (1,) and losses["GAN_Feat"].shape == (1,) and losses["Total Loss"].shape == ()
    ref = torch.autograd.grad(gan + feat, [fk] + list(leaves.values()))
    for k, r in zip(["fake"] + list(leaves), ref):
        assert E(grads[k], r) <= 1e-12, (k, E(grads[k], r))
    dl, dgrads, P3 = D64.discriminator_step(P2, fake, real)
    leaves = {k: v.clone().requires_grad_() for k, v in P3.items() if not k.endswith(("_u", "_v"))}
    feats = autograd_features({**P3, **leaves}, torch.cat([fake, real]))
    dfake = sum(-torch.clamp_max(-f[4][:N] - 1, 0).mean() for f in feats) / 2
    dreal = sum(-torch.clamp_max(f[4][N:] - 1, 0).mean() for f in feats) / 2
    assert E(dl["D_Fake"], dfake.detach()) <= 1e-12 and E(dl["D_real"], dreal.detach()) <= 1e-12
    ref = torch.autograd.grad(dfake + dreal, list(leaves.values()))
    for k, r in zip(leaves, ref):
        assert E(dgrads[k], r) <= 1e-12, (k, E(dgrads[k], r))


@pytest.fixture(scope="module")
def golden():
    return D64.load_packed(GOLDEN)


def _against(golden, prefix, got):
    n = 0
    for k, ref in golden.items():
        if not k.startswith(prefix):
            continue
        name = k[len(prefix):]
        g = got[name[:-2]].reshape(-1)[::7] if name.endswith("@7") else got[name].reshape(ref.shape)
        assert E(g, ref) <= 1e-10, (k, E(g, ref))
        n += 1
    return n


@pytest.mark.parametrize("case", sorted(CASES))
def test_both_steps_against_the_reference(golden, case):
    """The reference's DiscriminatorLoss in float64: losses, gradients and u / v after the first and after the second forward."""
    assert os.path.getsize(GOLDEN) < 1 << 20
    N, H, W = CASES[case]
    P = D64.fixture_state(case, NDF)
    fake, real = D64.fixture_param(case, "fake", (N, 3, H, W)).double(), D64.fixture_param(case, "real", (N, 3, H, W)).double()
    losses, _, grads, P2 = D64.generator_step(P, fake, real)
    assert _against(golden, f"{case}/g/loss/", losses) == 3
    assert _against(golden, f"{case}/g/grad/", grads) == 1 + 14
    assert _against(golden, f"{case}/g/state/", P2) == 12
    dl, dgrads, P3 = D64.discriminator_step(P2, fake, real)
    assert _against(golden, f"{case}/d/loss/", dl) == 3
    assert _against(golden, f"{case}/d/grad/", dgrads) == 14
    assert _against(golden, f"{case}/d/state/", P3) == 12       # two forwards in train() mode: u and v moved twice
    _, _, P4 = D64.discriminator_step(P3, fake, real, training=False, with_grads=False)
    assert all(torch.equal(P4[k], P3[k]) for k in P3)           # eval(): no iteration


def test_new_classes_carry_the_reference_names_and_move_u_v(golden):
    """State-dict keys of DiscriminatorLoss = the reference's 26, a state dict of that form loads, and the spectral layers' u / v after two
    train() scales equal the reference's after two forwards; eval() leaves them alone.  (float64 on the CPU: the power iteration and
    sigma are torch operators; the convolutions are not run.)"""
    import slr_sfs_amd as S
    case = "d16"
    loss = S.DiscriminatorLoss(ndf=NDF)
    keys = [str(k) for k in golden[f"{case}/keys"]]
    assert list(loss.state_dict().keys()) == keys and len(keys) == 26
    assert ["netD.netD." + k for k in D64.param_shapes(NDF)] == keys
    loss.load_state_dict({"netD.netD." + k: v for k, v in D64.fixture_state(case, NDF, torch.float32).items()})
    loss = loss.double().train()
    layers = [m for m in loss.modules() if isinstance(m, S.adversarial._SpectralConv4x4)]
    assert len(layers) == 6
    scales = [[m.scale() for m in layers] for _ in range(2)]
    state = loss.state_dict()
    for k in keys:
        if k.endswith(("_u", "_v")):
            ref = golden[f"{case}/d/state/" + k[len("netD.netD."):]]
            assert E(state[k], ref) <= 1e-10, k
    P = {k[len("netD.netD."):]: v for k, v in state.items()}
    for m, sc, k in zip(layers, scales[1], [k for k in P if k.endswith("weight_orig")]):
        assert sc.shape == (1,) and E(1.0 / sc.detach(), D64.sn_sigma(P[k], P[k[:-5] + "_u"], P[k[:-5] + "_v"]).reshape(1)) <= 1e-12
    # the gradient through 1 / sigma is the second term of (dW - <dW, W> u v^T) / sigma
    m = layers[0]
    w, u, v = m.weight_orig.detach(), m.weight_u.clone(), m.weight_v.clone()
    loss.eval()
    dW = rnd(*w.shape, seed=11)
    sc = m.scale()
    assert torch.equal(m.weight_u, u) and torch.equal(m.weight_v, v)
    (sc * (dW * m.weight_orig).sum().detach()).sum().backward()
    total = dW * sc.detach() + m.weight_orig.grad
    assert E(total, D64.sn_weight_grad(dW, w, u, v)) <= 1e-12


def test_operators_refuse_cpu_tensors():
    import slr_sfs_amd as S
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        S.conv4x4(z(1, 3, 8, 8), z(4, 3, 4, 4), stride=2)
    with pytest.raises(NotImplementedError):
        S.instnorm_lrelu(z(1, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        S.DiscriminatorLoss(ndf=8).run_generator_one_step(z(1, 3, 16, 16), z(1, 3, 16, 16))


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def test_discriminator_entry_points_refuse_bad_arguments(L):
    """Every argument check of csrc/disc.hip returns the library's error code and names the argument before anything touches a device
    (the pointers are dummy integers), and the size functions give the documented formulas."""
    P = 0x10000                                              # a 256-byte aligned non-null "pointer"
    al = lambda n: (n + 255) & ~255

    def refused(rc, *words, code=-1):
        msg = L.slr_last_error()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    # prepared weights: ceil(produced channels / 32) * summed channels * 512 floats
    assert L.slr_conv4x4_weight_bytes(128, 64, 0) == 4 * 64 * 2048 and L.slr_conv4x4_weight_bytes(128, 64, 1) == 2 * 128 * 2048
    assert L.slr_conv4x4_weight_bytes(1, 3, 0) == 3 * 2048 and L.slr_conv4x4_weight_bytes(1, 3, 1) == 2048
    assert L.slr_conv4x4_weight_bytes(0, 3, 0) == 0 and L.slr_conv4x4_weight_bytes(3, -1, 1) == 0
    # weight-gradient workspace: S slabs of 16 Cout Cin floats; chunks = N * OH * ceil(OW / 32), tiles of 32 x 32 channels
    assert L.slr_conv4x4_grad_ws_bytes(2, 8, 16, 9, 11, 1, 3) == al(3 * 16 * 16 * 8 * 4)
    assert L.slr_conv4x4_grad_ws_bytes(1, 8, 8, 1, 1, 2, 3) == al(1 * 16 * 8 * 8 * 4)            # one chunk: at most one slab per chunk
    assert L.slr_conv4x4_grad_ws_bytes(4, 64, 128, 129, 129, 2, 0) == al(64 * 16 * 128 * 64 * 4)     # ceil(512 / 8) slabs; 780 chunks
    assert L.slr_conv4x4_grad_ws_bytes(4, 256, 512, 33, 33, 1, 0) == al(4 * 16 * 512 * 256 * 4)      # 512 / 128 tiles = 4 = 32 MiB / 8 MiB
    assert L.slr_conv4x4_grad_ws_bytes(4, 512, 512, 33, 33, 1, 0) == al(2 * 16 * 512 * 512 * 4)      # the 32 MiB cap: 2 slabs
    assert L.slr_conv4x4_grad_ws_bytes(4, 64, 128, 129, 129, 3, 0) == 0 and L.slr_conv4x4_grad_ws_bytes(0, 64, 128, 9, 9, 1, 0) == 0
    assert L.slr_conv4x4_grad_ws_bytes(1, 8, 8, 9, 9, 1, -1) == 0

    for stride in (0, 3, -1, 4):
        refused(L.slr_conv4x4_f32_weights(P, None, P, 8, 8, stride, 0, None), b"slr_conv4x4_f32_weights", b"stride")
        refused(L.slr_conv4x4_forward(P, P, None, P, 1, 8, 8, 9, 9, stride, 0, 0.2, None), b"slr_conv4x4_forward", b"stride")
        refused(L.slr_conv4x4_backward_data(P, None, P, P, 1, 8, 8, 9, 9, stride, 0.2, None), b"slr_conv4x4_backward_data", b"stride")
        refused(L.slr_conv4x4_weight_grad(P, P, None, P, None, 1, 8, 8, 9, 9, stride, 0.2, 0, P, 1 << 20, None), b"slr_conv4x4_weight_grad", b"stride")
    refused(L.slr_conv4x4_f32_weights(None, None, P, 8, 8, 1, 0, None), b"null")
    refused(L.slr_conv4x4_f32_weights(P, None, None, 8, 8, 1, 0, None), b"null")
    refused(L.slr_conv4x4_f32_weights(P, P + 2, P, 8, 8, 1, 0, None), b"aligned")
    refused(L.slr_conv4x4_f32_weights(P, None, P, 0, 8, 1, 0, None), b"sizes")
    for args in ((None, P, None, P), (P, None, None, P), (P, P, None, None)):
        refused(L.slr_conv4x4_forward(*args, 1, 8, 8, 9, 9, 1, 0, 0.2, None), b"slr_conv4x4_forward", b"null")
    refused(L.slr_conv4x4_forward(P, P, None, P, 1, 8, 8, 0, 9, 1, 0, 0.2, None), b"sizes")
    refused(L.slr_conv4x4_forward(P, P, None, P, 65536, 8, 8, 9, 9, 1, 0, 0.2, None), b"sizes")
    refused(L.slr_conv4x4_forward(P, P, P + 1, P, 1, 8, 8, 9, 9, 1, 0, 0.2, None), b"aligned")
    for args in ((None, None, P, P), (P, None, None, P), (P, None, P, None)):
        refused(L.slr_conv4x4_backward_data(*args, 1, 8, 8, 9, 9, 2, 0.2, None), b"slr_conv4x4_backward_data", b"null")
    refused(L.slr_conv4x4_backward_data(P, None, P, P, 1, 0, 8, 9, 9, 2, 0.2, None), b"sizes")
    need = L.slr_conv4x4_grad_ws_bytes(1, 8, 8, 9, 9, 1, 0)

    def wg(x=P, g=P, dw=P, ws=P, ws_bytes=need, splits=0, N=1):
        return L.slr_conv4x4_weight_grad(x, g, None, dw, None, N, 8, 8, 9, 9, 1, 0.2, splits, ws, ws_bytes, None)

    for name in ("x", "g", "dw"):
        refused(wg(**{name: None}), b"slr_conv4x4_weight_grad", b"null")
    refused(wg(splits=-1), b"splits")
    refused(wg(N=0), b"sizes")
    refused(wg(ws=None), b"slr_conv4x4_weight_grad", b"ws", code=-2)
    refused(wg(ws=P + 128), b"ws", b"aligned", code=-2)
    refused(wg(ws_bytes=need - 1), b"ws", code=-2)
    refused(wg(ws_bytes=L.slr_conv4x4_grad_ws_bytes(1, 8, 8, 9, 9, 1, 3)), b"ws", code=-2)       # (3 slabs' worth for the 10 of splits = 0)
    for args in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        refused(L.slr_instnorm_lrelu_forward(*args, 1, 8, 4, 4, 1e-5, 0.2, None), b"slr_instnorm_lrelu_forward", b"null")
    refused(L.slr_instnorm_lrelu_forward(P, P, P, P, 1, 8, 1, 3, 1e-5, 0.2, None), b"sizes")
    refused(L.slr_instnorm_lrelu_forward(P, P, P, P, 0, 8, 4, 4, 1e-5, 0.2, None), b"sizes")
    for args in ((None, P, P, P, P), (P, None, P, P, P), (P, P, None, P, P), (P, P, P, None, P), (P, P, P, P, None)):
        refused(L.slr_instnorm_lrelu_backward(*args, 1, 8, 4, 4, 0.2, None), b"slr_instnorm_lrelu_backward", b"null")
    refused(L.slr_instnorm_lrelu_backward(P, P, P, P, P + 2, 1, 8, 4, 4, 0.2, None), b"aligned")
