"""The training loss on the device (slr_sfs_amd.losses, csrc/loss.hip) against the float64 definition of tests/loss_f64.py.

Criterion (tests/test_gpu_splat_blend.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the
same definition evaluated by torch in float32 on the CPU against float64, computed in the test from the test's inputs and never from the
kernels.  What is elementwise (the gate / seed kernel's gradient, the pooling backward, the L1 gradient) must be BIT-equal to the
float32 expression.  The end-to-end gradient is discontinuous in the features (tests/loss_f64.py), so it is held to float64 evaluated at
the DEVICE's own discrete decisions, after checking that those agree with float64's wherever float64's margin is clear.  Every test
prints its figures (run with -s)."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_f64 as L64
import losses_fixture as LF
from metrics_fixture import from_blocked, to_blocked
from nets_fixture import _rng

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = ((2, 3, 16, 16), (2, 3, 32, 48), (2, 3, 37, 51))                 # 37 x 51: odd pooled sizes at two levels (18 x 25 -> 9 x 12)
_id = lambda s: "x".join(map(str, s))                                     # noqa: E731


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


@functools.lru_cache(maxsize=None)
def _sd():
    return LF.vgg19_state_dict()


@pytest.fixture(scope="module")
def vgg(S):
    return S.load_vgg19_state_dict(S.VGG19Features(), _sd()).to(DEV)


def E(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max())


def bound(e_plain):
    return 10.0 * e_plain + 1e-6


def held(name, got, ref64, plain32):
    e_gpu, e_plain = E(got, ref64), E(plain32, ref64)
    print(f"{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    assert e_gpu <= bound(e_plain), (name, e_gpu, e_plain)
    return e_gpu


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """Float64 and float32 CPU runs of the definition for the seeded pair of ``shape``, computed once and shared: per dtype
    (gradient, loss, distances, activations of pred, activations of gt)."""
    pred, gt = LF.image_pair(shape[0], shape[2], shape[3], tag="gpu")
    return pred, gt, L64.perceptual_gradient(pred, gt, _sd(), torch.float64), L64.perceptual_gradient(pred, gt, _sd(), torch.float32)


# ------------------------------------------------------------------ 1. gate / seed kernel

def _gate_inputs(C, H, W, N=2):
    """Features on the grid of multiples of 1/8: a exactly 0, negative and positive, b equal to a or at least 1/8 away."""
    r = _rng("losses", "gate", C, H, W)
    a = torch.from_numpy(r.integers(-16, 17, (N, C, H, W)).astype(np.float32) / 8)
    a.view(-1)[::7] = 0.0
    delta = torch.from_numpy(r.integers(-8, 9, (N, C, H, W)).astype(np.float32) / 8)
    delta.view(-1)[::3] = 0.0
    g = torch.from_numpy(r.standard_normal((N, C, H, W)).astype(np.float32))
    return a, a + delta, g


@pytest.mark.parametrize("hw", [(5, 7), (9, 13)], ids=_id)
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("with_b,with_g", [(True, False), (True, True), (False, True)], ids=["seed", "seed+g_in", "relu"])
def test_gate_kernel(S, C, hw, with_b, with_g):
    """(Without b and without g_in there is nothing to gate: the entry point refuses that, tests/test_losses_f64.py.)"""
    a, b, g = _gate_inputs(C, *hw)
    assert ((a - b).abs() >= 1e-3).logical_or(a == b).all() and (a == 0).any() and (a < 0).any() and (a > 0).any() and (a == b).any()
    coef, gscale = 0.37 / a.numel(), torch.tensor([1.7], dtype=torch.float32)
    dev = lambda t: to_blocked(t).to(DEV)                                 # noqa: E731
    out = torch.full(a.shape, float("nan"), device=DEV)
    total = torch.full((1,), float("nan"), device=DEV) if with_b else None
    ws = S.losses._sum_ws(out, *a.shape) if with_b else None
    S.losses._gate(dev(a), dev(b) if with_b else None, dev(g) if with_g else None, total, out, coef, gscale.to(DEV), ws)
    gi = g if with_g else torch.zeros_like(a)
    if with_b:
        d = torch.relu(a) - torch.relu(b)
        want = torch.where(a > 0, gi + torch.sign(d) * (torch.tensor(coef, dtype=torch.float32) * gscale), torch.zeros(()))
    else:
        want = torch.where(a > 0, gi, torch.zeros(()))
    assert torch.equal(from_blocked(out.cpu()), want)
    if with_b:
        d64 = (torch.relu(a.double()) - torch.relu(b.double())).abs().sum()
        held("sum", total.cpu()[0], d64, d.abs().sum())


# ------------------------------------------------------------------ 2. pooling backward

@pytest.mark.parametrize("hw", [(5, 7), (8, 12)], ids=_id)
@pytest.mark.parametrize("C", [8, 16])
def test_pool_backward_is_torchs(S, C, hw):
    H, W = hw
    r = _rng("losses", "pool", C, H, W)
    x = torch.from_numpy(r.integers(-2, 3, (2, C, H, W)).astype(np.float32) / 2)     # five levels: ties in most windows
    x[0, :, 0:2, 0:2] = -1.0                                                  # an all-negative window (tie of negatives)
    x[0, :, 0:2, 2:4] = 0.5                                                   # a positive tie of all four
    x[1, :, 2:4, 0:2] = torch.tensor([[-1.0, 0.0], [0.0, -0.5]])              # maximum exactly 0
    x[1, :, 2:4, 2:4] = torch.tensor([[-1.0, 1.0], [1.0, 0.5]])               # positive tie of the second and third
    g = torch.from_numpy(r.standard_normal((2, C, H // 2, W // 2)).astype(np.float32))
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(torch.relu(xr), 2, 2).backward(g)
    out = torch.full(x.shape, float("nan"), device=DEV)
    S._lib.call("slr_relu_maxpool2x2_backward_b8", out.device, to_blocked(x).to(DEV), to_blocked(g).to(DEV), out, *x.shape)
    assert torch.equal(from_blocked(out.cpu()), xr.grad)


# ------------------------------------------------------------------ 3. L1 + gradient

@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "4-byte-aligned"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 37, 51)], ids=_id)
def test_l1_loss_and_gradient(S, shape, offset):
    pred, gt = LF.image_pair(shape[0], shape[2], shape[3], tag="l1")
    pred.view(-1)[::5] = gt.view(-1)[::5]                                     # equal elements: gradient exactly 0
    n = pred.numel()

    def dev(t):                                                               # (offset 1: a contiguous tensor that is only 4-byte aligned)
        return torch.empty(n + offset, device=DEV)[offset:].view(shape).copy_(t)
    p = dev(pred).requires_grad_(True)
    loss = S.losses.l1_loss(p, dev(gt))
    (3.0 * loss).backward()
    d = pred - gt
    want = torch.sign(d) * (torch.tensor(1.0 / n, dtype=torch.float32) * torch.tensor(3.0, dtype=torch.float32))
    assert torch.equal(p.grad.cpu(), want) and bool((p.grad.view(-1)[::5] == 0).all())
    held("L1", loss, (pred.double() - gt.double()).abs().mean(), d.abs().mean())


# ------------------------------------------------------------------ 4. backward-data convolution

@pytest.mark.parametrize("nhw", [(2, 9, 13), (1, 8, 12)], ids=_id)
@pytest.mark.parametrize("k", [0, 2, 5, 9], ids=["3<-64", "64<-128", "256<-256", "512<-512"])
def test_backward_data_convolution(S, vgg, k, nhw):
    """The gradient at a convolution's input from the one at its output, on the forward kernels with flipped, transposed weights,
    against float64 conv_transpose2d.  Linear: nothing can flip."""
    N, H, W = nhw
    w = _sd()[f"features.{L64.CONVS[k]}.weight"]
    cout, cin = w.shape[:2]
    assert (cin, cout) == {0: (3, 64), 2: (64, 128), 5: (256, 256), 9: (512, 512)}[k]
    g = torch.from_numpy(_rng("losses", "bwd", k, N, H, W).standard_normal((N, cout, H, W)).astype(np.float32))
    with S.nets.fp32_kernels(winograd=False), torch.no_grad():
        out = vgg.backward_conv(k).conv(to_blocked(g).to(DEV), None, None, layout=S.nets.IN_B8 | (S.nets.OUT_B8 if k else 0))
    assert tuple(out.shape) == (N, cin, H, W)
    out = out.cpu() if k == 0 else from_blocked(out.cpu())
    held(f"conv {k}", out, F.conv_transpose2d(g.double(), w.double(), padding=1), F.conv_transpose2d(g, w, padding=1))


# ------------------------------------------------------------------ 5. forward

def _device_forward(S, vgg, shape):
    pred, gt = _reference(shape)[:2]
    with torch.no_grad():
        dists, acts = S.losses._perceptual_forward(vgg, pred.to(DEV), gt.to(DEV), True)
    return dists.cpu(), [from_blocked(a.cpu()) for a in acts]


def _ref_act(r, k):
    """What the device keeps of activation k: prediction and ground truth of a slice end, the prediction alone otherwise."""
    return torch.cat([r[3][k], r[4][k]]) if k in L64.SLICE_ENDS else r[3][k]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_forward_vs_float64(S, vgg, shape):
    pred, gt, r64, r32 = _reference(shape)
    N = shape[0]
    dists, acts = _device_forward(S, vgg, shape)
    assert len(acts) == 13
    worst = 0.0
    for k in range(13):
        ref = lambda r: _ref_act(r, k)                                    # noqa: E731
        assert acts[k].shape == ref(r64).shape
        worst = max(worst, held(f"activation {k}", acts[k], ref(r64), ref(r32)))
    for s in range(5):
        worst = max(worst, held(f"distance {s}", dists[s], r64[2][s], r32[2][s]))
    loss = S.losses.perceptual_loss(vgg, pred.to(DEV), gt.to(DEV))
    assert not loss.requires_grad and loss.dim() == 0
    worst = max(worst, held("Perceptual", loss, r64[1], r32[1]))
    l1 = S.L1LossWrapper()(pred.to(DEV), gt.to(DEV))["L1"]
    worst = max(worst, held("L1", l1, L64.l1(pred, gt), L64.l1(pred, gt, torch.float32)))
    print(f"forward {shape}: worst E_gpu {worst:.3e}")


# ------------------------------------------------------------------ 6. gradient end to end, flip-proof

def _device_gradient(S, vgg, shape, scale):
    pred, gt = _reference(shape)[:2]
    p = pred.to(DEV).requires_grad_(True)
    loss = S.losses.perceptual_loss(vgg, p, gt.to(DEV))
    assert loss.requires_grad
    (loss if scale == 1.0 else scale * loss).backward()
    return p.grad.cpu()


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_gradient_vs_float64_at_the_devices_decisions(S, vgg, shape):
    pred, gt, r64, r32 = _reference(shape)
    N = shape[0]
    _, acts = _device_forward(S, vgg, shape)
    dev_pred, dev_gt = [a[:N].double() for a in acts], [acts[k][N:].double() for k in L64.SLICE_ENDS]
    # the error bound of item 5 per activation tensor, absolute: (10 E_plain32 + 1e-6) max|a64|; a decision counts where float64's margin is 10x that
    thr = []
    for k in range(13):
        ref64, ref32 = _ref_act(r64, k), _ref_act(r32, k)
        thr.append(10.0 * bound(E(ref32, ref64)) * float(ref64.abs().max()))
    ends64 = [r64[4][k] for k in L64.SLICE_ENDS]
    dec_dev, dec_64, mar_64 = L64.decisions(dev_pred, dev_gt), L64.decisions(r64[3], ends64), L64.margins(r64[3], ends64)
    tensor_of = (list(range(13)), list(L64.SLICE_ENDS), [k - 1 for k in L64.POOLS])      # the activation a decision is read from
    matters = L64.sign_matters(r64[3])                                        # (a sign acts through its open gate only, loss_f64.margins)
    unclear = total = 0
    for kind, name in enumerate(("gate", "sign", "route")):
        for j, (d_dev, d_64, m) in enumerate(zip(dec_dev[kind], dec_64[kind], mar_64[kind])):
            clear = m > thr[tensor_of[kind][j]]
            differ = (d_dev != d_64) & matters[j] if name == "sign" else d_dev != d_64
            wrong = int((differ & clear).sum())
            assert wrong == 0, f"{name} {j}: {wrong} decisions differ from float64's at a clear margin"
            unclear += int((~clear).sum())
            total += clear.numel()
    share = unclear / total
    print(f"gradient {shape}: {unclear} of {total} decisions below the margin ({100 * share:.4f} %)")
    assert share <= 1e-3
    worst = 0.0
    for scale in (1.0, 3.0):
        want64 = L64.gradient_from_decisions(_sd(), *dec_dev, scale, torch.float64)
        plain32 = L64.gradient_from_decisions(_sd(), *dec_dev, scale, torch.float32)
        got = _device_gradient(S, vgg, shape, scale)
        worst = max(worst, held(f"gradient x{scale:g}", got, want64, plain32))
        assert torch.equal(got, _device_gradient(S, vgg, shape, scale)), "two runs differ"
    print(f"gradient {shape}: worst E_gpu {worst:.3e}; against float64's own decisions: E {E(_device_gradient(S, vgg, shape, 1.0), r64[0]):.3e}")


# ------------------------------------------------------------------ 7. SynthesisLoss

def test_synthesis_loss_vs_reference(S, vgg, golden_dir, monkeypatch):
    golden = np.load(f"{golden_dir}/losses_vs_reference.npz")
    N, _, H, W = LF.GOLDEN_SHAPE
    pred, gt = LF.image_pair(N, H, W)
    plain = L64.synthesis_loss(pred, gt, _sd(), LF.LOSSES, torch.float32)
    fn = S.SynthesisLoss(types.SimpleNamespace(losses=list(LF.LOSSES)), vgg).to(DEV)
    kept = []
    real = S.losses._perceptual_forward
    monkeypatch.setattr(S.losses, "_perceptual_forward", lambda v, p, g, every: kept.append(every) or real(v, p, g, every))
    p, g = pred.to(DEV).requires_grad_(True), gt.to(DEV)
    fn(p, g)["Total Loss"].backward()                                         # (weights prepared, library loaded)
    p.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = fn(p, g)
        out["Total Loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sorted(out) == list(golden["keys"]) and kept == [True, True]
    for k in golden["keys"]:
        assert out[k].dim() == 0 and out[k].requires_grad == (k in ("L1", "Perceptual", "Total Loss"))
        held(k, out[k], golden[k.replace(" ", "_")], plain[k])
    assert p.grad.shape == pred.shape and bool(torch.isfinite(p.grad).all())
    # the L1 term's share of the gradient is exact: Total Loss = L1 + 10 Perceptual
    p2 = pred.to(DEV).requires_grad_(True)
    S.losses.perceptual_loss(vgg, p2, g).backward(torch.tensor(10.0, device=DEV))
    want_l1 = torch.sign(pred - gt) * (torch.tensor(1.0 / pred.numel(), dtype=torch.float32) * torch.tensor(1.0))
    assert torch.equal(p.grad, want_l1.to(DEV) + p2.grad)
    # a prediction that needs no gradient: nothing is saved, nothing can be back-propagated
    del kept[:]
    out = fn(pred.to(DEV), g)
    assert kept == [False] and not out["Total Loss"].requires_grad and out["Total Loss"].grad_fn is None
    held("Total Loss (no grad)", out["Total Loss"], golden["Total_Loss"], plain["Total Loss"])


def test_bad_inputs_raise_before_the_device_is_touched(S, vgg):
    x = torch.zeros(1, 3, 16, 16, device=DEV)
    fn = S.PerceptualLoss(vgg)
    with pytest.raises(ValueError, match="16"):
        fn(torch.zeros(1, 3, 15, 32, device=DEV), torch.zeros(1, 3, 15, 32, device=DEV))
    with pytest.raises(TypeError):
        fn(x.double(), x.double())
    with pytest.raises(ValueError):
        fn(x, torch.zeros(1, 3, 16, 32, device=DEV))
    with pytest.raises(ValueError):
        fn(x[0], x[0])
    with pytest.raises(ValueError, match="contiguous"):
        S.L1LossWrapper()(x.permute(0, 1, 3, 2), x.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="RGB"):
        fn(torch.zeros(1, 4, 16, 16, device=DEV), torch.zeros(1, 4, 16, 16, device=DEV))
    with pytest.raises(NotImplementedError):
        fn(x, x.cpu())
