"""CPU checks of the training loss: the float64 yardstick (tests/loss_f64.py) against the reference's own SynthesisLoss
(tests/golden/losses_vs_reference.npz, float64 too: both make the same discrete decisions, so they agree to rounding), its
decision-argument gradient against float64 autograd, and the host-side checks of slr_sfs_amd.losses that need no device."""
import types

import numpy as np
import pytest
import torch

import loss_f64 as L64
import losses_fixture as LF

REL = 1e-12


@pytest.fixture(scope="module")
def sd():
    return LF.vgg19_state_dict()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/losses_vs_reference.npz")


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_f64_definition_equals_the_reference(sd, golden):
    N, _, H, W = LF.GOLDEN_SHAPE
    pred, gt = LF.image_pair(N, H, W)
    p = pred.double().requires_grad_(True)
    out = L64.synthesis_loss(p, gt.double(), sd, LF.LOSSES)
    out["Total Loss"].backward()
    assert sorted(k for k in out if k != "distances") == list(golden["keys"])
    for k in golden["keys"]:
        e = _rel(out[k].detach().numpy(), golden[k.replace(" ", "_")])
        print(k, float(out[k].detach()), e)
        assert e <= REL, (k, e)
    assert _rel(out["distances"].numpy(), golden["distances"]) <= REL
    e = _rel(p.grad.numpy(), golden["grad"])
    print("grad", e)
    assert e <= REL


@pytest.mark.parametrize("shape", [(2, 3, 32, 48), (1, 3, 21, 19)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_decision_form_equals_autograd(sd, shape, scale):
    """gradient_from_decisions with float64's own gates, signs and routes IS float64 autograd's gradient (21 x 19: odd sizes at the pools)."""
    pred, gt = LF.image_pair(shape[0], shape[2], shape[3], tag="decisions")
    grad, _, _, ap, ag = L64.perceptual_gradient(pred, gt, sd, torch.float64, scale)
    gates, signs, routes = L64.decisions(ap, [ag[k] for k in L64.SLICE_ENDS])
    got = L64.gradient_from_decisions(sd, gates, signs, routes, scale)
    e = _rel(got.numpy(), grad.numpy())
    print(shape, scale, e)
    assert e <= REL


def test_flipping_a_decision_changes_the_gradient(sd):
    """The decision form really uses its arguments: one flipped relu5_1 sign moves the gradient by far more than rounding."""
    pred, gt = LF.image_pair(1, 16, 16, tag="flip")
    grad, _, _, ap, ag = L64.perceptual_gradient(pred, gt, sd)
    gates, signs, routes = L64.decisions(ap, [ag[k] for k in L64.SLICE_ENDS])
    at = int(torch.nonzero(gates[12].flatten() & (signs[4].flatten() != 0))[0])
    signs[4].view(-1)[at] *= -1
    got = L64.gradient_from_decisions(sd, gates, signs, routes)
    assert _rel(got.numpy(), grad.numpy()) > 1e-6


# ---------------------------------------------------------------- host checks of slr_sfs_amd.losses (no device)

def test_cpu_tensors_raise():
    import slr_sfs_amd as S
    x = torch.zeros(1, 3, 16, 16)
    vgg = S.losses.VGG19Features()
    opt = types.SimpleNamespace(losses=["1.0_l1", "10.0_content"])
    for fn in (S.losses.L1LossWrapper(), S.losses.PerceptualLoss(vgg), S.losses.PSNR(), S.losses.SSIM(), S.losses.SynthesisLoss(opt, vgg)):
        with pytest.raises(NotImplementedError):
            fn(x, x)


def test_style_and_unknown_losses_raise():
    import slr_sfs_amd as S
    with pytest.raises(NotImplementedError, match="style"):
        S.losses.SynthesisLoss(types.SimpleNamespace(losses=["1.0_l1", "1.0_style"]), S.losses.VGG19Features())
    with pytest.raises(ValueError, match="gan"):
        S.losses.SynthesisLoss(types.SimpleNamespace(losses=["1.0_gan"]))
    with pytest.raises(ValueError, match="VGG19Features"):
        S.losses.SynthesisLoss(types.SimpleNamespace(losses=["1.0_content"]))
    with pytest.raises(TypeError):
        S.losses.PerceptualLoss(None)


def test_synthesis_loss_has_the_reference_modules_and_lambdas():
    import slr_sfs_amd as S
    loss = S.SynthesisLoss(types.SimpleNamespace(losses=["1.0_l1", "10.0_content"]), S.VGG19Features(), subname="_x")
    assert [type(m).__name__ for m in loss.losses] == ["L1LossWrapper", "PerceptualLoss", "PSNR", "SSIM"]
    assert loss.lambdas == [1.0, 10.0] and all(m.subname == "_x" for m in loss.losses)
    assert loss.losses[1].weights == [1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0]


def test_state_dict_loader(sd):
    import slr_sfs_amd as S
    net = S.load_vgg19_state_dict(S.VGG19Features(), dict(sd, **{"classifier.0.weight": torch.zeros(2), "features.30.weight": torch.zeros(2),
                                                                 "features.34.bias": torch.zeros(2)}))
    assert S.losses.VGG19_CONVS == LF.VGG19_CONVS == L64.CONVS
    for k, idx in enumerate(LF.VGG19_CONVS):
        w = sd[f"features.{idx}.weight"]
        assert torch.equal(net.convs[k].weight, w) and torch.equal(net.convs[k].bias, sd[f"features.{idx}.bias"])
        assert torch.equal(net.bwd[k].weight, w.flip(2, 3).transpose(0, 1)) and net.bwd[k].bias is None
        assert not net.convs[k].weight.requires_grad and not net.bwd[k].weight.requires_grad
    with torch.no_grad():                                # an in-place update of a forward weight reaches its backward convolution
        net.convs[3].weight.mul_(2.0)
    assert torch.equal(net.backward_conv(3).weight, (2.0 * sd["features.7.weight"]).flip(2, 3).transpose(0, 1))
    missing = {k: v for k, v in sd.items() if k != "features.16.bias"}
    with pytest.raises(KeyError, match="features.16.bias"):
        S.load_vgg19_state_dict(S.VGG19Features(), missing)
    with pytest.raises(ValueError, match="features.5.weight"):
        S.load_vgg19_state_dict(S.VGG19Features(), dict(sd, **{"features.5.weight": torch.zeros(128, 64, 1, 1)}))
    for extra in ("features.3.weight", "features.29.weight", "avgpool.weight"):
        with pytest.raises(ValueError, match="unexpected"):
            S.load_vgg19_state_dict(S.VGG19Features(), dict(sd, **{extra: torch.zeros(1)}))


def test_small_images_raise():
    import slr_sfs_amd as S
    vgg = S.VGG19Features()
    for H, W in ((15, 64), (64, 15), (8, 8)):
        with pytest.raises(ValueError, match="16"):
            vgg.check_input(H, W)
    vgg.check_input(16, 16)


def test_loss_entry_points_refuse_bad_arguments():
    """csrc/loss.hip: argument checks return -1 and name the argument before anything touches a device (dummy pointers), and the
    workspace size is the documented one."""
    import slr_sfs_amd as S
    L = S._lib.lib()
    P = 0x10000
    assert L.slr_loss_ws_bytes(2, 3, 37, 51) == ((2 * 3 * 37 * 51 + 1023) // 1024) * 8 and L.slr_loss_ws_bytes(0, 3, 8, 8) == 0

    def refused(rc, *words):
        msg = L.slr_last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    refused(L.slr_l1_loss_grad(P, P, None, None, 1.0, P, 1, 3, 8, 8, P, 8, None), b"slr_l1_loss_grad", b"null")
    refused(L.slr_l1_loss_grad(P, P, None, P, 1.0, None, 1, 3, 8, 8, P, 8, None), b"slr_l1_loss_grad", b"gscale")
    refused(L.slr_l1_loss_grad(P, P, P, None, 1.0, None, 1, 0, 8, 8, P, 8, None), b"slr_l1_loss_grad", b"sizes")
    refused(L.slr_l1_loss_grad(P, P, P, None, 1.0, None, 1, 3, 8, 8, P, 0, None), b"slr_l1_loss_grad", b"ws")
    refused(L.slr_l1_loss_grad(P, P, P, None, 1.0, None, 1, 3, 8, 8, P + 4, 8, None), b"slr_l1_loss_grad", b"ws")
    refused(L.slr_feature_l1_gate_b8(P, P, None, None, None, 1.0, P, 1, 8, 8, 8, P, 8, None), b"slr_feature_l1_gate_b8", b"null")
    refused(L.slr_feature_l1_gate_b8(P, None, P, P, None, 1.0, P, 1, 8, 8, 8, P, 8, None), b"slr_feature_l1_gate_b8", b"needs b")
    refused(L.slr_feature_l1_gate_b8(P, None, None, None, P, 1.0, P, 1, 8, 8, 8, P, 8, None), b"slr_feature_l1_gate_b8", b"g_in")
    refused(L.slr_feature_l1_gate_b8(P, P, None, None, P, 1.0, None, 1, 8, 8, 8, P, 8, None), b"slr_feature_l1_gate_b8", b"gscale")
    refused(L.slr_feature_l1_gate_b8(P + 8, P, None, None, P, 1.0, P, 1, 8, 8, 8, P, 8, None), b"slr_feature_l1_gate_b8", b"16-byte")
    refused(L.slr_feature_l1_gate_b8(P, P, None, None, P, 1.0, P, 1, 12, 8, 8, P, 8, None), b"slr_feature_l1_gate_b8", b"C % 8")
    refused(L.slr_feature_l1_gate_b8(P, P, None, P, None, 1.0, P, 1, 8, 8, 8, P, 0, None), b"slr_feature_l1_gate_b8", b"ws")
    refused(L.slr_relu_maxpool2x2_backward_b8(P, P, None, 1, 8, 8, 8, None), b"slr_relu_maxpool2x2_backward_b8", b"null")
    refused(L.slr_relu_maxpool2x2_backward_b8(P, P + 8, P, 1, 8, 8, 8, None), b"slr_relu_maxpool2x2_backward_b8", b"16-byte")
    refused(L.slr_relu_maxpool2x2_backward_b8(P, P, P, 1, 12, 8, 8, None), b"slr_relu_maxpool2x2_backward_b8", b"C % 8")
    refused(L.slr_relu_maxpool2x2_backward_b8(P, P, P, 1, 8, 1, 8, None), b"slr_relu_maxpool2x2_backward_b8", b"H, W >= 2")
