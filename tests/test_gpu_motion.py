"""The motion U-Nets on the GPU (csrc/motion.hip + the fp32-rung 3x3 convolution): every new kernel against float64 torch, both whole
networks against the reference's outputs (tests/golden/motion_vs_reference.npz), the SPADE net at 768 x 768 against the reference's
float64 digests (tests/golden/motion_768.npz), no torch fallback, and motion prediction through the animators and tools/animate.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import motion_fixture as MF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def _dev(x):
    return x.float().contiguous().cuda()


CONV4_CASES = [  # (N, cin, cout, output H, output W, leaky, bn)
    (1, 3, 32, 96, 96, False, False), (2, 6, 32, 24, 24, False, True), (1, 4, 64, 10, 14, True, False),
    (1, 32, 64, 96, 96, True, True), (2, 32, 256, 6, 6, True, False), (1, 256, 256, 3, 3, True, True),
    (2, 256, 32, 1, 1, True, True), (1, 256, 256, 1, 1, True, False), (1, 6, 256, 10, 14, True, True),
    (2, 3, 64, 3, 3, False, False), (1, 32, 32, 24, 24, True, True), (1, 256, 64, 6, 6, False, True),
]


@pytest.mark.parametrize("n,cin,cout,oh,ow,leaky,bn", CONV4_CASES)
def test_conv4x4s2_vs_fp64(S, n, cin, cout, oh, ow, leaky, bn):
    g = torch.Generator().manual_seed(cin * 1000 + cout + oh)
    x = torch.randn(n, cin, 2 * oh, 2 * ow, generator=g, dtype=torch.float64)
    conv = S.nets.Conv4x4s2(cin, cout)
    conv.weight.data.copy_(torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5)
    conv.bias.data.copy_(torch.randn(cout, generator=g) * 0.1)
    bnm = None
    if bn:
        bnm = S.nets.EvalBN(cout)
        bnm.running_mean.copy_(torch.randn(cout, generator=g) * 0.2)
        bnm.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
        bnm.weight.copy_(1 + 0.1 * torch.randn(cout, generator=g))
        bnm.bias.copy_(0.1 * torch.randn(cout, generator=g))
    conv_d = conv.cuda()
    with torch.no_grad():
        out = conv_d(_dev(x), leaky=0.2 if leaky else None, bn=bnm.cuda() if bn else None).cpu().double()
        xr = F.leaky_relu(x, 0.2) if leaky else x
        ref = F.conv2d(xr, conv.weight.double().cpu(), conv.bias.double().cpu(), stride=2, padding=1)
        if bn:
            ref = F.batch_norm(ref, bnm.running_mean.double().cpu(), bnm.running_var.double().cpu(), bnm.weight.double().cpu(),
                               bnm.bias.double().cpu(), False, 0.0, 1e-5)
    assert out.shape == (n, cout, oh, ow)
    err = (out - ref).abs().max().item()
    assert err <= 2e-6 * max(ref.abs().max().item(), 1.0), err


# The encoder convolution and the discriminator's stride-2 forward are one kernel body (csrc/conv4x4.hip): a zero row on top and a zero
# column on the left turn the pad-1 taps of output o into the pad-2 taps of output o + 1, so the two entry points give the same bits
# wherever their launches take the same CT (tiles of 32 output channels per workgroup) and KW (waves splitting the input channels).
SAME_BITS = {(2, 3, 8, 2, 2): (1, 2), (1, 5, 40, 9, 6): (1, 4), (1, 33, 70, 7, 11): (1, 16), (2, 256, 32, 12, 12): (1, 16),
             (1, 8, 64, 256, 256): (2, 4), (1, 8, 128, 256, 256): (4, 4)}        # (N, Cin, Cout, H, W): (CT, KW)


def _launch_rule(cout, pixels, cin):
    """(CT, KW) of c4_launch in csrc/conv4x4.hip for a forward launch."""
    ntile, ptiles = (cout + 31) // 32, (pixels + 31) // 32
    ct = 4 if ntile % 4 == 0 else 2 if ntile % 2 == 0 else 1
    if ptiles * (ntile // ct) < 512:
        ct = 1
    wgs, kw = ptiles * (ntile // ct), 1
    while kw < 16 // ct and wgs * kw < 2048 and 2 * kw <= cin:
        kw *= 2
    return ct, kw


def _bits(t):
    return t.contiguous().view(torch.int32)


def _both_entry_points(S, shape, leaky=None):
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(cin * 1000 + cout + h)
    x = _dev(torch.randn(n, cin, h, w, generator=g))
    conv = S.nets.Conv4x4s2(cin, cout)
    conv.weight.data.copy_(torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5)
    conv.bias.data.copy_(torch.randn(cout, generator=g) * 0.1)
    conv = conv.cuda()
    oh, ow = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    with torch.no_grad():
        motion = conv(x, leaky=leaky)
        xp = F.pad(x, (1, 0, 1, 0))
        disc = S.conv4x4(xp if leaky is None else F.leaky_relu(xp, leaky), conv.weight, conv.bias, stride=2)[:, :, 1:1 + oh, 1:1 + ow]
    assert motion.shape == disc.shape == (n, cout, oh, ow)
    return conv, x, motion, disc


@pytest.mark.parametrize("shape", sorted(SAME_BITS), ids=lambda s: "x".join(map(str, s)))
def test_conv4x4s2_and_the_discriminator_forward_give_the_same_bits(S, shape):
    n, cin, cout, h, w = shape
    pair = SAME_BITS[shape]
    assert _launch_rule(cout, n * ((h - 2) // 2 + 1) * ((w - 2) // 2 + 1), cin) == pair
    assert _launch_rule(cout, n * ((h + 1) // 2 + 1) * ((w + 1) // 2 + 1), cin) == pair
    conv, x, motion, disc = _both_entry_points(S, shape)
    assert torch.equal(_bits(motion), _bits(disc))
    if shape != (1, 33, 70, 7, 11):
        return
    # the LeakyReLU of the value read is the LeakyReLU of the input
    _, _, motion_leaky, disc_leaky = _both_entry_points(S, shape, leaky=0.2)
    assert torch.equal(_bits(motion_leaky), _bits(disc_leaky)) and not torch.equal(motion_leaky, motion)
    # the affine epilogue is a multiply, then an add, of the plain result
    g = torch.Generator().manual_seed(7)
    bn = S.nets.EvalBN(cout)
    bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.2)
    bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    bn.weight.copy_(1 + 0.1 * torch.randn(cout, generator=g))
    bn.bias.copy_(0.1 * torch.randn(cout, generator=g))
    bn = bn.cuda()
    with torch.no_grad():
        scale, shift = bn.scale_shift()
        fused = conv(x, bn=bn)
        unfused = motion * scale[None, :, None, None] + shift[None, :, None, None]
    assert torch.equal(_bits(fused), _bits(unfused))


@pytest.mark.parametrize("n,c,h,w", [(1, 32, 96, 64), (2, 256, 3, 3), (1, 64, 2, 4), (1, 128, 48, 48)])
def test_instnorm_spade_vs_fp64(S, n, c, h, w):
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 3 + 1
    gb = torch.randn(n, 2 * c, h, w, generator=g, dtype=torch.float64) * 0.3
    out = S.nets.instnorm_spade(_dev(x), _dev(gb)).cpu().double()
    ref = F.instance_norm(x, eps=1e-5) * (1 + gb[:, :c]) + gb[:, c:]
    assert (out - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.parametrize("h,w", [(256, 256), (256, 512), (768, 768)])
def test_resize_segmap_vs_fp64(S, h, w):
    x = MF.motion_input("resize", (1, 6, h, w)).double()
    x[:, 3] = (torch.rand(h, w, generator=torch.Generator().manual_seed(h)) > 0.5).double()     # the mask channel: nearest
    xd = _dev(x)
    with torch.no_grad():
        for k in range(1, 8):
            out = S.nets.resize_segmap(xd, k).cpu().double()
            with S.nets.cpu_reference():
                ref = S.nets.resize_segmap(x, k)
            assert out.shape == ref.shape
            assert (out - ref).abs().max().item() <= 1e-6, k
            assert torch.equal(out[:, 3], ref[:, 3])


@pytest.mark.parametrize("nearest,relu", [(-1, 1), (3, 1), (3, 2), (-1, 0)])
@pytest.mark.parametrize("n,ca,cb,h,w", [(1, 256, 256, 1, 1), (2, 64, 64, 6, 10), (1, 32, 32, 24, 24), (1, 256, 0, 3, 5)])
def test_upsample2x_concat_vs_fp64(S, nearest, relu, n, ca, cb, h, w):
    g = torch.Generator().manual_seed(ca + h * 7 + relu)
    a = torch.randn(n, ca, h, w, generator=g, dtype=torch.float64)
    b = torch.randn(n, cb, h, w, generator=g, dtype=torch.float64) if cb else None
    with torch.no_grad():
        out = S.nets.upsample2x_concat(_dev(a), None if b is None else _dev(b), nearest, relu).cpu().double()
        with S.nets.cpu_reference():
            ref = S.nets.upsample2x_concat(a, b, nearest, relu)
    assert out.shape == ref.shape == (n, ca + cb, 2 * h, 2 * w)
    assert (out - ref).abs().max().item() <= 1e-6
    if nearest == 3:                                         # channel 3 of each source: nearest (exact copies)
        up3 = a[:, 3].float().double().repeat_interleave(2, -1).repeat_interleave(2, -2)
        assert torch.equal(out[:, 3], F.relu(up3) if relu else up3)


def _net(flagset):
    from slr_sfs_amd import nets
    ref = np.load(os.path.join(ROOT, "tests", "golden", "motion_vs_reference.npz"))
    keys = [str(k) for k in ref[f"{flagset}_keys"]]
    sd = {MF.PREFIX + k: v for k, v in MF.state_dict(flagset, keys, ref[f"{flagset}_shapes"]).items()}
    cls, cin = {"unet": ("Unet4Motion", 3), "spade": ("SPADEUnet4MaskMotion", 6)}[flagset]
    return nets.load_motion_state_dict(getattr(nets, cls)(cin), sd, MF.PREFIX).cuda().eval(), ref


@pytest.mark.parametrize("case", ["unet_256", "spade_256", "spade_256x512"])
def test_motion_nets_on_gpu_vs_reference(S, case):
    flagset = MF.CASES[case][0]
    net, ref = _net(flagset)
    out = (net(_dev(MF.motion_input(case))) * float(ref[f"{flagset}_div_flow"])).cpu()
    if f"{case}_out" in ref:
        ra = torch.from_numpy(ref[f"{case}_out"])
        err, scale = (ra - out).abs().max().item(), ra.abs().max().item()
    else:
        flat = out.double()[0].reshape(-1)
        err = float(np.abs(flat[MF.digest_positions(case, flat.numel())].numpy() - ref[f"{case}_samples"]).max())
        scale = float(ref[f"{case}_max_abs"])
    print(f"{case}: max |GPU - reference| = {err:.3e} = {err / scale:.2e} of max|flow| {scale:.3f}")
    assert err <= 1e-4 * scale, (err, scale)


def test_spade_net_768_vs_reference_fp64(S):
    g = np.load(os.path.join(ROOT, "tests", "golden", "motion_768.npz"))
    net, _ = _net("spade")
    out = net(_dev(MF.motion_input("spade_768", (1, 6, 768, 768)))).double().cpu()[0].reshape(-1)
    pos = MF.digest_positions("spade_768", out.numel())
    scale = float(g["f64_max_abs"])
    err = float(np.abs(out[pos].numpy() - g["f64_samples"]).max())
    err32 = float(np.abs(g["f32_samples"] - g["f64_samples"]).max())
    sums = np.abs(out.reshape(2, -1).sum(1).numpy() - g["f64_plane_sums"]).max()
    print(f"768x768 SPADE net: max |GPU - reference fp64| = {err:.3e} = {err / scale:.2e} of max|flow| {scale:.3f} "
          f"(reference fp32 on CPU: {err32 / scale:.2e}); plane sums off by {sums:.3e}")
    assert err <= 1e-4 * scale
    assert abs(out.abs().max().item() - scale) <= 1e-4 * scale


def test_no_torch_fallback(S, monkeypatch):
    net, _ = _net("spade")
    unet, _ = _net("unet")

    def boom(*a, **k):
        raise AssertionError("torch fallback")
    for name in ("conv2d", "interpolate", "instance_norm", "batch_norm"):
        monkeypatch.setattr(F, name, boom)
    x = _dev(MF.motion_input("spade_256"))
    assert torch.isfinite(net(x)).all()
    assert torch.isfinite(unet(x[:, :3].contiguous())).all()


def _regressor(S, flagset):
    ref = np.load(os.path.join(ROOT, "tests", "golden", "motion_vs_reference.npz"))
    keys = [str(k) for k in ref[f"{flagset}_keys"]]
    sd = {S.motion.PREFIX_JOINT + k: v for k, v in MF.state_dict(flagset, keys, ref[f"{flagset}_shapes"]).items()}
    opts = dict(model_type="softmax_splating", motion_model_type={"unet": "unet_motion", "spade": "SPADE_unet_mask_motion"}[flagset],
                norm_G="sync:spectral_batch", motion_norm_G="sync:spectral_instance", div_flow=1.0,
                use_mask_as_motion_input=flagset == "spade", use_hint_as_motion_input=flagset == "spade")
    return S.motion.MotionRegressor(opts, sd).cuda()


def test_forward_flow_without_motions_predicts_them(S):
    torch.manual_seed(0)
    W, N = 256, 6
    inp = MF.motion_input("spade_256")
    image, mask, hint = _dev(inp[:, :3]), _dev(inp[:, 3:4]), _dev(inp[:, 4:6])
    reg = _regressor(S, "spade")
    pred = reg.forward_flow(image, mask, hint)["PredMotion"]
    base = S.pipeline.BaselineAnimator(motion_regressor=reg).cuda().eval()
    fs, Z = base.encoder(image)
    b = {"images": [image], "features": [(fs, Z)], "index": [[0, 2, N - 1]], "motion_mask": mask, "motion_hint": hint}
    assert torch.equal(reg.forward_flow(image, mask, hint)["PredMotion"], pred)          # the prediction is deterministic
    a = base.forward_flow(b)["PredImg"]
    ref = base.forward_flow(dict(b, motions=[pred]))["PredImg"]
    assert (a - ref).abs().max().item() <= 1e-5                      # (the splat's accumulation order is not fixed)
    v1 = S.pipeline.SLRv1Animator(motion_regressor=_regressor(S, "unet")).cuda().eval()
    pred1 = v1.motion_regressor.forward_flow(image)["PredMotion"]
    fs, Z = v1.encoder(image)
    b = {"images": [image], "features": [(fs, Z)], "index": [[0, 3, N - 1]], "BGImg": [v1.net_bg(image)]}
    a = v1.forward_flow(b)
    r = v1.forward_flow(dict(b, motions=[pred1]))
    for k in r:
        assert (a[k] - r[k]).abs().max().item() <= 1e-5, k
    # synthesize(image, None, N) predicts once per clip = synthesize with the predicted field
    d = base.synthesize(image, None, N, motion_mask=mask, motion_hint=hint) - base.synthesize(image, pred, N)
    assert d.abs().max().item() <= 1e-5
    with pytest.raises(ValueError):
        S.pipeline.BaselineAnimator().cuda().synthesize(image, None, N)


def test_animate_cli_with_motion_checkpoint(S, tmp_path):
    from slr_sfs_amd import io
    ref = np.load(os.path.join(ROOT, "tests", "golden", "motion_vs_reference.npz"))
    keys = [str(k) for k in ref["spade_keys"]]
    sd = {S.motion.PREFIX_MOTION + k: v for k, v in MF.state_dict("spade", keys, ref["spade_shapes"]).items()}
    import argparse
    opts = argparse.Namespace(model_type="SPADE_unet_mask_motion", norm_G="sync:spectral_batch", motion_norm_G="sync:spectral_instance",
                              div_flow=1.0, use_mask_as_motion_input=True, use_hint_as_motion_input=True, train_motion=True)
    ckpt = tmp_path / "motion.pth"
    torch.save({"state_dict": sd, "opts": opts}, ckpt)
    H = W = 256
    r = np.random.default_rng(1)
    img = (r.uniform(0, 255, (H, W, 3))).astype(np.uint8)
    io.save_image(torch.from_numpy(img), str(tmp_path / "scene_input.png"))
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    flow = np.stack([np.sin(x / 20) * 2 * (x > 100), np.cos(y / 30) * (x > 100)], -1).astype(np.float32)
    io.write_flo(str(tmp_path / "scene.flo"), flow)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "animate.py"), str(tmp_path / "scene_input.png"), str(tmp_path / "scene.flo"),
           str(tmp_path / "out"), "None", "scene", str(W), "8", "1", "--motion-ckpt", str(ckpt), "--hint-points", "60,150;100,200;128,120;180,220;230,160",
           "--write-motion"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONNOUSERSITE="1"))
    assert res.returncode == 0, res.stderr[-3000:]
    frames = sorted(os.listdir(tmp_path / "out" / "scene" / "PredImg"))
    assert len([f for f in frames if f.endswith(".png")]) == 8
    pred = io.read_flo(str(tmp_path / "out" / "scene" / "Motion.flo"))
    assert pred.shape == (H, W, 2) and np.isfinite(pred).all() and np.abs(pred).max() > 0
