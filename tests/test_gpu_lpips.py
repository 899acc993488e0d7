"""LPIPS (alex, v0.1) on the kernels of csrc/lpips.hip against the written-out definition of tests/lpips_f64.py in float64, with the
seeded weights of tests/lpips_fixture.py: each new kernel alone, the whole metric, the exact cases, the reference's [0, 1] quirk and
evaluate_clip.

The criterion is the project's: E_gpu <= 10 E_plain32 + 1e-6, E the largest error relative to max|.| of the float64 result, E_plain32
the same definition evaluated by torch in float32 on the CPU -- computed here from the test's inputs, never from the kernel.  As a
condition on the inputs (not a measurement) E_plain32 <= 1e-5 is asserted.  Every test prints both figures (run with -s).

Measured on an MI355X (E_gpu | E_plain32): the K x K convolutions 2.5e-7 .. 1.3e-6 | 8.6e-8 .. 7.6e-7 (worst ratio 3.6), the distance
kernel 2.2e-8 .. 3.8e-7 | 4.4e-8 .. 2.4e-7, the score 1.3e-8 .. 4.6e-7 | 1.3e-8 .. 6.3e-7, the worst layer 3.0e-7 .. 2.5e-6 | 9.8e-8 .. 3.4e-6."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_f64 as D
import lpips_fixture as LF
from metrics_fixture import from_blocked, to_blocked
from nets_fixture import _rng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd.metrics


@functools.lru_cache(maxsize=1)
def _weights():
    return LF.alexnet_state_dict(), LF.linear_state_dict()


@pytest.fixture(scope="module")
def net(M):
    return M.load_lpips_state_dicts(M.LPIPSAlex(), *_weights()).cuda()


def _check(tag, got, f64, f32):
    """The criterion for one quantity; prints the figures."""
    e_gpu, e_ref = D.rel_err(got, f64), D.rel_err(f32, f64)
    print(f"[{tag}] E_gpu {e_gpu:.3e}  E_plain32 {e_ref:.3e}  bound {10 * e_ref + 1e-6:.3e}")
    assert e_ref <= 1e-5, (tag, e_ref)
    assert e_gpu <= 10 * e_ref + 1e-6, (tag, e_gpu, e_ref)
    return e_gpu, e_ref


def _randn(*what, shape):
    return torch.from_numpy(_rng("lpips_gpu", *what).standard_normal(shape).astype(np.float32))


# ------------------------------------------------------------------ the K x K convolution

# (K, stride, pad, Cin, in_b8), then (N, H, W, Cout).  11 / 4 / 2: OW = (W - 7) // 4 + 1 -- widths 1, 7, 31, 32, 33, 79 with
# (W + 2 P - K) mod S = 1, 0, 3, 1, 2, 0 and heights with 0, 2, 3, 1, 2, 0; 5 / 1 / 2: OW = W.  Cout 40: a last channel tile of 8.
# The last three: each shape with the other input layout, and a channel count that leaves a last stage of 8 channels.
CONV_CASES = [((11, 4, 2, 3, False), c) for c in [(1, 7, 8, 64), (3, 33, 31, 64), (1, 34, 130, 40), (3, 12, 132, 64), (1, 9, 137, 192),
                                                    (1, 31, 319, 64)]] + \
             [((5, 1, 2, 64, True), c) for c in [(1, 1, 1, 192), (3, 3, 7, 192), (1, 5, 31, 64), (3, 2, 32, 192), (1, 4, 33, 40),
                                                 (1, 3, 79, 192)]] + \
             [((5, 1, 2, 3, False), (3, 6, 33, 64)), ((5, 1, 2, 24, True), (1, 7, 9, 64)), ((11, 4, 2, 8, True), (1, 15, 131, 64))]


@pytest.mark.parametrize("kind,case", CONV_CASES, ids=lambda v: "-".join(str(int(x)) for x in v))
def test_convkxk_vs_fp64(M, kind, case):
    """slr_convkxk_forward (raw output: conv + bias, channel-blocked) against F.conv2d in float64."""
    from slr_sfs_amd import nets
    K, S, P, cin, b8 = kind
    N, H, W, cout = case
    conv = nets.ConvKxK(cin, cout, K, S, P)
    w = _randn("w", K, cin, cout, shape=(cout, cin, K, K)) * (2.0 / (cin * K * K)) ** 0.5
    b = 0.1 * _randn("b", K, cin, cout, shape=(cout,))
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    conv = conv.cuda()
    x = _randn("x", K, cin, N, H, W, shape=(N, cin, H, W))
    f64 = F.conv2d(x.double(), w.double(), b.double(), stride=S, padding=P)
    f32 = F.conv2d(x, w, b, stride=S, padding=P)
    got = from_blocked(conv((to_blocked(x) if b8 else x).cuda(), in_b8=b8).cpu())
    assert got.shape == f64.shape == (N, cout, (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1)
    _check(f"conv {kind} {case}", got, f64, f32)


def test_convkxk_batch_and_rerun_bit_equal(M):
    """An image alone and as the middle one of three: the same bits (pixel tiles are flat over the batch, sums are not); two runs too."""
    from slr_sfs_amd import nets
    conv = nets.ConvKxK(3, 64, 11, 4, 2).cuda()
    x = _randn("batch", shape=(3, 3, 45, 61)).cuda()
    a, b, c = conv(x), conv(x[1:2].contiguous()), conv(x)
    assert torch.equal(a, c) and torch.equal(a[1:2], b)


def test_convkxk_refuses(M):
    from slr_sfs_amd import nets
    with pytest.raises(NotImplementedError):
        nets.ConvKxK(3, 64, 11, 4, 2)(torch.zeros(1, 3, 31, 31))
    with pytest.raises(ValueError):
        nets.ConvKxK(3, 64, 11, 4, 2).cuda()(torch.zeros(1, 3, 6, 31, device="cuda"))       # 6 + 4 < 11: no output row
    with pytest.raises(RuntimeError, match="slr_convkxk"):
        nets.ConvKxK(3, 64, 7, 2, 3).cuda()(torch.zeros(1, 3, 31, 31, device="cuda"))       # not one of the two shapes


# ------------------------------------------------------------------ ReLU + MaxPool2d(3, 2)

@pytest.mark.parametrize("shape", [(1, 8, 3, 3), (2, 64, 7, 7), (1, 192, 8, 10), (3, 16, 21, 39), (1, 8, 4, 3)])
def test_relu_maxpool3x3s2(M, shape):
    """Exact: a max of fp32 values.  Even and odd sizes, 3 x 3 -> 1 x 1; a NaN in a window gives NaN, as torch's max_pool2d does."""
    x = _randn("pool", *shape, shape=shape)
    x[0, 3, 1, 1] = float("nan")
    want = F.max_pool2d(torch.relu(x), 3, 2)
    got = from_blocked(M.relu_maxpool3x3s2(to_blocked(x).cuda()).cpu())
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got[0, 3, 0, 0]))
    assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0))


# ------------------------------------------------------------------ the distance kernel

@pytest.mark.parametrize("C", [64, 192, 384, 256])
@pytest.mark.parametrize("hw", [(1, 1), (23, 15)])
def test_lpips_distance_vs_fp64(M, C, hw):
    """slr_lpips_distance on raw features (negative values: the ReLU is the kernel's), with a negative head weight, and with a third
    of the pixels all-zero after the ReLU in f0, in f1 and in both (the 1e-10 outside the root; 0 / 1e-10 - 0 / 1e-10 = 0, no NaN)."""
    H, W = hw
    N = 4
    f0, f1 = _randn("f0", C, H, W, shape=(N, C, H, W)), _randn("f1", C, H, W, shape=(N, C, H, W))
    dead = torch.zeros(H * W, dtype=torch.bool)
    dead[: max(1, H * W // 3)] = True
    dead = dead.view(1, H, W)
    f0[1, :, dead[0]] = -f0[1, :, dead[0]].abs() - 0.5
    f1[2, :, dead[0]] = -f1[2, :, dead[0]].abs() - 0.5
    f0[3, :, dead[0]] = -f0[3, :, dead[0]].abs() - 0.5
    f1[3, :, dead[0]] = -f1[3, :, dead[0]].abs() - 0.5
    w = 0.05 * _randn("w", C, shape=(C,)).abs()
    w[C // 3] = -0.07
    got = M.lpips_distance(to_blocked(f0).cuda(), to_blocked(f1).cuda(), w.cuda()).cpu()
    assert bool(torch.isfinite(got).all())
    _check(f"distance C={C} {H}x{W}", got, D.layer_distance(f0, f1, w), D.layer_distance(f0, f1, w, torch.float32))
    same = M.lpips_distance(to_blocked(f0).cuda(), to_blocked(f0).cuda(), w.cuda()).cpu()
    assert torch.equal(same, torch.zeros(N))
    if hw == (1, 1):                                                         # image 3: both vectors all zero at the only pixel
        assert float(got[3]) == 0.0


# ------------------------------------------------------------------ the whole metric

@functools.lru_cache(maxsize=None)
def _case(shape, normalize=False, u8=False):
    """(in0, in1, float64 (val, per), float32 (val, per)) of a seeded pair -- computed once, shared, never modified."""
    sd, lin = _weights()
    a, b = LF.image_pair(*shape)
    if u8:
        a, b = ((t * 255).round().byte().permute(0, 2, 3, 1).contiguous() for t in (a, b))
    return a, b, D.lpips(a, b, sd, lin, torch.float64, normalize), D.lpips(a, b, sd, lin, torch.float32, normalize)


def _check_metric(tag, val, per, f64, f32):
    assert val.shape == (f64[0].shape[0], 1, 1, 1) and all(p.shape == val.shape for p in per) and len(per) == 5
    _check(f"{tag} score", val.view(-1), f64[0], f32[0])
    e_gpu = max(D.rel_err(p.view(-1), q) for p, q in zip(per, f64[1]))
    e_ref = max(D.rel_err(p, q) for p, q in zip(f32[1], f64[1]))
    print(f"[{tag} worst layer] E_gpu {e_gpu:.3e}  E_plain32 {e_ref:.3e}  bound {10 * e_ref + 1e-6:.3e}")
    assert e_ref <= 1e-5, (tag, e_ref)
    assert e_gpu <= 10 * e_ref + 1e-6, (tag, e_gpu, e_ref)


@pytest.mark.parametrize("shape", LF.SHAPES + ((1, 3, 180, 320),), ids=lambda s: "x".join(map(str, s)))
def test_lpips_vs_fp64(net, shape):
    """forward(in0, in1, retPerLayer=True): the score and all five layers."""
    a, b, f64, f32 = _case(shape)
    val, per = net(a.cuda(), b.cuda(), retPerLayer=True)
    _check_metric(f"lpips {shape}", val, per, f64, f32)
    assert torch.equal(net(a.cuda(), b.cuda()), val)


def test_lpips_normalize_and_uint8_vs_fp64(M, net):
    a, b, f64, f32 = _case(LF.SHAPES[2], normalize=True)
    val, per = net(a.cuda(), b.cuda(), retPerLayer=True, normalize=True)
    _check_metric("lpips normalize", val, per, f64, f32)
    a, b, f64, f32 = _case(LF.SHAPES[1], u8=True)
    val, per = net.score(a.cuda(), b.cuda(), retPerLayer=True)
    _check_metric("lpips uint8", val.view(-1, 1, 1, 1), [p.view(-1, 1, 1, 1) for p in per], f64, f32)
    assert torch.equal(M.lpips_sim(a.cuda(), b.cuda(), net), val)


def test_lpips_exact_cases(M, net):
    """LPIPS(x, x) == 0 bit for bit; with the first bias at -1e3 every feature of relu1 is zero and both images give the same
    features behind it: the score is exactly 0 and finite; alone or as the middle one of a batch of three: the same bits; two runs too."""
    a, b, _, _ = _case(LF.SHAPES[2])
    a, b = a.cuda(), b.cuda()
    val, per = net(a, a.clone(), retPerLayer=True)
    assert torch.equal(val, torch.zeros_like(val)) and all(torch.equal(p, torch.zeros_like(p)) for p in per)
    sd, lin = _weights()
    sd = dict(sd)
    sd["features.0.bias"] = torch.full_like(sd["features.0.bias"], -1e3)
    dead = M.load_lpips_state_dicts(M.LPIPSAlex(), sd, lin).cuda()
    val, per = dead(a, b, retPerLayer=True)
    assert torch.equal(val, torch.zeros_like(val)) and bool(torch.isfinite(torch.stack(per)).all())
    v3, p3 = net(a, b, retPerLayer=True)
    v1, p1 = net(a[1:2].contiguous(), b[1:2].contiguous(), retPerLayer=True)
    assert torch.equal(v3[1:2], v1) and all(torch.equal(x[1:2], y) for x, y in zip(p3, p1))
    v3b, p3b = net(a, b, retPerLayer=True)
    assert torch.equal(v3, v3b) and all(torch.equal(x, y) for x, y in zip(p3, p3b))


def test_lpips_sim_is_the_quirk(M, net):
    """lpips_sim = forward on the [0, 1] tensors as they are (eval_CLAW.py:37 passes no normalize=True), bit for bit -- and NOT the
    normalize=True value: the two differ by more than 100 x the bound, so this test would notice the wrong one."""
    a, b, f64, f32 = _case(LF.SHAPES[2])
    got = M.lpips_sim(a.cuda(), b.cuda(), net)
    assert got.shape == (a.shape[0],)
    assert torch.equal(got.view(-1, 1, 1, 1), net(a.cuda(), b.cuda()))
    bound = 10 * D.rel_err(f32[0], f64[0]) + 1e-6
    wrong = _case(LF.SHAPES[2], normalize=True)[2][0]
    assert D.rel_err(got, f64[0]) <= bound
    assert D.rel_err(wrong, f64[0]) > 100 * bound and D.rel_err(got, wrong) > 100 * bound


def test_lpips_input_checks(M, net):
    x = torch.zeros(1, 3, 40, 40)
    with pytest.raises(NotImplementedError):
        net(x, x)
    for shape in [(1, 3, 30, 40), (1, 3, 40, 30)]:
        with pytest.raises(ValueError, match="31"):
            net(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    assert M.lpips_batch(720, 1280) == 18 and M.lpips_batch(4000, 6000) == 1


def test_evaluate_clip_with_lpips(M, net):
    """evaluate_clip: "LPIPS" only with lpips=, the other keys unchanged by it, and the same bits per frame whatever the batch."""
    a, b = LF.image_pair(5, 3, 40, 52, tag="clip")
    a, b = ((t * 255).round().byte().permute(0, 2, 3, 1).contiguous().cuda() for t in (a, b))
    plain = M.evaluate_clip(a, b)
    assert list(plain) == ["PSNR", "SSIM"]
    r1, r3, rd = M.evaluate_clip(a, b, lpips=net, batch=1), M.evaluate_clip(a, b, lpips=net, batch=3), M.evaluate_clip(a, b, lpips=net)
    for r in (r1, r3, rd):
        assert list(r) == ["PSNR", "SSIM", "LPIPS"] and r["LPIPS"].shape == (5,)
        assert torch.equal(r["PSNR"], plain["PSNR"]) and torch.equal(r["SSIM"], plain["SSIM"])
        assert torch.equal(r["LPIPS"], r1["LPIPS"])
    assert torch.equal(r1["LPIPS"], M.lpips_sim(a, b, net)) and bool((r1["LPIPS"] > 0).all())


def test_evaluate_tool_writes_lpips(M, tmp_path):
    """tools/evaluate.py with both LPIPS files, plain and --fluid (the composite of eval_CLAW_fluid.py:95-109): metric.json in the
    reference's key order, its LPIPS the float64 definition's on the [0, 1] frames as they are; without the files: no LPIPS key."""
    import json
    import os
    import sys

    from metrics_fixture import fluid_inputs
    from metrics_fixture import image_pair as u8_pair
    from metrics_fixture import to_tensor
    from slr_sfs_amd import evaluation, io
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import evaluate
    finally:
        sys.path.pop(0)
    pred, gt = tmp_path / "out" / "pred", tmp_path / "gt"
    os.makedirs(pred), os.makedirs(gt)
    n, H, W = 3, 40, 56
    a, b = u8_pair(H, W, n=n, tag="lpips_tool")
    io.save_frames(torch.from_numpy(a), str(pred / "sA"))
    np.save(str(gt / "sA.npy"), b)
    flow_hw2, image, _ = fluid_inputs()
    io.write_flo(str(gt / "sA.flo"), flow_hw2)
    io.save_image(torch.from_numpy(image), str(gt / "sA_input.jpg"))
    sd, lin = _weights()
    torch.save(sd, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    files = ["--lpips-alexnet", str(tmp_path / "alexnet.pth"), "--lpips-linear", str(tmp_path / "alex.pth")]
    mask = evaluation.fluid_mask(evaluation.fluid_flow_tensor(str(gt / "sA.flo")), (H, W))
    img = evaluation.load_input_image(str(gt / "sA_input.jpg"), (H, W))
    cases = {"metric.json": ([], to_tensor(a)), "metric_fluid.json": (["--fluid"], evaluation.fluid_composite(torch.from_numpy(a), img, mask))}
    for name, (flags, x) in cases.items():
        got = evaluate.main([str(pred), str(gt), "--frames", str(n)] + flags + files)
        assert got == json.load(open(tmp_path / "out" / name))
        order = ["LPIPS", "PSNR", "SSIM"]
        assert list(got) == [f"Total{k}" for k in order] + [f"Total{k}_std" for k in order] + order + [f"{k}_std" for k in order]
        f64, f32 = (D.lpips(x, to_tensor(b), sd, lin, dt)[0] for dt in (torch.float64, torch.float32))
        tol = (10 * D.rel_err(f32, f64) + 1e-6) * float(f64.abs().max())
        print(f"[tool {name}] LPIPS {got['TotalLPIPS']:.6f}  float64 {float(f64.mean()):.6f}  tol {tol:.2e}")
        assert abs(got["TotalLPIPS"] - float(f64.mean())) <= tol and abs(got["LPIPS"]["sA"] - float(f64.mean())) <= tol
        assert abs(got["TotalLPIPS_std"] - float(np.std(f64.numpy()))) <= 2 * tol
    with_lpips = evaluate.main([str(pred), str(gt), "--frames", str(n)] + files)
    plain = evaluate.main([str(pred), str(gt), "--frames", str(n)])
    assert plain == {k: v for k, v in with_lpips.items() if "LPIPS" not in k} and list(plain)[0] == "TotalPSNR"
