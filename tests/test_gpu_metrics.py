"""The clip-evaluation metrics on the GPU (csrc/metrics.hip + the fp32-rung 3x3 convolution): SSIM / PSNR and the VGG16 Perceptual metric
against the reference's own outputs (tests/golden/metrics_vs_reference.npz) and the float64 restatement of tests/metrics_fixture.py at
full size, determinism and batch independence, the VGG16 loader, tools/evaluate.py end to end and tools/animate.py --gt-frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_fixture as MF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd.metrics


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(f"{golden_dir}/metrics_vs_reference.npz")


@pytest.fixture(scope="module")
def vgg(M):
    return M.load_vgg16_state_dict(M.PerceptualVGG16(), MF.vgg16_state_dict()).cuda()


def _inputs(hw, tag="pair"):
    a_u8, b_u8 = MF.image_pair(*hw, tag=tag)
    return (torch.from_numpy(a_u8).cuda(), torch.from_numpy(b_u8).cuda(), MF.to_tensor(a_u8).cuda(), MF.to_tensor(b_u8).cuda())


@pytest.mark.parametrize("hw", MF.SIZES)
@pytest.mark.parametrize("ws", MF.WINDOWS)
@pytest.mark.parametrize("form", ["float", "uint8"])
def test_ssim_psnr_vs_reference(M, ref, hw, ws, form):
    a_u8, b_u8, a, b = _inputs(hw)
    x, y = (a, b) if form == "float" else (a_u8, b_u8)
    mask = torch.from_numpy(MF.mask_for(*hw)).cuda()
    t = f"{hw[0]}x{hw[1]}_w{ws}"
    got = {"ssim_mean": M.ssim(x, y, ws, None, True), "ssim": M.ssim(x, y, ws, None, False),
           "ssim_mask": M.ssim(x, y, ws, mask, True), "ssim_mask_noavg": M.SSIM(ws, False)(x, y, mask)}
    for k, v in got.items():
        np.testing.assert_allclose(v.cpu().numpy(), ref[f"{t}_{k}"], rtol=0, atol=1e-5, err_msg=k)
    if ws == 11:
        t = f"{hw[0]}x{hw[1]}"
        np.testing.assert_allclose(M.psnr(x, y).cpu().numpy(), ref[f"{t}_psnr"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(M.psnr(x, y, mask).cpu().numpy(), ref[f"{t}_psnr_mask"], rtol=0, atol=1e-4)
        np.testing.assert_array_equal(M.ssim_metric(x, y).cpu().numpy(), got["ssim"].cpu().numpy())


def test_ssim_psnr_720p_vs_fp64_deterministic_and_batch_independent(M):
    H, W = 720, 1280
    a_u8, b_u8 = MF.image_pair(H, W, n=4, tag="720p")
    mask = torch.from_numpy(MF.mask_for(H, W, n=4)).cuda()
    x, y = torch.from_numpy(a_u8).cuda(), torch.from_numpy(b_u8).cuda()
    a, b = MF.to_tensor(a_u8), MF.to_tensor(b_u8)
    for m in (None, mask):
        sm = M.ssim_mse(x, y, 11, m)
        assert torch.equal(sm, M.ssim_mse(x, y, 11, m))                                   # two calls: bit-identical
        assert torch.equal(sm[2:3], M.ssim_mse(x[2:3], y[2:3], 11, None if m is None else m[2:3]))   # alone == inside the batch
        mc = None if m is None else m.cpu()
        np.testing.assert_allclose(sm[:, 0].cpu().numpy(), MF.ssim_f64(a, b, 11, mc, False).numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(M.psnr_from_mse(sm[:, 1]).cpu().numpy(), MF.psnr_f64(a, b, mc).numpy(), rtol=0, atol=1e-4)
    f = M.ssim_mse(a.cuda(), b.cuda())
    np.testing.assert_allclose(f.cpu().numpy(), M.ssim_mse(x, y).cpu().numpy(), rtol=0, atol=1e-7)      # float input == uint8 input


@pytest.mark.parametrize("hw", MF.VGG_SIZES)
def test_perceptual_vs_reference(M, ref, vgg, hw):
    a_u8, b_u8, a, b = _inputs(hw, "vgg")
    t = f"{hw[0]}x{hw[1]}"
    for x, y in ((a, b), (a_u8, b_u8)):
        total, per = vgg.score(x, y, True, retPerLayer=True)
        np.testing.assert_allclose(total.cpu().numpy(), ref[f"{t}_perceptual"], rtol=1e-4)
        np.testing.assert_allclose(torch.stack(per).cpu().numpy(), ref[f"{t}_perceptual_layers"], rtol=1e-4)
    np.testing.assert_allclose(vgg(a * 2 - 1, b * 2 - 1).cpu().numpy(), ref[f"{t}_perceptual"], rtol=1e-4)   # PNet's own input
    p = M.perceptual_sim(a_u8, b_u8, vgg)
    assert torch.equal(p, M.perceptual_sim(a_u8, b_u8, vgg))
    assert torch.equal(p[1:2], M.perceptual_sim(a_u8[1:2], b_u8[1:2], vgg))


def test_perceptual_256x384_vs_fp64(M, vgg):
    a_u8, b_u8 = MF.image_pair(256, 384, n=1, tag="vgg256")
    got, per = vgg.score(torch.from_numpy(a_u8).cuda(), torch.from_numpy(b_u8).cuda(), True, retPerLayer=True)
    assert torch.equal(got, M.perceptual_sim(torch.from_numpy(a_u8).cuda(), torch.from_numpy(b_u8).cuda(), vgg))
    want, want_per = MF.perceptual_f64(MF.to_tensor(a_u8), MF.to_tensor(b_u8), per_layer=True)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4)
    np.testing.assert_allclose(torch.stack(per).cpu().numpy(), torch.stack(want_per).numpy(), rtol=1e-4)      # each slice, not only their sum


def test_relu_maxpool_odd_sizes(M):
    x = torch.randn(2, 16, 45, 81, device="cuda")
    xb = x.view(2, 2, 8, 45, 81).permute(0, 1, 3, 4, 2).contiguous().view(2, 16, 45, 81)          # channel-blocked
    out = M.relu_maxpool2x2(xb)
    assert out.shape == (2, 16, 22, 40)
    want = torch.nn.functional.max_pool2d(torch.relu(x), 2, 2)
    assert torch.equal(out.view(2, 2, 22, 40, 8).permute(0, 1, 4, 2, 3).reshape(2, 16, 22, 40), want)


def test_loader_rejects_missing_and_misshaped_keys(M, tmp_path):
    sd = MF.vgg16_state_dict()
    torch.save(dict(sd, **{"classifier.6.bias": torch.zeros(1000)}), tmp_path / "vgg16.pth")
    net = M.PerceptualVGG16.from_file(str(tmp_path / "vgg16.pth"), "cuda")
    assert torch.equal(net.convs[0].weight.cpu(), sd["features.0.weight"])
    bad = dict(sd)
    del bad["features.26.weight"]
    with pytest.raises(KeyError):
        M.load_vgg16_state_dict(M.PerceptualVGG16(), bad)
    with pytest.raises(ValueError):
        M.load_vgg16_state_dict(M.PerceptualVGG16(), dict(sd, **{"features.2.bias": torch.zeros(65)}))


def _write_scene(pred_dir, gt_dir, name, a_u8, b_u8, gt_form):
    from slr_sfs_amd import io
    io.save_frames(torch.from_numpy(a_u8), os.path.join(pred_dir, name))
    if gt_form == "npy":
        np.save(os.path.join(gt_dir, name + ".npy"), b_u8)
    else:
        io.save_frames(torch.from_numpy(b_u8), os.path.join(gt_dir, name), key="")


def _run_evaluate(args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py")] + args, capture_output=True, text=True,
                         timeout=600, env=dict(os.environ, PYTHONNOUSERSITE="1"))
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout


def test_evaluate_tool_end_to_end(M, tmp_path):
    """Two synthetic scenes (PNG and .npy ground truth), --perceptual-weights with the seeded weights in a file, and --fluid: metric.json
    equals the float64 restatement's numbers."""
    from slr_sfs_amd import evaluation, io
    pred, gt = tmp_path / "out" / "pred", tmp_path / "gt"
    os.makedirs(pred), os.makedirs(gt)
    n, H, W = 4, 48, 64
    scenes = {"sA": MF.image_pair(H, W, n=n, tag="sA"), "sB": MF.image_pair(H, W, n=n, tag="sB")}
    for (name, (a, b)), form in zip(scenes.items(), ("png", "npy")):
        _write_scene(str(pred), str(gt), name, a, b, form)
    torch.save(MF.vgg16_state_dict(), tmp_path / "vgg16.pth")
    _run_evaluate([str(pred), str(gt), "--frames", str(n), "--perceptual-weights", str(tmp_path / "vgg16.pth")])
    got = json.load(open(tmp_path / "out" / "metric.json"))
    feats = MF.vgg16_features(dtype=torch.float64)
    per = {}
    for name, (a, b) in scenes.items():
        x, y = MF.to_tensor(a), MF.to_tensor(b)
        per[name] = {"PSNR": MF.psnr_f64(x, y).tolist(), "SSIM": MF.ssim_f64(x, y, 11, None, False).tolist(),
                     "Perceptual": MF.perceptual_f64(x, y, features=feats).tolist()}
    want = evaluation.aggregate(per)
    assert list(got) == list(want)
    for k, v in want.items():
        tol = 1e-4 if "PSNR" in k else 1e-5 if "SSIM" in k else 1e-4 * max(abs(x) for x in per["sA"]["Perceptual"])
        if isinstance(v, dict):
            for s in v:
                assert abs(got[k][s] - v[s]) <= tol, (k, s, got[k][s], v[s])
        else:
            assert abs(got[k] - v) <= tol, (k, got[k], v)
    # --fluid: mask from NAME.flo, prediction composited over NAME_input.jpg
    flow_hw2, image, _ = MF.fluid_inputs()
    for name in scenes:
        io.write_flo(str(gt / f"{name}.flo"), flow_hw2)
        io.save_image(torch.from_numpy(image), str(gt / f"{name}_input.jpg"))
    _run_evaluate([str(pred), str(gt), "--frames", str(n), "--fluid"])
    got = json.load(open(tmp_path / "out" / "metric_fluid.json"))
    per = {}
    for name, (a, b) in scenes.items():
        mask = evaluation.fluid_mask(evaluation.fluid_flow_tensor(str(gt / f"{name}.flo")), (H, W))
        img = evaluation.load_input_image(str(gt / f"{name}_input.jpg"), (H, W))
        x = evaluation.fluid_composite(torch.from_numpy(a), img, mask)
        y = MF.to_tensor(b)
        per[name] = {"PSNR": MF.psnr_f64(x, y).tolist(), "SSIM": MF.ssim_f64(x, y, 11, None, False).tolist()}
    want = evaluation.aggregate(per, ("PSNR", "SSIM"))
    for k, v in want.items():
        tol = 1e-4 if "PSNR" in k else 1e-5
        vals = v.values() if isinstance(v, dict) else [v]
        gots = got[k].values() if isinstance(v, dict) else [got[k]]
        assert all(abs(p - q) <= tol for p, q in zip(gots, vals)), (k, got[k], v)


def test_animate_gt_frames_matches_evaluate(M, tmp_path):
    """tools/animate.py --gt-frames scores the clip from the uint8 frames it writes: equal to tools/evaluate.py on those PNGs."""
    from slr_sfs_amd import io
    H = W = 64
    n = 6
    r = np.random.default_rng(5)
    io.save_image(torch.from_numpy(r.integers(0, 256, (H, W, 3), dtype=np.uint8)), str(tmp_path / "scene_input.png"))
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    io.write_flo(str(tmp_path / "scene.flo"), np.stack([np.sin(x / 9) * 2, np.cos(y / 7)], -1).astype(np.float32))
    gt = tmp_path / "gt"
    io.save_frames(torch.from_numpy(r.integers(0, 256, (n, H, W, 3), dtype=np.uint8)), str(gt / "scene"), key="")
    out = tmp_path / "out" / "pred"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "animate.py"), str(tmp_path / "scene_input.png"), str(tmp_path / "scene.flo"),
           str(out), "None", "scene", str(W), str(n), "1", "--gt-frames", str(gt / "scene"), "--metrics-json", str(tmp_path / "a.json")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONNOUSERSITE="1"))
    assert res.returncode == 0, res.stderr[-3000:]
    _run_evaluate([str(out), str(gt), "--frames", str(n), "--out", str(tmp_path / "b.json")])
    a, b = json.load(open(tmp_path / "a.json")), json.load(open(tmp_path / "b.json"))
    assert a == b
