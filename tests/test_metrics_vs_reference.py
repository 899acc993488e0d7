"""CPU checks of the clip-evaluation metrics: the float64 restatement of tests/metrics_fixture.py (the GPU tests' large-size yardstick)
reproduces every value the reference's own ssim.py / metrics.py / PNet("vgg") computed into tests/golden/metrics_vs_reference.npz
(tools/make_golden_metrics.py); metric.json aggregation; the fluid mask and composite of eval_CLAW_fluid.py; CPU tensors raise."""
import numpy as np
import pytest
import torch

import metrics_fixture as MF


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(f"{golden_dir}/metrics_vs_reference.npz")


@pytest.mark.parametrize("hw", MF.SIZES)
@pytest.mark.parametrize("ws", MF.WINDOWS)
def test_ssim_psnr_restatement_vs_reference(ref, hw, ws):
    H, W = hw
    a_u8, b_u8 = MF.image_pair(H, W)
    a, b = MF.to_tensor(a_u8), MF.to_tensor(b_u8)
    mask = torch.from_numpy(MF.mask_for(H, W))
    t = f"{H}x{W}"
    got = {"ssim_mean": MF.ssim_f64(a, b, ws, None, True), "ssim": MF.ssim_f64(a, b, ws, None, False),
           "ssim_mask": MF.ssim_f64(a, b, ws, mask, True), "ssim_mask_noavg": MF.ssim_f64(a, b, ws, mask, False)}
    # bounds: the reference's own fp32 error -- measured up to 7.3e-6 in SSIM (its fp32 grouped convolutions, E[x^2] - mu^2) and 2e-6 dB
    for k, v in got.items():
        np.testing.assert_allclose(v.numpy(), ref[f"{t}_w{ws}_{k}"], rtol=0, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(MF.psnr_f64(a, b).numpy(), ref[f"{t}_psnr"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(MF.psnr_f64(a, b, mask).numpy(), ref[f"{t}_psnr_mask"], rtol=0, atol=5e-6)


def test_perceptual_restatement_vs_reference(ref):
    feats = MF.vgg16_features(dtype=torch.float64)
    for H, W in MF.VGG_SIZES:
        a_u8, b_u8 = MF.image_pair(H, W, tag="vgg")
        total, per = MF.perceptual_f64(MF.to_tensor(a_u8), MF.to_tensor(b_u8), per_layer=True, features=feats)
        np.testing.assert_allclose(total.numpy(), ref[f"{H}x{W}_perceptual"], rtol=1e-5)
        np.testing.assert_allclose(torch.stack(per).numpy(), ref[f"{H}x{W}_perceptual_layers"], rtol=1e-5, atol=2e-7)


def test_fluid_mask_and_composite(ref):
    from slr_sfs_amd import evaluation
    flow_hw2, image, pred = MF.fluid_inputs()
    hw = MF.FLUID["pred_hw"]
    mask = evaluation.fluid_mask(torch.from_numpy(flow_hw2).unsqueeze(0), hw)
    np.testing.assert_array_equal(mask.numpy(), ref["fluid_mask"])
    from PIL import Image
    import tempfile, os
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "scene_input.png")
        Image.fromarray(image).save(p)
        img = evaluation.load_input_image(p, hw)
    comp = evaluation.fluid_composite(torch.from_numpy(pred), img, mask)
    np.testing.assert_allclose(comp[0].numpy(), ref["fluid_composite"], rtol=0, atol=1e-7)


def test_fluid_flow_tensor_reads_flo_as_the_reference(tmp_path):
    from slr_sfs_amd import evaluation, io
    flow_hw2, _, _ = MF.fluid_inputs()
    io.write_flo(str(tmp_path / "s.flo"), flow_hw2)
    t = evaluation.fluid_flow_tensor(str(tmp_path / "s.flo"))
    assert tuple(t.shape) == (1,) + flow_hw2.shape                     # [1,h,w,2], as eval_CLAW_fluid.py:90 builds it
    np.testing.assert_array_equal(t[0].numpy(), flow_hw2)


def test_metric_json_aggregation():
    from slr_sfs_amd import evaluation
    per = {"b": {"PSNR": [20.0, 22.0], "SSIM": [0.5, 0.7], "Perceptual": [0.1, 0.3]},
           "a": {"PSNR": [30.0, 30.0, 33.0], "SSIM": [0.9, 0.8, 0.7], "Perceptual": [0.2, 0.2, 0.2]}}
    res = evaluation.aggregate(per)
    assert list(res) == ["TotalPerceptual", "TotalPSNR", "TotalSSIM", "TotalPerceptual_std", "TotalPSNR_std", "TotalSSIM_std",
                         "Perceptual", "PSNR", "SSIM", "Perceptual_std", "PSNR_std", "SSIM_std"]
    assert res["PSNR"] == {"b": 21.0, "a": 31.0} and res["PSNR_std"]["b"] == 1.0
    allp = np.array([20.0, 22.0, 30.0, 30.0, 33.0])
    assert res["TotalPSNR"] == pytest.approx(allp.mean()) and res["TotalPSNR_std"] == pytest.approx(allp.std())
    assert res["SSIM_std"]["a"] == pytest.approx(np.std([0.9, 0.8, 0.7]))
    res2 = evaluation.aggregate({k: {m: v[m] for m in ("PSNR", "SSIM")} for k, v in per.items()}, ("PSNR", "SSIM"))
    assert "TotalPerceptual" not in res2 and "LPIPS" not in res2 and res2["TotalSSIM"] == res["TotalSSIM"]


def test_scene_selection_lists_skipped(tmp_path):
    """tools/evaluate.py's scene choice (eval_CLAW.py:66-77): a scene is scored when PredImg holds --frames frames and its ground truth is
    there with as many; the others are listed with the reason."""
    import importlib.util, os
    from slr_sfs_amd import io
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools",
                                                                                 "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    fr = torch.zeros(3, 8, 8, 3, dtype=torch.uint8)
    io.save_frames(fr, str(pred / "ok"))
    io.save_frames(fr[:2], str(pred / "short"))
    io.save_frames(fr, str(pred / "nogt"))
    os.makedirs(gt, exist_ok=True)
    np.save(gt / "ok.npy", fr.numpy())
    np.save(gt / "short.npy", fr.numpy())
    scenes, skipped = ev.select_scenes(str(pred), str(gt), 3)
    assert [s for s, _ in scenes] == ["ok"]
    assert sorted(n for n, _ in skipped) == ["nogt", "short"]


def test_cpu_tensors_raise():
    from slr_sfs_amd import metrics
    a = torch.rand(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        metrics.ssim(a, a)
    with pytest.raises(NotImplementedError):
        metrics.psnr(a, a)
    with pytest.raises(NotImplementedError):
        metrics.perceptual_sim(a, a, metrics.PerceptualVGG16())


def test_vgg16_loader_rejects_bad_state_dicts():
    from slr_sfs_amd import metrics
    sd = MF.vgg16_state_dict()
    net = metrics.load_vgg16_state_dict(metrics.PerceptualVGG16(), dict(sd, **{"classifier.0.weight": torch.zeros(4, 4)}))
    assert torch.equal(net.convs[12].weight, sd["features.28.weight"])
    bad = dict(sd)
    del bad["features.12.bias"]
    with pytest.raises(KeyError):
        metrics.load_vgg16_state_dict(metrics.PerceptualVGG16(), bad)
    bad = dict(sd, **{"features.5.weight": torch.zeros(128, 64, 1, 1)})
    with pytest.raises(ValueError):
        metrics.load_vgg16_state_dict(metrics.PerceptualVGG16(), bad)
    with pytest.raises(ValueError):
        metrics.load_vgg16_state_dict(metrics.PerceptualVGG16(), dict(sd, **{"features.99.weight": torch.zeros(1)}))
