"""The motion U-Nets of slr_sfs_amd.nets (Unet4Motion, SPADEUnet4MaskMotion) against the reference's own UnetMotion /
SPADEUnetMaskMotion, on CPU: the reference modules were built by its option parser with the flag sets of tests/motion_fixture.py,
their state dicts replaced by the deterministic ones of that module, and their forward_flow outputs stored in
tests/golden/motion_vs_reference.npz (tools/make_golden_motion.py).  Here the same state dicts are regenerated and loaded through
load_motion_state_dict; plus the input preparation of the reference's motion test script (motion_inputs_from_flow)."""
import numpy as np
import pytest
import torch

import motion_fixture as MF

NET = {"unet": ("Unet4Motion", 3), "spade": ("SPADEUnet4MaskMotion", 6)}


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(f"{golden_dir}/motion_vs_reference.npz")


def _net(ref, flagset, prefix=MF.PREFIX):
    from slr_sfs_amd import nets
    keys = [str(k) for k in ref[f"{flagset}_keys"]]
    sd = {prefix + k: v for k, v in MF.state_dict(flagset, keys, ref[f"{flagset}_shapes"]).items()}
    cls, cin = NET[flagset]
    return nets.load_motion_state_dict(getattr(nets, cls)(cin), sd, prefix).eval(), sd


@pytest.mark.parametrize("case", ["unet_256", "spade_256", "spade_256x512"])
def test_motion_nets_vs_reference(ref, case):
    from slr_sfs_amd import nets
    flagset = MF.CASES[case][0]
    net, _ = _net(ref, flagset)
    with nets.cpu_reference():
        out = net(MF.motion_input(case)) * float(ref[f"{flagset}_div_flow"])
    if f"{case}_out" in ref:
        ra = torch.from_numpy(ref[f"{case}_out"])
        assert ra.shape == out.shape
        err, scale = (ra - out).abs().max().item(), ra.abs().max().item()
    else:
        flat = out.double()[0].reshape(-1)
        pos = MF.digest_positions(case, flat.numel())
        err = float(np.abs(flat[pos].numpy() - ref[f"{case}_samples"]).max())
        scale = float(ref[f"{case}_max_abs"])
        assert np.allclose(flat.reshape(2, -1).sum(1).numpy(), ref[f"{case}_plane_sums"], rtol=0, atol=1e-4 * scale * flat.numel() ** 0.5)
        assert abs(flat.abs().max().item() - scale) <= 1e-4 * scale
    assert err <= 1e-4 * scale, (case, err, scale)


def test_loader_consumes_every_key_and_checks_them(ref):
    from slr_sfs_amd import nets
    for flagset in NET:
        _, sd = _net(ref, flagset, prefix="model.module.motion_regressor.motion_predictor.")
        cls, cin = NET[flagset]
        extra = dict(sd, **{"model.module.motion_regressor.motion_predictor.unknown.weight": torch.zeros(1)})
        with pytest.raises(KeyError, match="not consumed"):
            nets.load_motion_state_dict(getattr(nets, cls)(cin), extra, "model.module.motion_regressor.motion_predictor.")
        missing = {k: v for k, v in sd.items() if not k.endswith("conv3.bias")}
        with pytest.raises(KeyError):
            nets.load_motion_state_dict(getattr(nets, cls)(cin), missing, "model.module.motion_regressor.motion_predictor.")


def test_grid_channels_and_cpu_tensors_raise(ref):
    from slr_sfs_amd import nets
    net, _ = _net(ref, "spade")
    with nets.cpu_reference():
        with pytest.raises(ValueError, match="multiples of 256"):
            net(torch.zeros(1, 6, 256, 384))
        with pytest.raises(ValueError, match="multiples of 256"):
            net(torch.zeros(1, 6, 200, 256))
        with pytest.raises(ValueError):
            net(torch.zeros(1, 4, 256, 256))
    with pytest.raises(ValueError):
        nets.SPADEUnet4MaskMotion(3)
    with pytest.raises(ValueError):
        nets.SPADEUnet4MaskMotion(4)
    with pytest.raises(NotImplementedError):                 # no CPU path outside cpu_reference()
        net(torch.zeros(1, 6, 256, 256))
    unet, _ = _net(ref, "unet")
    with pytest.raises(NotImplementedError):
        unet(torch.zeros(1, 3, 256, 256))


def _hints_numpy(flow, points):
    """NumPy restatement of test_animating/test_motion_4eval_rawsize_threshold.py:167-212 with the hint pixels given."""
    _, _, h, w = flow.shape
    f = flow[0].astype(np.float32)
    speed = np.sqrt(f[0] ** 2 + f[1] ** 2)
    mask = (speed > 0.2161635).astype(np.float32)
    if mask.sum() < 5:
        return mask, np.zeros_like(f)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    sigma = h / 5
    num = np.zeros_like(f, dtype=np.float64)
    den = np.zeros((h, w), np.float64)
    for hy, hx in points:
        d = np.sqrt((xs - hx) ** 2 + (ys - hy) ** 2)
        wgt = np.exp(-(d / sigma) ** 2)
        num += wgt * f[:, hy, hx][:, None, None]
        den += wgt
    den[den == 0] = 1
    return mask, (num / den).astype(np.float32) * mask


def test_motion_inputs_from_flow_with_given_points():
    from slr_sfs_amd import motion
    h, w, W = 37, 53, 256                                    # an odd raw size, resized to the network's W x W
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    flow = np.stack([np.sin(x / 7) * 2, np.cos(y / 5)])[None].astype(np.float32) * (x > 20)
    pts = [(3, 25), (10, 40), (20, 22), (30, 50), (36, 30)]
    mask, hint = motion.motion_inputs_from_flow(torch.from_numpy(flow), W, points=pts)
    m_ref, h_ref = _hints_numpy(flow, pts)
    iy = np.floor(np.arange(W) * (h / W)).astype(int)        # nearest resize of the raw-size mask / hint
    ix = np.floor(np.arange(W) * (w / W)).astype(int)
    assert mask.shape == (1, 1, W, W) and hint.shape == (1, 2, W, W)
    assert np.array_equal(mask[0, 0].numpy(), m_ref[iy][:, ix])
    assert np.abs(hint[0].numpy() - h_ref[:, iy][:, :, ix]).max() <= 1e-5 * np.abs(h_ref).max()


def test_motion_inputs_from_flow_small_and_no_hint_branches():
    from slr_sfs_amd import motion
    flow = np.zeros((1, 2, 40, 40), np.float32)
    flow[0, 0, 5, 5:9] = 1.0                                 # four moving pixels: fewer than 5 -> zero hint
    mask, hint = motion.motion_inputs_from_flow(torch.from_numpy(flow), 256)
    assert float(mask.sum()) > 0 and float(hint.abs().sum()) == 0.0
    # no-hint branch (:214-219): the flow resized (nearest) to W x W, mask = speed >= 0.1 * mean speed
    flow = np.random.default_rng(3).standard_normal((1, 2, 64, 64)).astype(np.float32)
    mask, hint = motion.motion_inputs_from_flow(torch.from_numpy(flow), 256, hints=False)
    assert hint is None
    g = np.repeat(np.repeat(flow, 4, 2), 4, 3)
    sp = np.sqrt(g[:, 0:1] ** 2 + g[:, 1:2] ** 2)
    assert np.array_equal(mask.numpy(), 1.0 - (sp < sp.mean() * 0.1).astype(np.float32))


def test_kmeans_hint_points_are_deterministic():
    from slr_sfs_amd import motion
    y, x = np.meshgrid(np.arange(48, dtype=np.float32), np.arange(64, dtype=np.float32), indexing="ij")
    flow = np.stack([np.ones_like(x), np.zeros_like(x)])[None].astype(np.float32) * ((x > 30) & (y > 10))
    a = motion.hint_points(torch.from_numpy(flow)[0].norm(dim=0) > 0.2161635)
    b = motion.hint_points(torch.from_numpy(flow)[0].norm(dim=0) > 0.2161635)
    assert a == b and len(a) == 5
    assert all(10 < py < 48 and 30 < px < 64 for py, px in a)
