"""Host-side checks of LPIPS (csrc/lpips.hip, ABI 26; metrics.LPIPSAlex), none of which needs a GPU: the written-out definition of
tests/lpips_f64.py against the reference's own PNet("alex") on the same seeded trunk (tests/golden/lpips_trunk_vs_reference.npz, made
by tools/make_golden_lpips.py), the loader of the two state dicts, metric.json's key order, the argument rule of tools/evaluate.py, the
entry points and their refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import lpips_f64 as D
import lpips_fixture as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("slr_lpips_prep", "slr_convkxk_weight_bytes", "slr_convkxk_f32_weights", "slr_convkxk_forward", "slr_relu_maxpool3x3s2_b8",
           "slr_lpips_distance_ws_bytes", "slr_lpips_distance")
P = 0x7F0000100000                                                           # a 16-byte aligned address that is never dereferenced


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def test_definition_reproduces_the_reference_trunk():
    """lpips_f64's trunk, scaling and normalisation give the reference's PNet("alex") value, per-layer scores and slice sums within
    1e-12 (float64 against float64).  The linear heads have no counterpart in the reference: they are not part of this file."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "lpips_trunk_vs_reference.npz"))
    assert sorted(g.files) == ["layers", "slice_sums", "val"]
    x0, x1 = LF.image_pair(*LF.GOLDEN_SHAPE)
    val, per, sums = D.pnet_alex(x0.double(), x1.double(), LF.alexnet_state_dict())
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())          # noqa: E731
    assert rel(val.numpy(), g["val"]) < 1e-12
    assert rel(torch.stack(per).numpy(), g["layers"]) < 1e-12
    assert rel(torch.stack(sums).numpy(), g["slice_sums"]) < 1e-12
    assert g["layers"].shape == (5, LF.GOLDEN_SHAPE[0]) and float(g["val"].min()) > 0.05


def test_definition_details():
    """The details the golden file cannot see or that are easy to get wrong: slice sizes at 31 x 31 (7, 3, 1, 1, 1), the eps outside
    the root, shift / scale as float32 values, the [0, 1] and [-1, 1] forms differing, two zero vectors giving 0."""
    sd, lin = LF.alexnet_state_dict(), LF.linear_state_dict()
    x = torch.rand(1, 3, 31, 31, dtype=torch.float64)
    assert [tuple(o.shape[1:]) for o in D.trunk(D.prep(x), sd)] == [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    with pytest.raises(RuntimeError):
        D.trunk(D.prep(torch.rand(1, 3, 30, 31, dtype=torch.float64)), sd)   # the second pool has no output
    f = torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)
    assert torch.equal(D.normalize_tensor(f), f / (5.0 + 1e-10))
    assert float(D.prep(torch.zeros(1, 3, 1, 1))[0, 0, 0, 0]) == float(np.float32(0.030)) / float(np.float32(0.458))
    z = torch.full((1, 8, 2, 2), -1.0)
    assert float(D.layer_distance(z, z - 1, torch.ones(8))) == 0.0
    a, b = LF.image_pair(*LF.SHAPES[0])
    assert abs(float(D.lpips(a, b, sd, lin)[0]) - float(D.lpips(a, b, sd, lin, normalize=True)[0])) > 1e-4
    assert float(D.lpips(a, a, sd, lin)[0]) == 0.0


def test_loader_takes_every_key_and_refuses_bad_ones():
    from slr_sfs_amd import metrics
    sd, lin = LF.alexnet_state_dict(), LF.linear_state_dict()
    full = dict(sd, **{"classifier.1.weight": torch.zeros(2, 2), "classifier.6.bias": torch.zeros(2)})
    net = metrics.load_lpips_state_dicts(metrics.LPIPSAlex(), full, lin)
    for conv, idx in zip((net.conv1, net.conv2, *net.convs), LF.ALEX_CONVS):
        assert torch.equal(conv.weight, sd[f"features.{idx}.weight"]) and torch.equal(conv.bias, sd[f"features.{idx}.bias"])
    for k, p in enumerate(net.lins):
        assert torch.equal(p, lin[f"lin{k}.model.1.weight"].view(-1)) and p.shape == (LF.CHANNELS[k],)
    assert [tuple(c.weight.shape) for c in (net.conv1, net.conv2, *net.convs)] == [(o, i, k, k) for i, o, k, _, _ in LF.ALEX_CFG]
    assert (net.conv1.stride, net.conv1.pad, net.conv2.stride, net.conv2.pad) == (4, 2, 1, 2)
    assert not any(p.requires_grad for p in net.parameters())
    fresh = metrics.LPIPSAlex
    for key in sd:
        with pytest.raises(KeyError, match=re.escape(key)):
            metrics.load_lpips_state_dicts(fresh(), {k: v for k, v in sd.items() if k != key}, lin)
        with pytest.raises(ValueError, match=re.escape(key)):
            metrics.load_lpips_state_dicts(fresh(), dict(sd, **{key: sd[key][..., :1] if sd[key].dim() > 1 else sd[key][:-1]}), lin)
    for key in lin:
        with pytest.raises(KeyError, match=re.escape(key)):
            metrics.load_lpips_state_dicts(fresh(), sd, {k: v for k, v in lin.items() if k != key})
        with pytest.raises(ValueError, match=re.escape(key)):
            metrics.load_lpips_state_dicts(fresh(), sd, dict(lin, **{key: lin[key].view(-1)}))
    with pytest.raises(ValueError, match="unexpected"):
        metrics.load_lpips_state_dicts(fresh(), dict(sd, **{"features.12.weight": torch.zeros(1)}), lin)
    with pytest.raises(ValueError, match="unexpected"):
        metrics.load_lpips_state_dicts(fresh(), sd, dict(lin, **{"lin5.model.1.weight": torch.zeros(1, 1, 1, 1)}))
    with pytest.raises(ValueError, match="unexpected"):
        metrics.load_lpips_state_dicts(fresh(), sd, dict(lin, **{"lin0.model.1.bias": torch.zeros(1)}))


def test_from_files_and_cpu_tensors(tmp_path):
    from slr_sfs_amd import metrics
    torch.save(LF.alexnet_state_dict(), tmp_path / "alexnet.pth")
    torch.save(LF.linear_state_dict(), tmp_path / "alex.pth")
    net = metrics.LPIPSAlex.from_files(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"))
    assert torch.equal(net.lins[4], LF.linear_state_dict()["lin4.model.1.weight"].view(-1))
    x = torch.zeros(1, 3, 40, 40)
    with pytest.raises(NotImplementedError):
        net(x, x)
    with pytest.raises(NotImplementedError):
        metrics.lpips_sim(x, x, net)


def test_metric_json_key_order():
    from slr_sfs_amd import evaluation
    assert evaluation.KEYS == ("Perceptual", "PSNR", "SSIM") and evaluation.KEYS_LPIPS == ("LPIPS", "Perceptual", "PSNR", "SSIM")
    per = {"s1": {k: [0.1, 0.3] for k in evaluation.KEYS_LPIPS}, "s0": {k: [0.5] for k in evaluation.KEYS_LPIPS}}
    res = evaluation.aggregate(per, evaluation.KEYS_LPIPS)
    order = ["LPIPS", "Perceptual", "PSNR", "SSIM"]                           # eval_CLAW.py:83-87, 150-155
    assert list(res) == [f"Total{k}" for k in order] + [f"Total{k}_std" for k in order] + order + [f"{k}_std" for k in order]
    assert res["TotalLPIPS"] == pytest.approx(0.3) and res["LPIPS"] == {"s1": pytest.approx(0.2), "s0": 0.5}
    assert list(evaluation.aggregate(per)) == list(evaluation.aggregate(per, evaluation.KEYS))       # the default is unchanged
    assert evaluation.metric_keys(True, True) == evaluation.KEYS_LPIPS and evaluation.metric_keys(True, False) == evaluation.KEYS
    assert evaluation.metric_keys(False, False) == ("PSNR", "SSIM") and evaluation.metric_keys(False, True) == ("LPIPS", "PSNR", "SSIM")


@pytest.mark.parametrize("tool", ["evaluate", "animate"])
def test_lpips_paths_go_together(tool, tmp_path, monkeypatch, capsys):
    """--lpips-alexnet without --lpips-linear (or the reverse) is an argument error, raised before anything touches a device."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        mod = __import__(tool)
    finally:
        sys.path.pop(0)
    base = [str(tmp_path), str(tmp_path)] if tool == "evaluate" else ["i.png", "f.flo", str(tmp_path), "None", "n", "64", "2", "1.0"]
    for flag in ("--lpips-alexnet", "--lpips-linear"):
        with pytest.raises(SystemExit) as e:
            if tool == "evaluate":
                mod.main(base + [flag, "x.pth"])
            else:
                monkeypatch.setattr(sys, "argv", ["animate.py"] + base + [flag, "x.pth"])
                mod.main()
        assert e.value.code == 2 and "go together" in capsys.readouterr().err


def test_entry_points_are_declared_and_abi_is_26(L):
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    section = re.sub(r"/\*.*?\*/", " ", "/*" + hdr[hdr.index("(ABI 26; csrc/lpips.hip)"):], flags=re.S)      # (prototypes, not comments)
    assert tuple(re.findall(r"\b(slr_[a-z0-9_]+)\s*\(", section)) == ENTRIES        # the section declares these, in this order
    src = open(os.path.join(ROOT, "slr-sfs_amd", "csrc", "lpips.hip")).read()
    assert sorted(re.findall(r"SLR_EXPORT\s+\w+\s+(slr_\w+)\s*\(", src)) == sorted(ENTRIES)     # ... and the source exports exactly them
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.ABI_VERSION >= 26 and L.slr_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION


def test_entry_points_refuse_before_launching(L):
    """Argument errors return before anything is launched: no device is needed to see them."""
    p = [ctypes.c_void_p(P + 65536 * k) for k in range(6)]
    refused = lambda rc, *words: rc == -1 and all(w in L.slr_last_error() for w in words)      # noqa: E731
    assert L.slr_convkxk_weight_bytes(64, 3, 11) == 2 * 3 * 61 * 64 * 4 and L.slr_convkxk_weight_bytes(192, 64, 5) == 6 * 64 * 13 * 64 * 4
    assert L.slr_convkxk_weight_bytes(40, 3, 5) == 2 * 3 * 13 * 64 * 4
    for bad in [(64, 3, 3), (64, 3, 7), (0, 3, 11), (64, 0, 5), (1 << 16, 3, 5)]:
        assert L.slr_convkxk_weight_bytes(*bad) == 0
    fw = L.slr_convkxk_forward
    assert refused(fw(None, p[1], p[2], p[3], 1, 3, 64, 31, 31, 11, 4, 2, 0, None), b"slr_convkxk_forward", b"null")
    for k, s, pad in [(11, 4, 1), (11, 2, 2), (5, 2, 2), (3, 1, 1), (7, 2, 3)]:
        assert refused(fw(*p[:4], 1, 3, 64, 31, 31, k, s, pad, 0, None), b"(11, 4, 2) or (5, 1, 2)")
    for N, cin, cout, H, W in [(0, 3, 64, 31, 31), (1, 3, 60, 31, 31), (1, 3, 64, 6, 31), (1, 3, 64, 31, 6), (1, 3, 64, 1 << 16, 1 << 16)]:
        assert refused(fw(*p[:4], N, cin, cout, H, W, 11, 4, 2, 0, None), b"sizes")
    assert refused(fw(*p[:4], 1, 12, 64, 31, 31, 5, 1, 2, 1, None), b"Cin % 8")
    assert refused(fw(ctypes.c_void_p(P + 2), *p[1:4], 1, 3, 64, 31, 31, 11, 4, 2, 0, None), b"aligned")
    assert refused(fw(ctypes.c_void_p(P + 4), *p[1:4], 1, 64, 192, 9, 9, 5, 1, 2, 1, None), b"aligned")      # channel-blocked: 16 bytes
    assert refused(fw(*p[:3], ctypes.c_void_p(P + 8), 1, 3, 64, 31, 31, 11, 4, 2, 0, None), b"aligned")
    assert refused(L.slr_convkxk_f32_weights(p[0], p[1], 64, 3, 7, None), b"K (11 or 5)")
    assert refused(L.slr_lpips_prep(None, 0, 0, p[1], 1, 31, 31, None), b"slr_lpips_prep", b"null")
    assert refused(L.slr_lpips_prep(p[0], 0, 0, p[1], 1, 0, 31, None), b"sizes")
    pool = L.slr_relu_maxpool3x3s2_b8
    for N, C, H, W in [(1, 8, 2, 3), (1, 8, 3, 2), (1, 12, 3, 3), (0, 8, 3, 3)]:
        assert refused(pool(p[0], p[1], N, C, H, W, None), b"sizes")
    assert refused(pool(ctypes.c_void_p(P + 8), p[1], 1, 8, 3, 3, None), b"aligned")
    assert L.slr_lpips_distance_ws_bytes(3, 23, 15) == 3 * 2 * 8 and L.slr_lpips_distance_ws_bytes(1, 1, 1) == 8
    assert L.slr_lpips_distance_ws_bytes(0, 4, 4) == 0
    dist = L.slr_lpips_distance
    assert refused(dist(p[0], p[1], None, p[3], 1, 64, 4, 4, p[4], 8, None), b"slr_lpips_distance", b"null")
    assert refused(dist(*p[:4], 1, 60, 4, 4, p[4], 8, None), b"sizes")
    assert refused(dist(*p[:4], 3, 64, 23, 15, p[4], 47, None), b"ws")
    assert refused(dist(*p[:4], 1, 64, 4, 4, ctypes.c_void_p(P + 4), 8, None), b"ws")
