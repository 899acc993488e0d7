"""The float64 definition of tests/splat_f64.py, pinned on the CPU: against the golden files made from the reference, against the
float32 oracle on every flow family the GPU sweeps use, and its restatement of the backward kernel's block rule against the counts
at the timed shapes -- so that tests/test_gpu_gradients.py leans on something checked.  Tolerances are the ones the GPU tests use for
the same data (tests/test_gpu_parity.py, tests/test_gpu_frontends.py); against the oracle the float32 oracle is the inexact side."""
import numpy as np
import pytest
import torch

import splat_f64 as F64

TOL = dict(rtol=1e-5, atol=1e-5)
MODES = ("summation", "average", "linear", "softmax")


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).double()


def smooth_motion(H, W, seed=0, amp=1.5):
    rng = np.random.default_rng(seed)
    p1, p2 = rng.uniform(0, 2 * np.pi, 2)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    u = amp * np.sin(2 * np.pi * (2 * x / W + y / H) + p1)
    v = amp * np.cos(2 * np.pi * (x / W - 1.5 * y / H) + p2)
    m = (x >= 0.35 * W).astype(np.float32)
    return np.stack([u * m, v * m])[None].astype(np.float32)


def sum_and_grads(x, flow, gout):
    xt, ft = t64(x).requires_grad_(True), t64(flow).requires_grad_(True)
    out = F64.splat_sum(xt, ft)
    gin, gflow = torch.autograd.grad(out, (xt, ft), t64(gout))
    return out.detach().numpy(), gin.numpy(), gflow.numpy()


def test_splat_sum_golden(golden_dir):
    g = np.load(f"{golden_dir}/splat_sum.npz")
    assert int(g["count"]) > 0
    for i in range(int(g["count"])):
        tag = str(g[f"c{i}_tag"])
        out, gin, gflow = sum_and_grads(g[f"c{i}_in"], g[f"c{i}_flow"], g[f"c{i}_gout"])
        np.testing.assert_allclose(out, g[f"c{i}_out"], err_msg=tag, **TOL)
        np.testing.assert_allclose(gin, g[f"c{i}_gin"], err_msg=tag, **TOL)
        np.testing.assert_allclose(gflow, g[f"c{i}_gflow"], rtol=1e-6, atol=1e-6, err_msg=tag)


def test_function_softsplat_modes_golden(golden_dir):
    g = np.load(f"{golden_dir}/splat_modes.npz")
    assert int(g["count"]) == 32
    for i in range(32):
        out = F64.function_softsplat(t64(g[f"c{i}_in"]), t64(g[f"c{i}_flow"]), t64(g[f"c{i}_metric"]), str(g[f"c{i}_mode"]))
        np.testing.assert_allclose(out.numpy(), g[f"c{i}_out"], err_msg=str(g[f"c{i}_tag"]), rtol=1e-4, atol=1e-5)


FAMILIES = ("uniform3", "uniform60", "integer", "collapse", "wave", "euler30", "euler59", "nonfinite", "far")
SHAPES = ((1, 1, 1, 1), (2, 3, 5, 1), (1, 2, 1, 7), (1, 17, 9, 65), (2, 6, 40, 72), (3, 5, 33, 130), (1, 4, 96, 200))


def family_flow(oracle, kind, N, H, W, rng):
    """The flow families of tests/test_gpu_frontends.py::test_randomised_sweep and of the Euler / non-finite / far-away cases."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    if kind == "uniform3":
        fl = rng.uniform(-3, 3, (N, 2, H, W))
    elif kind == "uniform60":
        fl = rng.uniform(-60, 60, (N, 2, H, W))
    elif kind == "integer":
        fl = rng.integers(-5, 6, (N, 2, H, W)).astype(np.float32)
    elif kind == "collapse":
        fl = np.stack([(W / 2 - x) * rng.uniform(0.5, 1.0), (H / 2 - y) * rng.uniform(0.5, 1.0)])[None].repeat(N, 0)
    elif kind == "wave":
        fl = np.stack([np.sin(x / 7 + y / 11) * 6, np.cos(x / 9 - y / 5) * 6])[None].repeat(N, 0)
    elif kind in ("euler30", "euler59"):
        fl = np.concatenate([oracle.euler_integration(smooth_motion(H, W, n, amp=3.0), int(kind[-2:]))[0] for n in range(N)])
    elif kind == "nonfinite":
        fl = rng.uniform(-2, 2, (N, 2, H, W))
        fl[rng.random(fl.shape) < 0.02] = np.nan
        fl[rng.random(fl.shape) < 0.01] = np.inf
        fl[rng.random(fl.shape) < 0.01] = -np.inf
    else:
        fl = rng.uniform(-2, 2, (N, 2, H, W))
        fl[rng.random(fl.shape) < 0.03] = 3.0e9
        fl[rng.random(fl.shape) < 0.03] = -1.0e4
        fl[rng.random(fl.shape) < 0.01] = np.nan
        fl[0, :, 0, 0] = (-2.0e9, 1.0e38)
    return fl.astype(np.float32)


@pytest.mark.parametrize("kind", FAMILIES)
def test_sum_forward_backward_vs_oracle(oracle, kind):
    """Forward within the per-pixel bound 4e-6 * splat(|x|) + 1e-6 (the oracle's float32 sums are the inexact side), gradInput and
    gradFlow within the golden files' tolerances on the scale of the tensor; a dropped pixel has gradients of exactly 0."""
    for case, (N, C, H, W) in enumerate(SHAPES):
        rng = np.random.default_rng(100 * FAMILIES.index(kind) + case)
        flow = family_flow(oracle, kind, N, H, W, rng)
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        go = rng.standard_normal((N, C, H, W)).astype(np.float32)
        out, gin, gflow = sum_and_grads(x, flow, go)
        assert np.isfinite(out).all() and np.isfinite(gin).all() and np.isfinite(gflow).all()
        ref = oracle.softsplat_forward(x, flow)
        bound = 4e-6 * oracle.softsplat_forward(np.abs(x), flow) + 1e-6
        assert (np.abs(out - ref) <= bound).all(), (kind, N, C, H, W, float((np.abs(out - ref) - bound).max()))
        ogi, ogf = oracle.softsplat_backward(x, flow, go)
        np.testing.assert_allclose(gin, ogi, err_msg=f"{kind} {N, C, H, W}", **TOL)
        scale = max(1.0, float(np.abs(ogf).max()))
        np.testing.assert_allclose(gflow, ogf, rtol=1e-6, atol=1e-6 * scale, err_msg=f"{kind} {N, C, H, W}")
        dropped = ~np.isfinite(flow).all(axis=1)
        assert (gin[np.broadcast_to(dropped[:, None], gin.shape)] == 0).all()
        assert (gflow[np.broadcast_to(dropped[:, None], gflow.shape)] == 0).all()
        assert (ogf[np.broadcast_to(dropped[:, None], ogf.shape)] == 0).all()


@pytest.mark.parametrize("kind", FAMILIES)
def test_modes_vs_oracle(oracle, kind):
    """function_softsplat in all modes against oracle.function_softsplat, the tolerance of the modes' golden file; same holes."""
    for case, (N, C, H, W) in enumerate(SHAPES):
        rng = np.random.default_rng(1000 + 100 * FAMILIES.index(kind) + case)
        flow = family_flow(oracle, kind, N, H, W, rng)
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        met = (rng.standard_normal((N, 1, H, W)) * 0.7).astype(np.float32)
        for mode in MODES:
            m = np.abs(met) + 0.1 if mode == "linear" else met
            out = F64.function_softsplat(t64(x), t64(flow), t64(m), mode).numpy()
            ref = oracle.function_softsplat(x, flow, m, mode)
            scale = max(1.0, float(np.abs(ref).max()))
            np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-5 * scale, err_msg=f"{kind} {mode} {N, C, H, W}")
            assert np.array_equal((out == 0).all(axis=1), (ref == 0).all(axis=1)), (kind, mode)


def test_exact_zero_normaliser_divides_by_one():
    """models/softsplat.py:684: two sources with weights +a and -a on one pixel (normaliser exactly 0) and a pixel nobody reaches."""
    x = np.array([[[[1.0, 2.0, 4.0, 8.0]]]], np.float32)
    flow = np.zeros((1, 2, 1, 4), np.float32)
    flow[0, 0, 0, 1] = -1.0                                 # pixel 1 lands on pixel 0; nobody reaches pixel 1
    met = np.array([[[[0.5, -0.5, 1.0, 2.0]]]], np.float32)
    xt, mt = t64(x).requires_grad_(True), t64(met).requires_grad_(True)
    out, norm = F64.function_softsplat(xt, t64(flow), mt, "linear", return_norm=True)
    assert norm.detach().flatten().tolist() == [0.0, 0.0, 1.0, 2.0]
    assert out.detach().flatten().tolist() == [1.0 * 0.5 - 2.0 * 0.5, 0.0, 4.0, 8.0]
    gx, gm = torch.autograd.grad(out.sum(), (xt, mt))
    assert gx.flatten().tolist() == [0.5, -0.5, 1.0, 1.0] and gm.flatten().tolist() == [1.0, 2.0, 0.0, 0.0]


def test_training_step_matches_the_oracle_forward(oracle):
    """training_step on the oracle's displacement fields = oracle.synth_baseline (the clamp of :605 is inactive on Z - Z.max() >= -20)."""
    H, W, N, t = 40, 72, 12, 5
    rng = np.random.default_rng(4)
    fs = rng.standard_normal((1, 8, H, W)).astype(np.float32)
    Z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    m = smooth_motion(H, W, 1, amp=2.0)
    ff, fp = oracle.euler_integration(m, t)[0], oracle.euler_integration(-m, N - t)[0]
    alpha = torch.tensor([1.0 - np.float32(t) / np.float32(N)], dtype=torch.float32).view(1, 1, 1, 1)
    out = F64.training_step(t64(fs), t64(Z), t64(ff), t64(fp), alpha).numpy()
    np.testing.assert_allclose(out, oracle.synth_baseline(fs, Z, m, t, N), rtol=1e-4, atol=1e-5)


def timed_flow(oracle, t):
    m = smooth_motion(768, 1280)
    return np.zeros_like(m) if t == 0 else oracle.euler_integration(m, t)[0]


def test_backward_block_paths_at_the_timed_shapes(oracle):
    """The block rule of csrc/grad.hip at 768x1280 (bench.py's backward_roofline flows): identity keeps every block straight;
    Euler t=30 reaches the staged loops of 1, 2, 3, 4 and 6 cells per work-item; t=59 all of them and the corner-pair path."""
    p = F64.backward_block_paths(timed_flow(oracle, 0))
    assert p == dict({k: 0 for k in F64.CLASSES}, straight=1920), p
    p30 = F64.backward_block_paths(timed_flow(oracle, 30))
    assert sum(p30.values()) == 1920
    for k in ("straight", "staged1", "staged2", "staged3", "staged4", "staged6", "empty"):
        assert p30[k] > 0, (k, p30)
    p59 = F64.backward_block_paths(timed_flow(oracle, 59))
    assert sum(p59.values()) == 1920
    for k in F64.CLASSES:
        assert p59[k] > 0, (k, p59)
    print("t=30", p30, "t=59", p59)


def test_backward_block_paths_small_cases():
    z = np.zeros((2, 2, 20, 70), np.float32)                # ragged: 3 x 2 blocks per sample, the right ones 6 columns wide
    assert F64.backward_block_paths(z)["straight"] == 12
    z[0] = 1.0e6                                            # a sample that leaves the image
    z[1, 0, 0, 0] = np.nan
    p = F64.backward_block_paths(z)
    assert p["empty"] == 6 and p["straight"] == 6, p
    yy, xx = np.meshgrid(np.arange(160, dtype=np.float32), np.arange(264, dtype=np.float32), indexing="ij")
    a = np.deg2rad(55.0)                                    # tests/test_gpu_parity.py::test_backward_blocks_whose_boxes_do_not_fit
    X = 132 + 2.2 * (np.cos(a) * (xx - 132) - np.sin(a) * (yy - 78.3)) + 0.37
    Y = 78.3 + 2.2 * (np.sin(a) * (xx - 132) + np.cos(a) * (yy - 78.3)) + 0.21
    cls = F64.backward_block_classes(np.stack([X - xx, Y - yy])[None].astype(np.float32))
    assert F64.CLASSES[cls[0, 6, 2]] == "bent_no_fit", cls[0]
