"""GPU parity: HIP kernels (through the Python mirror -> ctypes -> C ABI) vs the CPU oracle and
the golden fixtures generated from the reference.  Tolerances:
  * Euler integration, splat backward, maximum-splat family: bit-exact (deterministic order);
  * summation / normalised splats: 1e-5 abs+rel on O(1) data -- the summation ORDER of a splat
    is unspecified in the reference itself (racing fp32 atomicAdds, softsplat.py:187-199), so
    only rounding-noise-level agreement is meaningful; north_star's bound is 1e-4 max-abs.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()          # fail loudly if the HIP library is missing
    return slr_sfs_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def load(golden_dir, name):
    return np.load(f"{golden_dir}/{name}.npz")


def assert_same_holes(gen, ref, slack=4):
    """Holes (pixels no source reaches) are exactly 0.0 in every channel, and they are the same pixels.  Element-wise
    the zero patterns may differ in a handful of places: a value whose contributions cancel to exactly 0.0 in one
    summation order is ~1e-8 in another (the reference's own order is unspecified: racing atomicAdds)."""
    assert np.array_equal((gen == 0).all(axis=1), (ref == 0).all(axis=1))
    diff = (gen == 0) != (ref == 0)
    assert int(diff.sum()) <= slack, int(diff.sum())
    if diff.any():
        assert float(np.abs(gen[diff]).max()) < 1e-6 and float(np.abs(ref[diff]).max()) < 1e-6


def smooth_motion(H, W, seed=0, amp=1.5):
    rng = np.random.default_rng(seed)
    p1, p2 = rng.uniform(0, 2 * np.pi, 2)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    u = amp * np.sin(2 * np.pi * (2 * x / W + y / H) + p1)
    v = amp * np.cos(2 * np.pi * (x / W - 1.5 * y / H) + p2)
    m = (x >= 0.35 * W).astype(np.float32)
    return np.stack([u * m, v * m])[None].astype(np.float32)


# ------------------------------------------------------------------------------ euler

def test_euler_golden_bit_exact(S, golden_dir):
    g = load(golden_dir, "euler")
    for i in range(int(g["count"])):
        d, v = S.euler_integration(dev(g[f"c{i}_motion"]), int(g[f"c{i}_n"]))
        tag = str(g[f"c{i}_tag"])
        assert np.array_equal(host(d), g[f"c{i}_disp"]), tag
        assert np.array_equal(host(v), g[f"c{i}_vis"]), tag


def test_euler_tensor_step_count_and_module(S, golden_dir):
    g = load(golden_dir, "euler")
    m, dest = g["module_motion"], g["module_dest"]
    d, v = S.EulerIntegration()(dev(m), torch.from_numpy(dest.astype(np.int64)).cuda(), show_visible_pixels=True)
    assert np.array_equal(host(d), g["module_disp"])
    assert np.array_equal(host(v), g["module_vis"])
    d1 = S.EulerIntegration()(dev(m), torch.from_numpy(dest.astype(np.int64)))
    assert np.array_equal(host(d1), g["module_disp"])


def test_euler_batch_is_one_launch_without_host_sync(S, golden_dir):
    """EulerIntegration.forward on a batch (euler_integration_manipulator.py:58-71; the training step's call,
    animating_softmax_splating.py:579-580): 16 samples with their own step counts, bit-exact with the reference module's
    output, gradient w.r.t. the motion fields vs torch autograd through the reference -- and with the step counts on the device the
    call never synchronises the host (torch's sync debug mode raises on any .item() / blocking copy)."""
    g = load(golden_dir, "euler_batch")
    mod = S.EulerIntegration()
    for tag in ("a", "b"):
        m = dev(g[f"{tag}_motion"])
        steps = torch.from_numpy(g[f"{tag}_steps"]).cuda()
        gout = dev(g[f"{tag}_gout"])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            d, v = mod(m, steps, show_visible_pixels=True)
            mg_ = m.clone().requires_grad_(True)
            dg = mod(mg_, steps)
            (gm,) = torch.autograd.grad(dg, mg_, gout)
            d_neg = mod(-m, steps + 1 - steps)              # (device arithmetic on the counts, as the model does)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert np.array_equal(host(d), g[f"{tag}_disp"]), tag
        assert np.array_equal(host(v), g[f"{tag}_vis"]), tag
        assert np.array_equal(host(dg), g[f"{tag}_disp"]), tag
        # (fp32 atomics in any order against torch's index_put order: cells that hundreds of paths cross hold sums of ~3)
        np.testing.assert_allclose(host(gm), g[f"{tag}_gmotion"], rtol=1e-4, atol=1e-4, err_msg=tag)
        for b in (0, 5, 15):                                 # one step of the negated field, per sample = the one-sample call
            d1, _ = S.euler_integration(-m[b:b + 1], 1)
            assert np.array_equal(host(d_neg[b:b + 1]), host(d1))
        # step counts as a host tensor / a list / int32: same result
        assert np.array_equal(host(mod(m, torch.from_numpy(g[f"{tag}_steps"]))), g[f"{tag}_disp"])
        assert np.array_equal(host(mod(m, [int(x) for x in g[f"{tag}_steps"]])), g[f"{tag}_disp"])
        assert np.array_equal(host(mod(m, steps.to(torch.int32))), g[f"{tag}_disp"])
    assert mod(torch.zeros(0, 2, 4, 4).cuda(), torch.zeros(0, dtype=torch.long)).shape == (0, 2, 4, 4)
    with pytest.raises(NotImplementedError):
        mod(torch.zeros(2, 2, 4, 4), torch.tensor([1, 1]))


def test_euler_all_frames_vs_oracle(S, oracle):
    for (H, W, seed) in [(48, 80, 0), (37, 53, 1)]:
        m = smooth_motion(H, W, seed, amp=2.5)
        for sign in (1.0, -1.0):
            d, v = S.euler_integration_all(dev(m), 60, sign=sign)
            od, ov = oracle.euler_integration_all(sign * m, 60)
            assert np.array_equal(host(d), od)
            assert np.array_equal(host(v), ov)


def test_euler_full_size_vs_oracle(S, oracle):
    m = smooth_motion(768, 1280, 2)
    d, v = S.euler_integration(dev(m), 59)
    od, ov = oracle.euler_integration(m, 59)
    assert np.array_equal(host(d), od) and np.array_equal(host(v), ov)
    dn, _ = S.euler_integration(dev(-m), 17)
    dn2, _ = S.euler_integration_all(dev(m), 17, sign=-1.0)
    assert np.array_equal(host(dn)[0], host(dn2)[17])


def test_euler_backward_golden_and_oracle(S, oracle, golden_dir):
    """The drop-in euler_integration is differentiable w.r.t. the motion field like the reference's loop
    (euler_integration_manipulator.py:36-55): gradients vs torch autograd through the REFERENCE (golden), vs the
    oracle on a larger field, through EulerIntegration too; visible_pixels carries no gradient."""
    g = load(golden_dir, "euler_grad")
    for i in range(int(g["count"])):
        m = dev(g[f"c{i}_motion"]).requires_grad_(True)
        d, v = S.euler_integration(m, int(g[f"c{i}_n"]))
        assert d.requires_grad and not v.requires_grad
        (gm,) = torch.autograd.grad(d, m, dev(g[f"c{i}_gout"]))
        np.testing.assert_allclose(host(gm), g[f"c{i}_gmotion"], rtol=1e-5, atol=1e-5, err_msg=str(g[f"c{i}_tag"]))
    H, W, n = 96, 160, 23
    mo = smooth_motion(H, W, 7, amp=2.0)
    go = np.random.default_rng(3).standard_normal((1, 2, H, W)).astype(np.float32)
    m = dev(mo).requires_grad_(True)
    d = S.EulerIntegration()(m, torch.tensor([n]))
    d.backward(dev(go))
    np.testing.assert_allclose(host(m.grad), oracle.euler_backward(mo, n, go), rtol=1e-4, atol=1e-4)
    with torch.no_grad():                                     # inference path unchanged: no graph
        assert not S.euler_integration(m, n)[0].requires_grad
    with pytest.raises(RuntimeError):
        S.euler_integration_all(m, n)


def test_euler_asserts(S):
    with pytest.raises(AssertionError):
        S.euler_integration(torch.zeros(2, 2, 4, 4).cuda(), 1)        # batch must be 1 (:20)
    with pytest.raises(AssertionError):
        S.euler_integration(torch.zeros(1, 3, 4, 4).cuda(), 1)        # two channels (:21)
    with pytest.raises(NotImplementedError):
        S.euler_integration(torch.zeros(1, 2, 4, 4), 1)               # no CPU path


# ------------------------------------------------------------------------------ summation splat

def test_splat_sum_golden_forward_backward(S, golden_dir):
    g = load(golden_dir, "splat_sum")
    for i in range(int(g["count"])):
        tag = str(g[f"c{i}_tag"])
        x = dev(g[f"c{i}_in"]).requires_grad_(True)
        fl = dev(g[f"c{i}_flow"]).requires_grad_(True)
        out = S.softsplat._FunctionSoftsplat.apply(x, fl)
        np.testing.assert_allclose(host(out), g[f"c{i}_out"], err_msg=tag, **TOL)
        out.backward(dev(g[f"c{i}_gout"]))
        assert np.array_equal(host(x.grad), g[f"c{i}_gin"]), tag
        np.testing.assert_allclose(host(fl.grad), g[f"c{i}_gflow"], rtol=1e-6, atol=1e-6, err_msg=tag)


def test_splat_needs_input_grad_subsets(S, golden_dir):
    g = load(golden_dir, "splat_sum")
    x, fl, go = g["c3_in"], g["c3_flow"], g["c3_gout"]
    a = dev(x).requires_grad_(True)
    S.softsplat._FunctionSoftsplat.apply(a, dev(fl)).backward(dev(go))
    assert np.array_equal(host(a.grad), g["c3_gin"])
    b = dev(fl).requires_grad_(True)
    S.softsplat._FunctionSoftsplat.apply(dev(x), b).backward(dev(go))
    np.testing.assert_allclose(host(b.grad), g["c3_gflow"], rtol=1e-6, atol=1e-6)


def test_backward_one_launch_equals_separate_launches(S, oracle):
    """slr_softsplat_backward with both gradients requested runs ONE kernel that gathers gradOutput once for both
    (csrc/grad.hip); each gradient is bit-identical to the launch that computes it alone (same terms, same order),
    and gradInput to the oracle, on an Euler-integrated flow with non-finite and far-away entries, C = 65 (channel
    tail of the 4-channel passes), batch 2."""
    from slr_sfs_amd._lib import check, lib, ptr, stream_of
    N, C, H, W = 2, 65, 96, 200
    rng = np.random.default_rng(12)
    flow = np.concatenate([oracle.euler_integration(smooth_motion(H, W, n, amp=3.0), 35 + n)[0] for n in range(N)])
    flow[0, 0, 5, 7] = np.nan
    flow[1, 1, 50, 60] = np.inf
    flow[0, :, 20, 30] = (3.0e9, -2.0e9)
    x, go = rng.standard_normal((N, C, H, W)).astype(np.float32), rng.standard_normal((N, C, H, W)).astype(np.float32)
    X, F, G = dev(x), dev(flow), dev(go)
    gi1, gf1, gi2, gf2 = torch.empty_like(X), torch.empty_like(F), torch.empty_like(X), torch.empty_like(F)
    L, st = lib(), stream_of(X)
    check(L.slr_softsplat_backward(ptr(X), ptr(F), ptr(G), ptr(gi1), ptr(gf1), N, C, H, W, st), "both")
    check(L.slr_softsplat_backward(ptr(X), ptr(F), ptr(G), ptr(gi2), None, N, C, H, W, st), "input")
    check(L.slr_softsplat_backward(ptr(X), ptr(F), ptr(G), None, ptr(gf2), N, C, H, W, st), "flow")
    assert torch.equal(gi1, gi2) and torch.equal(gf1, gf2)
    ogi, ogf = oracle.softsplat_backward(x, flow, go)
    assert np.array_equal(host(gi1), ogi)
    np.testing.assert_allclose(host(gf1), ogf, rtol=1e-5, atol=1e-4)


def test_backward_blocks_whose_boxes_do_not_fit(S, oracle):
    """grad_tile_kernel, third path (round 6): a flow that rotates and stretches every 8 x 64 block (destination boxes far above the
    4096 LDS cells, rows bent) takes the direct gathers with the two corners of a destination row as ONE 4-byte-aligned 8-byte load.
    gradInput bit-identical to the oracle, both-gradient launch = the separate launches; the pair's edge cases are planted: the
    plane's first pixel reached from x0 = -1 (pair shifted right), its last pixel reached with x0 + 1 past the row (pair shifted left),
    the same one row up for the bottom pair, and destinations outside the image."""
    from slr_sfs_amd._lib import check, lib, ptr, stream_of
    N, C, H, W = 2, 65, 160, 264
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    flows = []
    for n, (deg, sc) in enumerate(((55.0, 2.2), (-60.0, 2.4))):
        a = np.deg2rad(deg)
        cx, cy = W / 2 + 3.3 * n, H / 2 - 1.7
        X = cx + sc * (np.cos(a) * (xx - cx) - np.sin(a) * (yy - cy)) + 0.37
        Y = cy + sc * (np.sin(a) * (xx - cx) + np.cos(a) * (yy - cy)) + 0.21
        flows.append(np.stack([X - xx, Y - yy]))
    flow = np.stack(flows).astype(np.float32)
    # the kernel's rule on the host: blocks of the image centre have two strip boxes of more than 4096 cells together (third path)
    x0, y0 = np.floor(xx + flow[0, 0]).astype(int), np.floor(yy + flow[0, 1]).astype(int)
    cells = sum((x0[48:56, q:q + 32].max() - x0[48:56, q:q + 32].min() + 2) * (y0[48:56, q:q + 32].max() - y0[48:56, q:q + 32].min() + 2) for q in (128, 160))
    assert cells > 4096 and x0[48:56, 128:192].min() > 0 and x0[48:56, 128:192].max() < W - 2, cells

    def plant(n, y, x, tx, ty):
        flow[n, 0, y, x] = tx - x
        flow[n, 1, y, x] = ty - y
    plant(0, 50, 140, -0.5, 0.25)                # x0 = -1, y0 = 0: only NE / SE corners, top pair starts before the plane
    plant(0, 51, 150, W - 0.5, H - 0.75)         # x0 = W-1, y0 = H-1: only NW, top pair ends past the plane
    plant(0, 52, 160, W - 0.25, H - 1.5)         # x0 = W-1, y0 = H-2: bottom pair ends past the plane
    plant(1, 60, 130, -0.75, -0.5)               # x0 = -1, y0 = -1: only SE = the plane's first pixel (bottom pair before the plane)
    plant(1, 61, 131, -7.0, 3.0)                 # outside
    plant(1, 62, 132, 12.0, H + 4.0)             # outside
    rng = np.random.default_rng(77)
    x, go = rng.standard_normal((N, C, H, W)).astype(np.float32), rng.standard_normal((N, C, H, W)).astype(np.float32)
    Xd, F, G = dev(x), dev(flow), dev(go)
    gi1, gf1, gi2, gf2 = torch.empty_like(Xd), torch.empty_like(F), torch.empty_like(Xd), torch.empty_like(F)
    L, st = lib(), stream_of(Xd)
    check(L.slr_softsplat_backward(ptr(Xd), ptr(F), ptr(G), ptr(gi1), ptr(gf1), N, C, H, W, st), "both")
    check(L.slr_softsplat_backward(ptr(Xd), ptr(F), ptr(G), ptr(gi2), None, N, C, H, W, st), "input")
    check(L.slr_softsplat_backward(ptr(Xd), ptr(F), ptr(G), None, ptr(gf2), N, C, H, W, st), "flow")
    assert torch.equal(gi1, gi2) and torch.equal(gf1, gf2)
    ogi, ogf = oracle.softsplat_backward(x, flow, go)
    assert np.array_equal(host(gi1), ogi)
    assert np.abs(ogi[0, :, 50, 140]).max() > 0 and np.abs(ogi[0, :, 51, 150]).max() > 0 and np.abs(ogi[1, :, 60, 130]).max() > 0
    scale = max(1.0, float(np.abs(ogf).max()))
    np.testing.assert_allclose(host(gf1), ogf, rtol=2e-6, atol=2e-6 * scale)


def test_backward_channel_groups_on_small_grids(S, oracle):
    """slr_softsplat_backward_ws (round 6): on grids smaller than the chip -- the reference's training crops, [2,65,256,256] -- the
    backward kernel's channels are dealt to 2-4 workgroups per tile; gradInput stays bit-identical (per channel), gradFlow is the groups'
    partial sums added in order (rounding of the grouping only).  Through the C ABI with and without scratch, and through autograd."""
    from slr_sfs_amd._lib import check, lib, ptr, stream_of
    L = lib()
    assert L.slr_softsplat_backward_ws_bytes(1, 65, 768, 1280) == 2 * 768 * 1280 * 4   # larger than the chip: two groups, group 0 writes gradFlow itself
    assert L.slr_softsplat_backward_ws_bytes(2, 65, 256, 256) == 3 * 2 * 2 * 256 * 256 * 4   # four groups
    for (N, C, H, W) in ((2, 65, 256, 256), (1, 64, 128, 240), (1, 13, 40, 100), (3, 9, 64, 64)):
        nb = int(L.slr_softsplat_backward_ws_bytes(N, C, H, W))
        assert (nb > 0) == (C >= 16), (N, C, H, W, nb)
        rng = np.random.default_rng(N * 100 + C)
        flow = np.concatenate([oracle.euler_integration(smooth_motion(H, W, n, amp=2.0), 20 + 9 * n)[0] for n in range(N)])
        x, go = rng.standard_normal((N, C, H, W)).astype(np.float32), rng.standard_normal((N, C, H, W)).astype(np.float32)
        X, F, G = dev(x), dev(flow), dev(go)
        gi1, gf1, gi2, gf2 = torch.empty_like(X), torch.empty_like(F), torch.empty_like(X), torch.empty_like(F)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
        st = stream_of(X)
        check(L.slr_softsplat_backward_ws(ptr(X), ptr(F), ptr(G), ptr(gi1), ptr(gf1), N, C, H, W, ptr(ws), nb, st), "groups")
        check(L.slr_softsplat_backward(ptr(X), ptr(F), ptr(G), ptr(gi2), ptr(gf2), N, C, H, W, st), "one group")
        ogi, ogf = oracle.softsplat_backward(x, flow, go)
        assert torch.equal(gi1, gi2) and np.array_equal(host(gi1), ogi)
        scale = max(1.0, float(np.abs(ogf).max()))
        np.testing.assert_allclose(host(gf1), ogf, rtol=2e-6, atol=2e-6 * scale)
        np.testing.assert_allclose(host(gf2), ogf, rtol=1e-6, atol=1e-6 * scale)
        a, b = X.clone().requires_grad_(True), F.clone().requires_grad_(True)
        S.softsplat._FunctionSoftsplat.apply(a, b).backward(G)
        assert torch.equal(a.grad, gi1) and torch.equal(b.grad, gf1)


@pytest.mark.parametrize("shape", [(1, 65, 256, 480), (2, 7, 45, 131), (1, 16, 100, 64), (3, 1, 17, 70)])
def test_splat_sum_vs_oracle_euler_flow(S, oracle, shape):
    """Euler-integrated fluid flow (piles sources up -> multi-segment tiles + combine path),
    odd widths (scalar store path), batch > 1."""
    N, C, H, W = shape
    rng = np.random.default_rng(C)
    flow = np.concatenate([oracle.euler_integration(smooth_motion(H, W, n, amp=3.0), 40 + n)[0] for n in range(N)])
    x = rng.standard_normal(shape).astype(np.float32)
    out = host(S.FunctionSoftsplat(dev(x), dev(flow), None, "summation"))
    ref = oracle.softsplat_forward(x, flow)
    # piled-up flows sum hundreds of O(1) terms per pixel: bound the error by the fp32 rounding of
    # the accumulated magnitude (the splat of |x|), the only order-independent statement
    bound = 4e-6 * oracle.softsplat_forward(np.abs(x), flow) + 1e-6
    assert (np.abs(out - ref) <= bound).all(), float((np.abs(out - ref) - bound).max())


def test_splat_incoherent_flow_vs_oracle(S, oracle):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 13, 96, 200)).astype(np.float32)
    flow = rng.uniform(-8, 8, (1, 2, 96, 200)).astype(np.float32)
    out = S.FunctionSoftsplat(dev(x), dev(flow), None, "summation")
    np.testing.assert_allclose(host(out), oracle.softsplat_forward(x, flow), **TOL)


def test_splat_all_into_one_tile(S, oracle):
    """Every source lands in one output tile: the bin is far longer than the partial budget."""
    H, W = 160, 256
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    flow = np.stack([(W / 2 - x) * 0.95 + 0.3, (H / 2 - y) * 0.95 - 0.2])[None].astype(np.float32)
    v = np.random.default_rng(1).standard_normal((1, 3, H, W)).astype(np.float32)
    out = S.FunctionSoftsplat(dev(v), dev(flow), None, "summation")
    ref = oracle.softsplat_forward(v, flow)
    np.testing.assert_allclose(host(out), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def test_splat_nonfinite_flow_and_input(S, oracle):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 4, 40, 72)).astype(np.float32)
    flow = rng.uniform(-2, 2, (1, 2, 40, 72)).astype(np.float32)
    flow[0, 0, 3, 5] = np.nan
    flow[0, 1, 7, 9] = np.inf
    flow[0, 0, 8, 1] = 3e9
    out = host(S.FunctionSoftsplat(dev(x), dev(flow), None, "summation"))
    np.testing.assert_allclose(out, oracle.softsplat_forward(x, flow), **TOL)
    x[0, 1, 20, 63] = np.inf          # lands across a tile edge: must pollute only its own corners
    flow[0, :, 20, 63] = (0.5, 0.5)
    out = host(S.FunctionSoftsplat(dev(x), dev(flow), None, "summation"))
    ref = oracle.softsplat_forward(x, flow)
    assert np.array_equal(np.isfinite(out), np.isfinite(ref))


def test_splat_asserts(S):
    z = torch.zeros
    with pytest.raises(AssertionError):
        S.FunctionSoftsplat(z(1, 3, 8, 8).cuda(), z(1, 3, 8, 8).cuda(), None, "summation")    # flow depth (:397)
    with pytest.raises(AssertionError):
        S.FunctionSoftsplat(z(1, 3, 8, 8).cuda(), z(1, 2, 8, 9).cuda(), None, "summation")    # width (:399)
    with pytest.raises(AssertionError):
        S.FunctionSoftsplat(z(1, 3, 8, 8).cuda(), z(1, 2, 8, 8).cuda(), None, "median")       # mode (:667)
    with pytest.raises(AssertionError):
        S.FunctionSoftsplat(z(1, 3, 8, 8).cuda(), z(1, 2, 8, 8).cuda(), z(1, 2, 8, 8).cuda(), "softmax")  # metric (:666)
    with pytest.raises(AssertionError):
        S.FunctionSoftsplat(z(1, 3, 8, 16).cuda()[:, :, :, ::2], z(1, 2, 8, 8).cuda(), None, "summation")  # contiguous (:401)
    with pytest.raises(NotImplementedError):
        S.FunctionSoftsplat(z(1, 3, 8, 8), z(1, 2, 8, 8), None, "summation")                  # CPU (:418-419)


# ------------------------------------------------------------------------------ modes / max family

def test_function_softsplat_modes_golden(S, golden_dir):
    g = load(golden_dir, "splat_modes")
    for i in range(int(g["count"])):
        tag = str(g[f"c{i}_tag"])
        out = S.FunctionSoftsplat(dev(g[f"c{i}_in"]), dev(g[f"c{i}_flow"]), dev(g[f"c{i}_metric"]),
                                  str(g[f"c{i}_mode"]))
        np.testing.assert_allclose(host(out), g[f"c{i}_out"], err_msg=tag, rtol=1e-4, atol=1e-5)
    mod = S.ModuleSoftsplat("summation")
    out = mod(tenInput=dev(g["module_in"]), tenFlow=dev(g["module_flow"]),
              tenMetric=torch.ones(1, 1, 12, 20).cuda())
    np.testing.assert_allclose(host(out), g["module_out"], **TOL)


def test_function_softsplat_modes_autograd_path_matches_fused(S):
    """The differentiable composition gives the fused kernel's output, and its gradients w.r.t. input, flow and metric are those of
    the float64 definition (tests/test_gpu_gradients.py: check_mode_gradients, its criterion and its condition on the inputs)."""
    from test_gpu_gradients import check_mode_gradients
    rng = np.random.default_rng(3)
    x, fl = dev(rng.standard_normal((1, 6, 40, 72))), dev(rng.uniform(-3, 3, (1, 2, 40, 72)))
    met = dev(rng.standard_normal((1, 1, 40, 72)))
    go = rng.standard_normal((1, 6, 40, 72)).astype(np.float32)
    for mode in ("average", "linear", "softmax"):
        m = met.abs() + 0.1 if mode == "linear" else met
        fused = S.FunctionSoftsplat(x, fl, m, mode)
        xg = x.clone().requires_grad_(True)
        comp = S.FunctionSoftsplat(xg, fl, m, mode)
        np.testing.assert_allclose(host(comp), host(fused), rtol=1e-4, atol=1e-5)
        comp.sum().backward()
        assert torch.isfinite(xg.grad).all()
        assert check_mode_gradients(S, host(x), host(fl), host(m), mode, go, "parity 1x6x40x72"), "condition on the inputs"


def test_max_splat_family_golden(S, golden_dir):
    g = load(golden_dir, "splat_max")
    for i in range(int(g["count"])):
        tag = str(g[f"c{i}_tag"])
        x, fl = dev(g[f"c{i}_in"]), dev(g[f"c{i}_flow"])
        assert np.array_equal(host(S.ModuleMaximumsplat()(x, fl)), g[f"c{i}_max"]), tag
        assert np.array_equal(host(S.ModuleMaximumWarpNormsplat()(x, fl)), g[f"c{i}_warpnorm"]), tag


def test_splat_normalize(S):
    rng = np.random.default_rng(4)
    acc = rng.standard_normal((2, 5, 9, 33)).astype(np.float32)
    acc[:, -1] = np.abs(acc[:, -1])
    acc[0, -1, 2, 3] = 0.0
    a = S.softsplat.splat_normalize(dev(acc), "zero_to_one")
    n = acc[:, -1:].copy(); n[n == 0] = 1
    np.testing.assert_allclose(host(a), acc[:, :-1] / n, rtol=1e-6, atol=0)
    b = S.softsplat.splat_normalize(dev(acc), "clamp", 1e-8)
    np.testing.assert_allclose(host(b), acc[:, :-1] / np.maximum(acc[:, -1:], 1e-8), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------ forward_flow block

@pytest.mark.parametrize("t", [0, 1, 30, 59])
def test_forward_flow_decoder_input_golden(S, golden_dir, t):
    g = load(golden_dir, "pipeline_a6")
    N = int(g["N"])
    fs, Z, motion = dev(g["fs"]), dev(g["Z"]), dev(g["motion"])
    gen = host(S.synthesis.ClipSynthesizer(fs, Z, motion, N).features(t))
    ref = g[f"baseline_t{t}_gen_fs"]
    np.testing.assert_allclose(gen, ref, rtol=1e-4, atol=1e-5)
    assert np.array_equal(gen == 0, ref == 0)            # holes exactly 0 (decoder mask is x != 0)
    a = g["alpha_out"]
    abg = torch.sigmoid(dev(a[:, 0:1]))
    for tag, a0 in (("v1", True), ("v1noa0", False)):
        if f"{tag}_t{t}_gen_fs" not in g:
            continue
        cs = S.synthesis.ClipSynthesizer(fs, Z, motion, N, alpha_fluid_logit=dev(a[:, 1:2]), alpha_bg=abg,
                                         use_alpha0=a0)
        gen, afl = cs.features(t)
        np.testing.assert_allclose(host(gen), g[f"{tag}_t{t}_gen_fs"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(host(torch.cat([gen, afl], 1)), g[f"{tag}_t{t}_dec_alpha_in"],
                                   rtol=1e-4, atol=2e-5)


def test_synthesis_vs_oracle_mid_size(S, oracle):
    """256x480 (config C2's grid), 64 features, all frames of a short clip, vs the oracle."""
    H, W, N = 256, 480, 12
    rng = np.random.default_rng(11)
    fs = rng.standard_normal((1, 64, H, W)).astype(np.float32)
    Z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    m = smooth_motion(H, W, 3, amp=4.0)
    cs = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N)
    for t in (0, 5, 11):
        np.testing.assert_allclose(host(cs.features(t)), oracle.synth_baseline(fs, Z, m, t, N),
                                   rtol=1e-4, atol=1e-5)


def test_clip_plans_in_chunks_and_for_unannounced_frames(S, oracle, monkeypatch):
    """MotionPlan bins / plans a clip in chunks of PLAN_CHUNK frames (32-bit list offsets; bounds the plan buffer): with
    a chunk of 3 frames an 8-frame clip takes three plans; a rank that announced only some frames (sharded job) gets a
    one-frame plan built on demand for any other frame.  Every frame against the oracle, and plan-independent."""
    H, W, N = 48, 136, 8
    rng = np.random.default_rng(21)
    fs = rng.standard_normal((1, 9, H, W)).astype(np.float32)
    Z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    m = smooth_motion(H, W, 5, amp=3.0)
    whole = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N)
    monkeypatch.setattr(S.synthesis, "PLAN_CHUNK", 3)
    chunked = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N)
    assert len({id(rec["plan"]) for rec, _ in chunked.plan._where.values()}) == 3
    sharded = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N, frames=[1, 5])
    assert sorted(sharded.plan._where) == [1, 5]
    for t in range(N):
        ref = oracle.synth_baseline(fs, Z, m, t, N)
        for cs in (whole, chunked, sharded):
            np.testing.assert_allclose(host(cs.features(t)), ref, rtol=1e-4, atol=1e-5, err_msg=str(t))
    assert sorted(sharded.plan._where) == list(range(N))             # the other six were planned on demand


def test_batched_frames_in_one_launch_vs_oracle(S, oracle):
    """features_batch: the frames of a decoder batch go through ONE launch of the tile kernel (and one of combine) per
    weight group -- baseline and SLR v1, batches of 1-4 and a ragged tail, a converging field (multi-segment tiles in
    several frames of the same launch: one partial-tile area per frame), frames from two plan chunks in one call."""
    H, W, N = 56, 200, 11
    rng = np.random.default_rng(33)
    fs = rng.standard_normal((1, 16, H, W)).astype(np.float32)
    Z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    dx, dy = W * 0.5 - x, H * 0.5 - y
    r = np.sqrt(dx * dx + dy * dy) + 1e-3
    conv = np.stack([dx / r * np.minimum(r, 2.0), dy / r * np.minimum(r, 2.0)])[None].astype(np.float32)
    afl = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    abg = rng.uniform(0.05, 0.95, (1, 1, H, W)).astype(np.float32)
    for m in (smooth_motion(H, W, 2, amp=3.0), conv):
        base = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N)
        ts = [0, 3, 4, 10, 7, 1, 9]                                   # 4 + 3 frames, any order
        out = torch.empty(len(ts), 16, H, W, device="cuda")
        base.features_batch(ts, out)
        for k, t in enumerate(ts):
            np.testing.assert_allclose(host(out[k:k + 1]), oracle.synth_baseline(fs, Z, m, t, N), rtol=2e-4, atol=2e-5,
                                       err_msg=str(t))
        v1 = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N, alpha_fluid_logit=dev(afl), alpha_bg=dev(abg))
        out = torch.empty(3, 16, H, W, device="cuda")
        oa = torch.empty(3, 1, H, W, device="cuda")
        v1.features_batch([2, 5, 8], out, oa)
        for k, t in enumerate([2, 5, 8]):
            rg, ra, _ = oracle.synth_v1(fs, Z, afl, abg, m, t, N)
            np.testing.assert_allclose(host(out[k:k + 1]), rg, rtol=2e-4, atol=2e-5)
            np.testing.assert_allclose(host(oa[k:k + 1]), ra, rtol=2e-4, atol=2e-5)
    # frames that live in different chunks of the plan are split into separate launches
    import slr_sfs_amd.synthesis as syn
    old = syn.PLAN_CHUNK
    syn.PLAN_CHUNK = 2
    try:
        cs = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(conv), N)
    finally:
        syn.PLAN_CHUNK = old
    out = torch.empty(4, 16, H, W, device="cuda")
    cs.features_batch([1, 2, 3, 4], out)
    for k, t in enumerate([1, 2, 3, 4]):
        np.testing.assert_allclose(host(out[k:k + 1]), oracle.synth_baseline(fs, Z, conv, t, N), rtol=2e-4, atol=2e-5)


def test_batched_launch_with_whole_tile_items(S, oracle):
    """A motion field that puts every source pixel onto the corner shared by four tiles after one step: 4 x H x W bin
    entries in four tiles, more segments than partial-tile slots -> whole-tile items.  In a batched launch each such
    frame gets its own whole-tile kernel behind the shared main launch; the other frames of the batch are ordinary."""
    H, W, N = 320, 640, 3
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    m = np.stack([W / 2 - x - 0.5, H / 2 - y - 0.5])[None].astype(np.float32)
    rng = np.random.default_rng(8)
    fs = rng.standard_normal((1, 5, H, W)).astype(np.float32)
    Z = (rng.standard_normal((1, 1, H, W)) * 0.3).astype(np.float32)
    cs = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N)
    ts = [1, 0, 2]
    hints = [cs.plan.lookup(t)[3] for t in ts]
    # (round 4: a piece of more than a segment is found by its workgroup at run time and walked by the pass-by-pass launch behind the
    #  main one -- the plan no longer knows; frames 1 and 2 pile 4 x H x W entries and overflowing row lists into four tiles)
    assert all(h >= (H // 8) * (W // 64) for h in hints), hints
    out = torch.empty(len(ts), 5, H, W, device="cuda")
    cs.features_batch(ts, out)
    for k, t in enumerate(ts):
        ref = oracle.synth_baseline(fs, Z, m, t, N)
        np.testing.assert_allclose(host(out[k:k + 1]), ref, rtol=1e-3, atol=1e-4 * max(1.0, float(np.abs(ref).max())), err_msg=str(t))
        np.testing.assert_allclose(host(cs.features(t)), host(out[k:k + 1]), rtol=1e-3, atol=1e-4)


def test_randomised_synthesis_vs_oracle(S, oracle):
    """Seeded sweep of the headline path itself -- all-frames Euler integration, two-direction exp-weighted splat,
    normalisation (animating_softmax_splating.py:847-924; SLR v1: ..._2layers_alpha_seperate.py:950-1045) -- over
    grids, clip lengths, frame indices and motion families, baseline and SLR-v1 packing, against the oracle."""
    rng = np.random.default_rng(int(os.environ.get("SLR_TEST_SEED", 5)))
    for case in range(int(os.environ.get("SLR_TEST_CASES", 12))):
        H, W = int(rng.integers(3, 100)), int(rng.integers(3, 170))
        N = int(rng.integers(2, 14))
        C = int(rng.integers(1, 70))
        y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        kind = case % 4
        if kind == 0:
            m = smooth_motion(H, W, case, amp=float(rng.uniform(0.5, 5)))
        elif kind == 1:
            m = rng.uniform(-6, 6, (1, 2, H, W)).astype(np.float32)
        elif kind == 2:                                  # converging field: long record lists, multi-segment tiles
            dx, dy = W * 0.5 - x, H * 0.5 - y
            r = np.sqrt(dx * dx + dy * dy) + 1e-3
            m = np.stack([dx / r * np.minimum(r, 3.0), dy / r * np.minimum(r, 3.0)])[None].astype(np.float32)
        else:                                            # everything leaves the image after a few steps
            m = np.full((1, 2, H, W), float(rng.uniform(2, 9)), np.float32)
        fs = rng.standard_normal((1, C, H, W)).astype(np.float32)
        Z = (rng.standard_normal((1, 1, H, W)) * float(rng.uniform(0.2, 3))).astype(np.float32)
        ts = sorted({0, N - 1, int(rng.integers(0, N))})
        cs = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N)
        for t in ts:
            ref = oracle.synth_baseline(fs, Z, m, t, N)
            scale = max(1.0, float(np.abs(ref).max()))
            np.testing.assert_allclose(host(cs.features(t)), ref, rtol=2e-4, atol=2e-5 * scale,
                                       err_msg=str((case, "baseline", H, W, N, C, kind, t)))
        if case % 3 == 0:                                # SLR v1 packing (with alpha0 as blending weight)
            afl = rng.standard_normal((1, 1, H, W)).astype(np.float32)
            abg = rng.uniform(0.05, 0.95, (1, 1, H, W)).astype(np.float32)
            c1 = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N, alpha_fluid_logit=dev(afl), alpha_bg=dev(abg))
            for t in ts:
                rg, ra = oracle.synth_v1(fs, Z, afl, abg, m, t, N)[:2]
                g, a = c1.features(t)
                scale = max(1.0, float(np.abs(rg).max()))
                np.testing.assert_allclose(host(g), rg, rtol=2e-4, atol=2e-5 * scale, err_msg=str((case, "v1 fs", t)))
                np.testing.assert_allclose(host(a), ra, rtol=2e-4, atol=2e-5, err_msg=str((case, "v1 alpha", t)))


# ------------------------------------------------------------------------------ full-size properties

def test_full_size_mass_conservation_and_linearity(S):
    """768x1280, C=65: size-independent properties (the oracle is too slow for every case here).
    sum_out == sum_in * (in-bounds weight of every source);  splat(a*x + y) == a*splat(x) + splat(y)."""
    H, W, C = 768, 1280, 65
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(1, C, H, W, device="cuda", generator=g)
    y = torch.randn(1, C, H, W, device="cuda", generator=g)
    m = dev(smooth_motion(H, W, 0))
    flow, _ = S.euler_integration(m, 30)
    out = S.FunctionSoftsplat(x, flow, None, "summation")
    # in-bounds weight per source pixel, computed independently with torch ops
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    X, Y = xx + flow[0, 0], yy + flow[0, 1]
    x0, y0 = torch.floor(X), torch.floor(Y)
    wsum = torch.zeros_like(X, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            cx, cy = x0 + dx, y0 + dy
            wx = (x0 + 1 - X) if dx == 0 else (X - x0)
            wy = (y0 + 1 - Y) if dy == 0 else (Y - y0)
            inb = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
            wsum += torch.where(inb, (wx * wy).double(), torch.zeros_like(wsum))
    expect = (x[0].double() * wsum).sum(dim=(1, 2))
    got = out[0].double().sum(dim=(1, 2))
    assert torch.allclose(got, expect, rtol=1e-6, atol=1e-2), (got - expect).abs().max()
    lin = S.FunctionSoftsplat(2.5 * x + y, flow, None, "summation")
    ref = 2.5 * out + S.FunctionSoftsplat(y, flow, None, "summation")
    assert (lin - ref).abs().max().item() < 1e-4
    # identity flow reproduces the input exactly
    ident = S.FunctionSoftsplat(x, torch.zeros_like(flow), None, "summation")
    assert torch.equal(ident, x)


def test_full_size_one_plane_vs_oracle(S, oracle):
    """768x1280 at the heaviest frame (t = 59): a few planes against the oracle."""
    H, W = 768, 1280
    m = smooth_motion(H, W, 1)
    flow = oracle.euler_integration(m, 59)[0]
    x = np.random.default_rng(2).standard_normal((1, 3, H, W)).astype(np.float32)
    out = S.FunctionSoftsplat(dev(x), dev(flow), None, "summation")
    np.testing.assert_allclose(host(out), oracle.softsplat_forward(x, flow), **TOL)


# ------------------------------------------------------------------------------ pipelines

class _Zeros(torch.nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.ch = ch

    def forward(self, x):
        return x.new_zeros(x.shape[0], self.ch, x.shape[2], x.shape[3])


@pytest.mark.parametrize("t", [0, 1, 30, 59])
def test_v1_compositing_golden(S, golden_dir, t):
    """PredImg / CompositeFluidAlpha of the reference's v1 forward_flow with zero decoders
    (fluid = tanh(0), alpha = sigmoid(0)): pins the compositing and the BG / alpha plumbing."""
    g = load(golden_dir, "pipeline_a6")
    N = int(g["N"])
    a = dev(g["alpha_out"])
    abg = torch.sigmoid(a[:, 0:1])
    an = S.pipeline.SLRv1Animator(decoder=_Zeros(3), alpha_decoder=_Zeros(1)).cuda()
    clip = S.synthesis.ClipSynthesizer(dev(g["fs"]), dev(g["Z"]), dev(g["motion"]), N,
                                       alpha_fluid_logit=a[:, 1:2].contiguous(), alpha_bg=abg)
    clip.bg, clip.alpha_bg = torch.tanh(dev(g["bg"])), abg
    out = an.frame(clip, t)
    np.testing.assert_allclose(host(out["PredImg"]), g[f"v1_t{t}_PredImg"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(out["CompositeFluidAlpha"]), g[f"v1_t{t}_CompositeFluidAlpha"],
                               rtol=1e-5, atol=1e-6)


class _FixedOut(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, x):
        return self.value


@pytest.mark.parametrize("tag", ["plain", "region", "clamp", "softmax", "fluidonly", "bgonly", "v1weights"])
def test_v1_forward_flow_batch_entry_vs_reference(S, golden_dir, tag):
    """SLRv1Animator.forward_flow(batch) -- the reference's batch keys and return dict
    (..._2layers_alpha_seperate.py:843-1108) -- against the return dict of the REFERENCE's forward_flow with the
    optional compositing paths on (alpha_region, clamp_alpha, use_alpha_softmax, use_fluid_alpha_only,
    use_bg_alpha_only, use_softmax_splatter_v1); the decoders / alpha encoder are the fixture's fixed maps."""
    from conftest import v1_surface_inputs
    from test_abi_and_host import V1_VARIANTS
    g = load(golden_dir, "pipeline_v1_surface")
    W, N, t = int(g["W"]), int(g["N"]), int(g["t"])
    d = {k: dev(v) for k, v in v1_surface_inputs(W).items()}
    an = S.pipeline.SLRv1Animator(decoder=_FixedOut(d["dec_out"]), alpha_decoder=_FixedOut(d["adec_out"]),
                                  alpha_encoder=_FixedOut(d["alpha_out"]), **V1_VARIANTS[tag]).cuda()
    batch = {"features": [(d["fs"], d["Z"])], "images": [d["img"]], "motions": [d["motion"]],
             "index": torch.tensor([[0, t, N - 1]]), "BGImg": [d["bg_raw"]]}
    if tag == "region":
        batch["alpha_region"] = d["alpha_region"]
    out = an.forward_flow(batch)
    assert sorted(out.keys()) == [str(k) for k in g[f"{tag}_keys"]]
    for k, v in out.items():
        ref = g[f"{tag}_{k}"] if f"{tag}_{k}" in g else g[f"plain_{k}"]
        np.testing.assert_allclose(host(v), ref, rtol=1e-4, atol=1e-5, err_msg=f"{tag} {k}")


def test_v1_synthesize_returns_the_runner_outputs(S):
    """synthesize(keys=...) stacks what test_v1_4eval_rawsize.py:240-284 writes (PredImg, FluidImg,
    CompositeFluidAlpha per frame, BGImg once) and agrees with frame() / the PredImg-only form."""
    H, W, N = 40, 72, 5
    torch.manual_seed(1)
    an = S.pipeline.SLRv1Animator().cuda().eval()
    img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
    m = dev(smooth_motion(H, W, 2, amp=2.0))
    outs = an.synthesize(img, m, N, keys=S.pipeline.SLRv1Animator.KEYS)
    assert outs["PredImg"].shape == (N, 3, H, W) and outs["FluidImg"].shape == (N, 3, H, W)
    assert outs["CompositeFluidAlpha"].shape == (N, 1, H, W) and outs["BGImg"].shape == (1, 3, H, W)
    # (two runs agree to rounding noise, not bit for bit: the order of a pixel's records depends on wave timing)
    assert torch.allclose(outs["PredImg"], an.synthesize(img, m, N), rtol=1e-4, atol=1e-5)
    clip = an.begin_clip(img, m, N)
    f3 = an.frame(clip, 3)
    for k in ("PredImg", "FluidImg", "CompositeFluidAlpha"):
        assert torch.allclose(outs[k][3], f3[k][0], rtol=1e-4, atol=1e-5)
    assert all(bool(torch.isfinite(v).all()) for v in outs.values())


def test_baseline_forward_flow_api_and_clip(S, oracle):
    """forward_flow(batch) (reference batch keys) == begin_clip/frame == oracle features + decoder."""
    H, W, N = 40, 72, 9
    torch.manual_seed(0)
    an = S.pipeline.BaselineAnimator().cuda().eval()
    img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
    m = dev(smooth_motion(H, W, 4, amp=2.0))
    clip = an.begin_clip(img, m, N)
    fs, Z = an.encoder(img)
    frames = an.synthesize(img, m, N)
    assert frames.shape == (N, 3, H, W) and torch.isfinite(frames).all()
    for t in (0, 4, 8):
        ref_feat = oracle.synth_baseline(host(fs), host(Z), host(m), t, N)
        np.testing.assert_allclose(host(clip.features(t)), ref_feat, rtol=1e-4, atol=1e-5)
        batch = {"features": [(fs, Z)], "images": [img], "motions": [m], "index": torch.tensor([[0, t, N - 1]])}
        pred = an.forward_flow(batch)["PredImg"]
        assert torch.allclose(pred[0], frames[t], atol=1e-5)
        # decoder applied to the oracle's features gives the same frame (<= 1e-4, north_star)
        ref_img = torch.tanh(an.projector(dev(ref_feat)))
        assert (ref_img[0] - frames[t]).abs().max().item() < 1e-4


# ------------------------------------------------------------------------------ decoder stages (f3)

def test_fused_decoder_stages_match_torch_definition(S):
    """slr_bn_relu_mask / slr_pconv_epilogue vs the torch composition in nets.py (same order of
    operations: bit-exact), float4 and scalar paths, all mask kinds."""
    nets = S.nets
    g = torch.Generator(device="cuda").manual_seed(3)
    for (N, C, H, W) in [(1, 8, 16, 24), (2, 5, 7, 9)]:
        x = torch.randn(N, C, H, W, device="cuda", generator=g)
        x[:, :, 2:5, 3:7] = 0
        scale = torch.rand(C, device="cuda", generator=g) + 0.5
        shift = torch.randn(C, device="cuda", generator=g)
        m1 = (torch.rand(N, 1, H, W, device="cuda", generator=g) > 0.3).float()
        mc = (torch.rand(N, C, H, W, device="cuda", generator=g) > 0.3).float()
        for mask in (None, m1, mc):
            ref = torch.relu(x * scale.view(1, -1, 1, 1) - shift.view(1, -1, 1, 1)) * ((x != 0).float() if mask is None else mask)
            assert torch.equal(nets.bn_relu_mask(x, scale, shift, mask), ref)
        assert torch.equal(nets.bn_relu_mask(x, scale, shift, False),
                           torch.relu(x * scale.view(1, -1, 1, 1) - shift.view(1, -1, 1, 1)))
        raw = torch.randn(N, C, H, W, device="cuda", generator=g)
        bias = torch.randn(C, device="cuda", generator=g)
        res = torch.randn(N, C, H, W, device="cuda", generator=g)
        box = torch.randint(0, 10, (N, 1, H, W), device="cuda", generator=g).float()
        umr = box * 3.0
        um = torch.clamp(umr, 0, 1)
        ratio = 27.0 / (umr + 1e-8) * um
        ref = (raw * ratio + bias.view(1, -1, 1, 1)) * um
        out, um_k = nets.pconv_epilogue(raw, bias, box, 3.0, 27.0)
        assert torch.equal(out, ref) and torch.equal(um_k, um)
        assert torch.equal(nets.pconv_epilogue(raw, bias, box, 3.0, 27.0, res)[0], ref + res)
        nxt = torch.relu(ref * scale.view(1, -1, 1, 1) - shift.view(1, -1, 1, 1)) * um
        assert torch.equal(nets.pconv_epilogue(raw, bias, box, 3.0, 27.0, next_bn=(scale, shift))[0], nxt)


def test_decoder_gpu_matches_cpu_definition(S):
    """Whole partial-conv decoder: device (fused matrix-core kernels) vs its torch definition on the CPU."""
    torch.manual_seed(5)
    dec = S.nets.DecoderPconv2(64, 3).eval()
    x = torch.randn(1, 64, 32, 48)
    x[:, :, 6:20, 10:30] = 0
    with torch.no_grad():
        with S.nets.cpu_reference():
            ref = dec(x)
        out = dec.cuda()(x.cuda()).cpu()
    assert (out - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()


# ------------------------------------------------------------------------------ edge shapes

@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 1, 7), (2, 3, 5, 1), (1, 1, 8, 64), (1, 17, 9, 65), (4, 2, 3, 5)])
def test_tiny_and_ragged_shapes(S, oracle, shape):
    N, C, H, W = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    flow = rng.uniform(-2.5, 2.5, (N, 2, H, W)).astype(np.float32)
    met = rng.standard_normal((N, 1, H, W)).astype(np.float32)
    np.testing.assert_allclose(host(S.FunctionSoftsplat(dev(x), dev(flow), None, "summation")),
                               oracle.softsplat_forward(x, flow), **TOL)
    np.testing.assert_allclose(host(S.FunctionSoftsplat(dev(x), dev(flow), dev(met), "softmax")),
                               oracle.function_softsplat(x, flow, met, "softmax"), rtol=1e-4, atol=1e-5)
    gi, gf = oracle.softsplat_backward(x, flow, x)
    a, b = dev(x).requires_grad_(True), dev(flow).requires_grad_(True)
    S.softsplat._FunctionSoftsplat.apply(a, b).backward(dev(x))
    assert np.array_equal(host(a.grad), gi)
    np.testing.assert_allclose(host(b.grad), gf, rtol=1e-6, atol=1e-6)
    if N == 1:
        m = rng.uniform(-1.5, 1.5, (1, 2, H, W)).astype(np.float32)
        d, v = S.euler_integration(dev(m), 4)
        od, ov = oracle.euler_integration(m, 4)
        assert np.array_equal(host(d), od) and np.array_equal(host(v), ov)


def test_streams_and_workspace_reuse(S, oracle):
    """Calls on a side stream, interleaved shapes (workspace cache keyed by stream/shape)."""
    rng = np.random.default_rng(8)
    xs = [rng.standard_normal((1, 4, 24, 40)).astype(np.float32), rng.standard_normal((1, 6, 17, 33)).astype(np.float32)]
    fl = [rng.uniform(-3, 3, (1, 2, 24, 40)).astype(np.float32), rng.uniform(-3, 3, (1, 2, 17, 33)).astype(np.float32)]
    side = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(side):
        dx, df = [dev(a) for a in xs], [dev(a) for a in fl]
        for rep in range(3):
            for i in (0, 1):
                outs.append((i, S.FunctionSoftsplat(dx[i], df[i], None, "summation")))
    side.synchronize()
    for i, o in outs:
        np.testing.assert_allclose(host(o), oracle.softsplat_forward(xs[i], fl[i]), **TOL)


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_softmax_splatter_variants_vs_oracle(S, oracle, variant):
    """--use_softmax_splatter_v1 (no shift) and _v2 (shift by the maximum-warp-norm splat of Z,
    animating_softmax_splating.py:849-853) against the oracle, with and without the Z clamp (:856-859)."""
    H, W, N = 48, 80, 10
    rng = np.random.default_rng(21)
    fs = rng.standard_normal((1, 64, H, W)).astype(np.float32)
    Z = (rng.standard_normal((1, 1, H, W)) * 2).astype(np.float32)
    m = smooth_motion(H, W, 6, amp=2.5)
    for clamp in (None, (-20.0, 20.0)):
        cs = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N, softmax_v1=(variant == "v1"),
                                         softmax_v2=(variant == "v2"), clamp_z=clamp)
        for t in (0, 4, 9):
            ref = oracle.synth_baseline(fs, Z, m, t, N, clamp_z=clamp, variant=variant)
            np.testing.assert_allclose(host(cs.features(t)), ref, rtol=2e-4, atol=2e-5)


def test_synthesize_is_reproducible(S):
    """synthesize() twice on the same clip: the features agree to summation-order noise (bins are filled in a
    non-deterministic order, like the reference's atomics), the frames to that noise through the decoder (measured
    6e-6 on this random-weight decoder; 1e-4 is the north star's budget)."""
    H, W, N = 40, 72, 7
    torch.manual_seed(1)
    for an in (S.pipeline.BaselineAnimator().cuda().eval(), S.pipeline.SLRv1Animator().cuda().eval()):
        img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
        m = dev(smooth_motion(H, W, 5, amp=2.0))
        order = [0, 2, 3, 6]
        a = an.synthesize(img, m, N, frames=order)
        for rep in range(3):
            b = an.synthesize(img, m, N, frames=order)
            assert (a - b).abs().max().item() < 1e-4, rep
        clip = an.begin_clip(img, m, N)
        for i, t in enumerate(order):
            f = an.frame(clip, t)
            f = f["PredImg"] if isinstance(f, dict) else f
            assert (a[i] - f[0]).abs().max().item() < 1e-4, t


def test_operators_from_concurrent_host_threads(S):
    """The boundary is re-entrant (DataParallel replicas call the operator from several Python threads):
    four host threads, each on its own HIP stream with its own inputs, run forward + backward of the operator and the
    fused synthesis at the same time; every result equals the one computed alone (workspaces are cached per stream,
    the error string is thread-local, launches carry no shared mutable state)."""
    import threading
    rng = np.random.default_rng(77)
    H, W, C = 37, 83, 6
    cases = []
    for i in range(4):
        x = dev(rng.standard_normal((2, C, H, W)).astype(np.float32))
        fl = dev(rng.uniform(-4, 4, (2, 2, H, W)).astype(np.float32))
        m = dev(rng.standard_normal((2, 1, H, W)).astype(np.float32))
        g = dev(rng.standard_normal((2, C, H, W)).astype(np.float32))
        cases.append((x, fl, m, g))

    def run(x, fl, m, g):
        x = x.clone().requires_grad_(True)
        fl = fl.clone().requires_grad_(True)
        y = S.FunctionSoftsplat(x, fl, None, "summation")
        y.backward(g)
        z = S.FunctionSoftsplat(x.detach(), fl.detach(), m, "softmax")
        return y.detach(), x.grad, fl.grad, z

    alone = [run(*c) for c in cases]
    torch.cuda.synchronize()
    got, errs = [None] * 4, []

    def worker(i):
        try:
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.default_stream())
            with torch.cuda.stream(st):
                for _ in range(5):
                    got[i] = run(*cases[i])
            st.synchronize()
        except Exception as e:                          # noqa: BLE001 -- reported below
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(4):
        for a, b, name in zip(alone[i], got[i], ("forward", "grad input", "grad flow", "softmax")):
            exact = name in ("grad input", "grad flow")                     # gathers: deterministic order
            assert (torch.equal(a, b) if exact else (a - b).abs().max().item() < 1e-4), (i, name)


def test_frame_is_graph_capturable(S):
    """One frame (Euler lookup, binning, fused splat, decoder) captured into a HIP graph and replayed: every launch
    goes to the caller's stream through the C ABI and nothing inside allocates or synchronises (workspaces and split
    weights are cached by the warm-up).  Replay reproduces the eager frame to summation-order noise."""
    H, W, N = 40, 72, 7
    torch.manual_seed(2)
    an = S.pipeline.BaselineAnimator().cuda().eval()
    img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
    m = dev(smooth_motion(H, W, 5, amp=2.0))
    with torch.no_grad():
        clip = an.begin_clip(img, m, N)
        ref = an.frame(clip, 3).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            an.frame(clip, 3)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = an.frame(clip, 3)
        for _ in range(3):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert (out - ref).abs().max().item() < 1e-4


def test_batched_frames_are_graph_capturable(S):
    """The batched path -- 7 frames through ONE launch of the tile kernel (their arguments travel as kernel arguments,
    no host memory is read at replay) and the decoder on the batch -- captured into a HIP graph and replayed."""
    H, W, N = 40, 72, 7
    torch.manual_seed(3)
    an = S.pipeline.BaselineAnimator().cuda().eval()
    img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
    m = dev(smooth_motion(H, W, 5, amp=2.0))
    ts = list(range(N))
    with torch.no_grad():
        clip = an.begin_clip(img, m, N)
        buf = torch.empty(N, 64, H, W, device="cuda")

        def run():
            clip.features_batch(ts, buf)
            return torch.tanh(an.projector(buf))
        ref = run().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run()
        for _ in range(3):
            out.zero_()
            buf.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert (out - ref).abs().max().item() < 1e-4
        for t in ts:                                         # and the batch equals the frames one at a time
            assert (ref[t:t + 1] - an.frame(clip, t)).abs().max().item() < 1e-4


def test_splat_next_to_concurrent_matrix_core_kernel(S):
    """The splat on a side HIP stream while a large matrix-core convolution runs on the caller's stream gives the
    sequential result.  Regression test of the round-1 finding: built WITH packed-fp32 instructions
    the tile kernel returned a few dozen wrong values (low halves of the v_pk_fma_f32 pairs) in 1-4 % of such
    launches -- 39 wrong frames of 4200, 0 of 4200 without them (csrc/Makefile NOPK); 280 frames here."""
    from slr_sfs_amd import nets
    from slr_sfs_amd.pipeline import _features_ahead
    H, W, N = 40, 72, 7
    torch.manual_seed(1)
    an = S.pipeline.BaselineAnimator().cuda().eval()
    img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
    m = dev(smooth_motion(H, W, 5, amp=2.0))
    order = [0, 2, 3, 6, 1, 4, 5]
    big = torch.randn(1, 64, 768, 1280, device="cuda")
    bigconv = nets.Conv(64, 64, 3).cuda()
    wrong = 0
    with torch.no_grad():
        for trial in range(40):
            clip = an.begin_clip(img, m, N)
            feats = []
            for gen_fs in _features_ahead(clip, order, overlap=True):
                feats.append(gen_fs.clone())
                bigconv(big)                                        # ~0.4 ms of MFMA work under the next frame's splat
            torch.cuda.synchronize()
            for i, t in enumerate(order):
                wrong += int((feats[i] - clip.features(t)).abs().max().item() > 1e-4)
    assert wrong == 0
    # and the whole pipeline with the option switched on
    a = an.synthesize(img, m, N, frames=order)
    b = an.synthesize(img, m, N, frames=order, overlap=True)
    assert (a - b).abs().max().item() < 1e-4


def test_banded_encoder_is_exact(S):
    """parallel.encode_band: the encoder on a band of rows + its 16-row halo gives, after the halo is cut off, the
    same BITS as the encoder on the whole image (what lets the ranks of a multi-GPU job share the per-clip encoder);
    with a halo that is too small it does not (the test can see the difference)."""
    from slr_sfs_amd import nets, parallel
    torch.manual_seed(11)
    img = torch.rand(1, 3, 152, 136, device="cuda") * 2 - 1
    with torch.no_grad():
        for enc in (nets.EncoderWithZ().cuda().eval(), nets.Encoder(3, 2).cuda().eval()):
            want = enc(img)
            want = torch.cat(want, 1) if isinstance(want, tuple) else want
            for world in (2, 4, 8):
                got = torch.cat([parallel.encode_band(enc, img, r, world)[0] for r in range(world)], 2)
                assert got.shape == want.shape and torch.equal(got, want), world
            short = torch.cat([parallel.encode_band(enc, img, r, 4, halo=6)[0] for r in range(4)], 2)
            assert not torch.equal(short, want)
        an = S.pipeline.BaselineAnimator().cuda().eval()
        m = torch.randn(1, 2, 152, 136, device="cuda")
        a = an.synthesize(img, m, 4, frames=[1, 3])
        b = an.synthesize(img, m, 4, frames=[1, 3], shard=(0, 1))
        assert (a - b).abs().max().item() < 1e-4


def test_repeated_frames_in_one_batch(S):
    """A frame list with repeats inside one 16-frame splat batch (a ping-pong loop; frames=[3, 3]): the reference's frame loop takes
    any index list (test_baseline_4eval_rawsize.py:234-245).  The tile launch renders each of its frames once, so the grouping closes
    a launch at a repeat: every output slot equals the frame rendered on its own, for both models."""
    torch.manual_seed(5)
    img = torch.rand(1, 3, 72, 136, device="cuda") * 2 - 1
    m = torch.randn(1, 2, 72, 136, device="cuda")
    N = 6
    with torch.no_grad():
        for an in (S.pipeline.BaselineAnimator().cuda().eval(), S.pipeline.SLRv1Animator().cuda().eval()):
            single = {t: an.synthesize(img, m, N, frames=[t]) for t in range(N)}
            for frames in ([0, 1, 1, 0], [3, 3], [0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0], [2, 2, 2, 5]):
                got = an.synthesize(img, m, N, frames=frames)
                assert got.shape[0] == len(frames)
                for k, t in enumerate(frames):
                    assert torch.allclose(got[k], single[t][0], rtol=0, atol=1e-4, equal_nan=True), (frames, k)   # (decoder batch of 1 vs n: other kernel tilings)


def _run_two_ranks(backend):
    import socket
    import subprocess
    import sys
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_two_rank_clip.py")
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2",
                   SLR_TEST_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, script], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0 and f"RANK{r} OK" in out, (r, out[-500:], err[-3000:])


def test_two_ranks_one_clip(S):
    """The multi-GPU job of bench.py / runner.py end to end with two processes (tests/_two_rank_clip.py): frames
    round-robin over the ranks; ONE all-gather of the finished clip (north_star form) and round-wise asynchronous assembly;
    encoder redundant and in row bands; a clip SHORTER than the world (a rank without frames still enters every
    collective); the 2-layer model's dict of outputs -- every rank ends with what a single process renders.  The test box
    has one GPU, so both ranks use cuda:0 and the collectives travel over gloo; test_two_ranks_on_rccl is the same on RCCL."""
    _run_two_ranks("gloo")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (enables itself on a multi-GPU node)")
def test_two_ranks_on_rccl(S):
    """tests/_two_rank_clip.py with backend nccl (= RCCL over xGMI), rank r on cuda:r: gather_clip, ClipAssembler and
    encode_banded on real device buffers of two GPUs, uneven shards (N = 7) and an empty one (N = 1)."""
    _run_two_ranks("nccl")


@pytest.mark.parametrize("form", [(), ("--assembly", "rounds", "--encoder", "banded"), ("--frames", "uint8")])
def test_bench_two_ranks_on_one_gpu(form):
    """bench.py's own multi-rank path, launched the way the driver launches it (torch.distributed.run, 2 ranks):
    warm-up, barrier-bracketed timed steps, MAX over ranks, rank 0's extra measurements while the other rank waits,
    ONE JSON line from rank 0.  One GPU here: both ranks on cuda:0, collectives over gloo (SLR_BENCH_ONE_GPU_GLOO=1),
    so the figure itself means nothing -- the control flow, the sharded clip and the JSON contract are what is checked."""
    import json
    import socket
    import subprocess
    import sys
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SLR_BENCH_ONE_GPU_GLOO="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                        "--gpus", "2", "--steps", "1", "--warmup", "1", "--full", *form], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["warmup"] == 1 and d["scaling"] == "strong"
    assert d["value"] > 0 and abs(d["value"] - 60 / (d["ms_per_step"] * 1e-3)) < 0.05 * d["value"]
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"] is None                       # rank 0 at N=1 only
    # the line says which multi-GPU form ran and what it moved: default = the north_star form (redundant encoder + ONE
    # all-gather of the finished clip), with the other form's figure beside it; explicit = per-round all-gathers + banded encoder
    cfg = d["config"]
    frame = 3 * 768 * 1280 * 4
    # ... and what the communicator itself reports: backend, world size, every rank's device and frames (ADVICE / VERDICT r3: a
    # scaling line has to prove how many ranks took part)
    com = d["communicator"]
    assert com["world_size"] == 2 and com["backend"] == "gloo" and [r["rank"] for r in com["ranks"]] == [0, 1]
    assert [r["frames"] for r in com["ranks"]] == [30, 30] and all(r["device_name"] for r in com["ranks"])
    if not form or form[0] == "--frames":
        assert cfg["assembly"] == "final" and cfg["encoder"] == "redundant"
        assert cfg["assembled_frames"] == ("uint8" if form else "fp32")
        assert cfg["collective_bytes_received_per_rank_per_clip"] == 30 * frame // (4 if form else 1)
        assert d["value_rounds_banded"]["value"] > 0
    else:
        assert cfg["assembly"] == "rounds" and cfg["encoder"] == "banded"
        assert cfg["collective_bytes_received_per_rank_per_clip"] == 30 * frame + 65 * 768 * 1280 * 4 // 2
        assert "value_rounds_banded" not in d


def test_bench_plain_run_and_dump_outputs(S, tmp_path):
    """A plain bench.py run (no --full): the timed steps and the line only, `steps` as asked, ms_per_step one timed step; with
    --dump-outputs the last timed step's clip as float32 .npy files within 64 MB, the frames equal to the sampled values."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 60 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    assert d["parity_err"] is None and d["cpu_baseline"] is None          # checks and baselines are --full's
    files = sorted(p.name for p in out.iterdir())
    assert files == ["clip_sample.npy", "frames.npy"]
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
    frames, sample = np.load(out / "frames.npy"), np.load(out / "clip_sample.npy")
    assert frames.dtype == np.float32 and frames.shape == (3, 3, 768, 1280) and np.isfinite(frames).all()
    assert sample.dtype == np.float32 and sample.shape == (1 << 20,) and np.isfinite(sample).all()
    assert np.abs(frames).max() <= 1.0 and frames.std() > 0                 # tanh frames, not a blank buffer
    pos = np.sort(np.random.default_rng(20261016).choice(60 * 3 * 768 * 1280, 1 << 20, replace=False))    # bench.dump_outputs
    per_frame = 3 * 768 * 1280
    for k, t in enumerate((0, 30, 59)):
        inside = (pos // per_frame) == t
        assert inside.any() and np.array_equal(sample[inside], frames[k].ravel()[pos[inside] % per_frame])


def test_clip_assembler_on_rccl(S, tmp_path):
    """parallel.ClipAssembler with backend nccl (= RCCL) in a child process: the asynchronous per-round collectives
    on RCCL's stream, the frames rendered on the caller's stream in between, finish() -> the clip.  One GPU here, so
    world_size 1 with the collective path forced; the 2-rank logic runs on gloo in tests/test_parallel_gloo.py."""
    import socket
    import subprocess
    import sys
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    script = tmp_path / "asm.py"
    script.write_text(
        "import os, sys, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
        "import slr_sfs_amd as S\n"
        "from slr_sfs_amd import parallel\n"
        f"os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='{port}', RANK='0', WORLD_SIZE='1')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))\n"
        "torch.manual_seed(3)\n"
        "an = S.pipeline.BaselineAnimator().cuda().eval()\n"
        "img = torch.rand(1, 3, 40, 72, device='cuda') * 2 - 1\n"
        "m = torch.randn(1, 2, 40, 72, device='cuda')\n"
        "ref = an.synthesize(img, m, 6)\n"
        "for rep in range(3):\n"
        "    asm = parallel.ClipAssembler(6, 0, 1, always_collective=True)\n"
        "    an.synthesize(img, m, 6, on_frame=asm.push)\n"
        "    clip = asm.finish()\n"
        "    torch.cuda.synchronize()\n"
        "    assert clip.shape == ref.shape and (clip - ref).abs().max().item() < 1e-4\n"
        "dist.destroy_process_group()\n"
        "print('ASSEMBLED')\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ASSEMBLED" in r.stdout, r.stderr[-2000:]


def test_multi_gpu_preflight_on_rccl(S, tmp_path):
    """Everything the N > 1 bench line runs on the communicator, on backend nccl (= RCCL) with the collectives FORCED at world size 1
    (the first real multi-GPU run must not be the first run of this code on RCCL): communicator_report (all_gather_object
    + device properties + RCCL version), gather_clip on fp32 frames and on the uint8 frames of frames_for_assembly
    (all_gather_into_tensor of padded shards + the reordering view), encode_banded (row band + all-gather of the band).  The 2 / 4 /
    8-rank logic of the same functions runs on gloo (tests/test_parallel_gloo.py)."""
    import socket
    import subprocess
    import sys
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    script = tmp_path / "preflight.py"
    script.write_text(
        "import os, sys, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
        "import slr_sfs_amd as S\n"
        "from slr_sfs_amd import parallel\n"
        f"os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='{port}', RANK='0', WORLD_SIZE='1')\n"
        "torch.cuda.set_device(0)\n"
        "dev = torch.device('cuda', 0)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)\n"
        "rep = parallel.communicator_report(dev, 7, 0.5)\n"
        "assert rep['backend'] == 'nccl' and rep['world_size'] == 1 and rep['distinct_devices'] == 1, rep\n"
        "assert rep['rccl_version'] and rep['ranks'][0]['frames'] == 7 and rep['ranks'][0]['device_name'], rep\n"
        "torch.manual_seed(5)\n"
        "frames = torch.rand(7, 3, 40, 72, device=dev) * 2 - 1\n"
        "clip = parallel.gather_clip(frames, 7, 0, 1, always_collective=True)\n"
        "assert clip.data_ptr() != frames.data_ptr() and torch.equal(clip, frames)\n"
        "u8 = parallel.frames_for_assembly(frames, (80, 144))\n"
        "assert u8.dtype == torch.uint8 and tuple(u8.shape) == (7, 80, 144, 3)\n"
        "assert torch.equal(parallel.gather_clip(u8, 7, 0, 1, always_collective=True), u8)\n"
        "an = S.pipeline.BaselineAnimator().cuda().eval()\n"
        "img = torch.rand(1, 3, 40, 72, device=dev) * 2 - 1\n"
        "with torch.no_grad():\n"
        "    want = an.encoder(img)\n"
        "    got = parallel.encode_banded(an.encoder, img, 0, 1, always_collective=True)\n"
        "want = want if isinstance(want, tuple) else (want,)\n"
        "got = got if isinstance(got, tuple) else (got,)\n"
        "assert len(want) == len(got) and all(torch.equal(a, b) for a, b in zip(want, got))\n"
        "torch.cuda.synchronize()\n"
        "dist.destroy_process_group()\n"
        "print('PREFLIGHT', rep['rccl_version'])\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PREFLIGHT" in r.stdout, r.stderr[-2000:]


def test_c_abi_from_a_plain_host_program(S, oracle, tmp_path):
    """examples/cabi_demo.cpp: a C++ host program with hipMalloc'ed buffers and its own stream, linked against the
    library through include/slr_splat.h only (no Python, no torch in the process) -- Euler integration, summation
    splat, fused softmax mode with the bins reused, and the per-clip path (clip plan + three frames in one launch); its
    outputs against the oracle."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "cabi_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples")])
    rng = np.random.default_rng(123)
    C, H, W, nsteps = 5, 61, 150, 7
    x = rng.standard_normal((1, C, H, W)).astype(np.float32)
    m = smooth_motion(H, W, 4, amp=2.5)
    met = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    for name, a in (("in", x), ("motion", m), ("metric", met)):
        a.tofile(tmp_path / f"{name}.f32")
    r = subprocess.run([exe, str(tmp_path / "in.f32"), str(tmp_path / "motion.f32"), str(tmp_path / "metric.f32"),
                        str(C), str(H), str(W), str(nsteps), str(tmp_path / "out_")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout, r.stderr)
    load = lambda n, shape: np.fromfile(tmp_path / f"out_{n}.f32", np.float32).reshape(shape)
    disp, vis = oracle.euler_integration(m, nsteps)
    assert np.array_equal(load("disp", (1, 2, H, W)), disp)
    assert np.array_equal(load("visible", (1, 1, H, W)), vis.reshape(1, 1, H, W))
    np.testing.assert_allclose(load("sum", (1, C, H, W)), oracle.softsplat_forward(x, disp), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(load("softmax", (1, C, H, W)), oracle.function_softsplat(x, disp, met, "softmax"),
                               rtol=2e-4, atol=2e-5)
    # the per-clip entry points from C: slr_euler_integrate_all x 2 -> slr_clip_plan_build -> three frames of the clip by ONE
    # slr_synth_group_clip_batch launch (N = nsteps + 3 frames; t = 1, N/2, N-1)
    N = nsteps + 3
    frames = load("frames", (3, C, H, W))
    for k, t in enumerate((1, N // 2, N - 1)):
        np.testing.assert_allclose(frames[k:k + 1], oracle.synth_baseline(x, met, m, t, N), rtol=2e-4, atol=2e-5, err_msg=str(t))


def test_c_abi_prebinned_reuse_and_errors(S, oracle):
    """Straight through ctypes: bin once, splat two tensors with the same bins (prebinned = 1);
    workspace too small / misaligned is refused with SLR_E_WORKSPACE."""
    from slr_sfs_amd._lib import lib, ptr, stream_of
    L = lib()
    rng = np.random.default_rng(31)
    N, C, H, W = 1, 5, 33, 70
    fl = rng.uniform(-3, 3, (N, 2, H, W)).astype(np.float32)
    xs = [rng.standard_normal((N, C, H, W)).astype(np.float32) for _ in range(2)]
    dfl = dev(fl)
    nbytes = int(L.slr_splat_workspace_bytes(N, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = stream_of(dfl)
    assert L.slr_splat_bin(ptr(dfl), N, H, W, ptr(ws), nbytes, st) == 0
    for x in xs:
        dx, out = dev(x), torch.empty(N, C, H, W, device="cuda")
        assert L.slr_softsplat_forward(ptr(dx), ptr(dfl), ptr(out), N, C, H, W, ptr(ws), nbytes, 1, st) == 0
        np.testing.assert_allclose(host(out), oracle.softsplat_forward(x, fl), **TOL)
    dx, out = dev(xs[0]), torch.empty(N, C, H, W, device="cuda")
    assert L.slr_softsplat_forward(ptr(dx), ptr(dfl), ptr(out), N, C, H, W, ptr(ws), nbytes // 2, 0, st) == -2
    assert b"workspace" in L.slr_last_error()
    off = ws[8:]                                              # 8-byte offset: not 16-byte aligned
    assert L.slr_softsplat_forward(ptr(dx), ptr(dfl), ptr(out), N, C, H, W, ptr(off), nbytes - 8, 0, st) == -2
    res, scratch = torch.empty(1, device="cuda"), torch.empty(1024, device="cuda")
    big = dev(rng.standard_normal(300001).astype(np.float32))
    assert L.slr_global_max(ptr(big), big.numel(), ptr(res), ptr(scratch), st) == 0
    assert float(res) == float(big.max())


def test_prebinned_pair_and_single_splats_share_their_bins_in_any_order(S, oracle):
    """Bins are reusable: bin a pair of flows once (slr_splat_bin_pair), then run the fused two-direction group on the
    pair AND the one-flow summation splat on each bin with prebinned = 1, in both orders -- the work plan of a splat
    (one bin: SEG_ONE segments, two bins: SEG_TWO) is rebuilt per call and must not depend on what ran before.  All
    three results against the oracle, on an Euler flow whose tiles split into several segments."""
    from slr_sfs_amd._lib import lib, ptr, stream_of
    L = lib()
    rng = np.random.default_rng(57)
    C, H, W = 5, 72, 200
    m = smooth_motion(H, W, 4, amp=3.0)
    ff = oracle.euler_integration(m, 45)[0]
    fp = oracle.euler_integration(-m, 30)[0]
    x = rng.standard_normal((1, C, H, W)).astype(np.float32)
    Z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    dff, dfp, dx, dZ = dev(ff), dev(fp), dev(x), dev(Z)
    st = stream_of(dx)
    nbytes = int(L.slr_splat_workspace_bytes(1, H, W))
    wsf, wsp = (torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))
    zmax = dZ.max().reshape(1)
    e = np.exp(Z - Z.max())
    alpha = 0.3
    S_f = oracle.softsplat_forward(np.concatenate([x * e * np.float32(alpha), e * np.float32(alpha)], 1), ff)
    S_p = oracle.softsplat_forward(np.concatenate([x * e * np.float32(1 - alpha), e * np.float32(1 - alpha)], 1), fp)
    nrm = S_f[:, -1:] + S_p[:, -1:]
    ref_pair = (S_f[:, :-1] + S_p[:, :-1]) / np.maximum(nrm, np.float32(1e-8))
    for order in (0, 1):
        assert L.slr_splat_bin_pair(ptr(dff), ptr(dfp), 1, H, W, ptr(wsf), ptr(wsp), nbytes, st) == 0
        outs = {}

        def pair():
            o = torch.empty(1, C, H, W, device="cuda")
            assert L.slr_synth_group(ptr(dx), ptr(dZ), ptr(zmax), 1, ptr(dff), ptr(dfp), alpha, ptr(o), None, C, H, W, 1e-8,
                                     ptr(wsf), ptr(wsp), nbytes, st) == 0, L.slr_last_error()
            outs["pair"] = o

        def singles():
            for tag, fl, ws in (("f", dff, wsf), ("p", dfp, wsp)):
                o = torch.empty(1, C, H, W, device="cuda")
                assert L.slr_softsplat_forward(ptr(dx), ptr(fl), ptr(o), 1, C, H, W, ptr(ws), nbytes, 1, st) == 0
                outs[tag] = o
        (pair, singles)[order]()
        (singles, pair)[order]()
        np.testing.assert_allclose(host(outs["f"]), oracle.softsplat_forward(x, ff), rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(host(outs["p"]), oracle.softsplat_forward(x, fp), rtol=1e-5, atol=2e-5)
        got = host(outs["pair"])
        mask = nrm[0, 0] > 1e-3                               # (tiny normalisers amplify the rounding of the sums)
        assert mask.mean() > 0.2
        np.testing.assert_allclose(got[:, :, mask], ref_pair[:, :, mask], rtol=2e-4, atol=2e-5)


def test_c_abi_clip_plan_entry_points_and_errors(S, oracle):
    """The per-clip entry points straight through ctypes: slr_clip_plan_bytes / _build / _totals,
    slr_synth_group_clip with and without the totals read back (exact grids vs upper-bound grids: same result),
    slr_synth_group_clip_batch; and their argument errors (codes + slr_last_error, nothing launched)."""
    import ctypes
    from slr_sfs_amd._lib import lib, ptr, stream_of
    L = lib()
    rng = np.random.default_rng(41)
    C, H, W, N = 6, 40, 136, 7
    fs = rng.standard_normal((1, C, H, W)).astype(np.float32)
    Z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    m = smooth_motion(H, W, 9, amp=3.0)
    dfs, dZ, dm = dev(fs), dev(Z), dev(m)
    st = stream_of(dfs)
    disp_f = torch.empty(N, 2, H, W, device="cuda")
    disp_p = torch.empty(N + 1, 2, H, W, device="cuda")
    assert L.slr_euler_integrate_all(ptr(dm), H, W, N - 1, 1.0, ptr(disp_f), None, st) == 0
    assert L.slr_euler_integrate_all(ptr(dm), H, W, N, -1.0, ptr(disp_p), None, st) == 0
    ts = [0, 2, 6]
    idx_f = torch.tensor(ts, dtype=torch.int32, device="cuda")
    idx_p = torch.tensor([N - t for t in ts], dtype=torch.int32, device="cuda")
    nb = len(ts)
    pbytes = int(L.slr_clip_plan_bytes(nb, H, W))
    assert pbytes > 0 and int(L.slr_clip_plan_bytes(0, H, W)) == 0
    assert int(L.slr_clip_plan_bytes(70000, 768, 1280)) == 0              # at most 16384 frames per plan
    plan = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.slr_clip_plan_build(ptr(disp_f), vp(idx_f), ptr(disp_p), vp(idx_p), nb, H, W, ptr(plan), pbytes // 2, st) == -2
    assert b"plan buffer" in L.slr_last_error()
    assert L.slr_clip_plan_build(ptr(disp_f), vp(idx_f), ptr(disp_p), vp(idx_p), nb, H, W, ptr(plan), pbytes, st) == 0
    off, stride = ctypes.c_size_t(), ctypes.c_int()
    assert L.slr_clip_plan_totals(nb, H, W, ctypes.byref(off), ctypes.byref(stride)) == 0
    totals = plan[off.value:off.value + nb * stride.value * 4].view(torch.int32).view(nb, stride.value).cpu()
    tiles = ((H + 7) // 8) * ((W + 63) // 64)
    assert all(int(totals[i, 0]) >= tiles for i in range(nb))             # at least one work item per tile
    zmax = dZ.max().reshape(1).contiguous()
    refs = [oracle.synth_baseline(fs, Z, m, t, N) for t in ts]
    alphas = [1.0 - t / N for t in ts]
    for k, t in enumerate(ts):                                             # one frame per call, exact and upper-bound grids
        for n_items in (int(totals[k, 0]), -1):
            out = torch.empty(1, C, H, W, device="cuda")
            assert L.slr_synth_group_clip(ptr(dfs), ptr(dZ), ptr(zmax), 1, ptr(disp_f[t]), ptr(disp_p[N - t]), alphas[k],
                                          ptr(out), None, C, H, W, 1e-8, ptr(plan), pbytes, nb, k, n_items, st) == 0
            np.testing.assert_allclose(host(out), refs[k], rtol=2e-4, atol=2e-5)
    outs = torch.empty(nb, C, H, W, device="cuda")                        # all three frames in one launch
    PP = ctypes.c_void_p * nb
    df, dp = PP(*[disp_f[t].data_ptr() for t in ts]), PP(*[disp_p[N - t].data_ptr() for t in ts])
    po = PP(*[outs[k].data_ptr() for k in range(nb)])
    al = (ctypes.c_float * nb)(*alphas)
    fr = (ctypes.c_int * nb)(*range(nb))
    call = lambda n_, fr_, ni_=None: L.slr_synth_group_clip_batch(ptr(dfs), ptr(dZ), ptr(zmax), 1, df, dp, al, po, None, C, H, W, 1e-8,
                                                                  ptr(plan), pbytes, nb, fr_, n_, ni_, st)
    assert call(nb, fr) == 0
    for k in range(nb):
        np.testing.assert_allclose(host(outs[k:k + 1]), refs[k], rtol=2e-4, atol=2e-5)
    assert call(17, fr) == -1 and b"frames per launch" in L.slr_last_error()
    assert call(nb, (ctypes.c_int * nb)(0, 1, 5)) == -1 and b"frame index" in L.slr_last_error()
    assert call(nb, (ctypes.c_int * nb)(0, 1, 1)) == -1 and b"twice" in L.slr_last_error()      # (a frame's deferred list is per frame)
    assert call(nb, fr, (ctypes.c_int * nb)(*[int(totals[k, 0]) for k in range(nb)])) == 0      # exact grids from the totals
    for k in range(nb):
        np.testing.assert_allclose(host(outs[k:k + 1]), refs[k], rtol=2e-4, atol=2e-5)
    assert L.slr_synth_group_clip_batch(ptr(dfs), ptr(dZ), ptr(zmax), 1, df, dp, al, po, None, C, H, W, 1e-8, ptr(plan), pbytes // 2,
                                        nb, fr, nb, None, st) == -2 and b"plan needs" in L.slr_last_error()


def test_splat_over_budget_tiles_whole_tile_path(S, oracle):
    """More segments than partial-tile slots (everything converges into one tile of a larger
    image): the over-budget tile is walked segment by segment by one workgroup (WHOLE kernel)."""
    H, W = 320, 640
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    flow = np.stack([(W / 2 - x) * 0.97 + 0.3, (H / 2 - y) * 0.97 - 0.2])[None].astype(np.float32)
    rng = np.random.default_rng(4)
    v = rng.standard_normal((1, 9, H, W)).astype(np.float32)
    met = (rng.standard_normal((1, 1, H, W)) * 0.5).astype(np.float32)
    ref = oracle.softsplat_forward(v, flow)
    out = host(S.FunctionSoftsplat(dev(v), dev(flow), None, "summation"))
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    refn = oracle.function_softsplat(v, flow, met, "softmax")
    outn = host(S.FunctionSoftsplat(dev(v), dev(flow), dev(met), "softmax"))
    np.testing.assert_allclose(outn, refn, rtol=1e-3, atol=1e-4)
    mx = host(S.ModuleMaximumsplat()(dev(v), dev(flow)))
    assert np.array_equal(mx, oracle.maxsplat_forward(v, flow))


@pytest.mark.parametrize("kind", ["row", "column", "shrink"])
def test_splat_collapsing_flows_vs_oracle(S, oracle, kind):
    """Everything collapses onto one row / one column / a 4x smaller image: long bins, many
    segments per tile, partial tiles + combine (and the whole-tile path when slots run out)."""
    H, W = 200, 328
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    z = np.zeros_like(x)
    flow = {"row": np.stack([z, (H / 2 - y) * 0.999 - 0.2]),
            "column": np.stack([(W / 2 - x) * 0.999 + 0.3, z]),
            "shrink": np.stack([(W / 2 - x) * 0.75, (H / 2 - y) * 0.75])}[kind][None].astype(np.float32)
    v = np.random.default_rng(7).standard_normal((1, 10, H, W)).astype(np.float32)
    ref = oracle.softsplat_forward(v, flow)
    out = host(S.FunctionSoftsplat(dev(v), dev(flow), None, "summation"))
    bound = 4e-6 * oracle.softsplat_forward(np.abs(v), flow) + 1e-6
    assert (np.abs(out - ref) <= bound).all(), float((np.abs(out - ref) - bound).max())


def test_randomised_shapes_flows_modes_vs_oracle(S, oracle):
    """Seeded sweep over shapes, channel counts, batch sizes, flow families (incl. collapsing and
    far-out-of-range flows) and all four modes, every case against the oracle."""
    rng = np.random.default_rng(int(os.environ.get("SLR_TEST_SEED", 20260928)))          # env: soak runs
    modes = ["summation", "average", "linear", "softmax"]
    for case in range(int(os.environ.get("SLR_TEST_CASES", 40))):
        N, C = int(rng.integers(1, 4)), int(rng.integers(1, 21))
        H, W = int(rng.integers(1, 90)), int(rng.integers(1, 210))
        y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        kind = case % 6
        if kind == 0:
            fl = rng.uniform(-3, 3, (N, 2, H, W))
        elif kind == 1:
            fl = rng.uniform(-60, 60, (N, 2, H, W))
        elif kind == 2:
            fl = np.stack([(W / 2 - x) * rng.uniform(0.5, 1.0), (H / 2 - y) * rng.uniform(0.5, 1.0)])[None].repeat(N, 0)
        elif kind == 3:
            fl = np.stack([np.sin(x / 7 + y / 11) * 6, np.cos(x / 9 - y / 5) * 6])[None].repeat(N, 0)
        elif kind == 4:
            fl = rng.integers(-5, 6, (N, 2, H, W)).astype(np.float32)
        else:
            fl = rng.uniform(-2, 2, (N, 2, H, W))
            fl[rng.random(fl.shape) < 0.02] = np.nan
        fl = fl.astype(np.float32)
        v = rng.standard_normal((N, C, H, W)).astype(np.float32)
        met = (rng.standard_normal((N, 1, H, W)) * 0.7).astype(np.float32)
        mode = modes[case % 4]
        m = np.abs(met) + 0.1 if mode == "linear" else met
        ref = oracle.function_softsplat(v, fl, m, mode)
        out = host(S.FunctionSoftsplat(dev(v), dev(fl), dev(m), mode))
        scale = max(1.0, float(np.abs(ref).max()))
        assert np.allclose(out, ref, rtol=2e-4, atol=2e-5 * scale), (case, N, C, H, W, kind, mode,
                                                                       float(np.abs(out - ref).max()))


def test_randomised_backward_vs_oracle(S, oracle):
    """Seeded sweep of the operator's backward (grad input: bit-exact gather; grad flow: C-loop per work-item in the
    reference's order, 1e-6) over shapes, batch sizes and flow families incl. out-of-range and integer flows
    (softsplat.py:204-326 restated in oracle/slr_oracle.c)."""
    rng = np.random.default_rng(int(os.environ.get("SLR_TEST_SEED", 99)))
    for case in range(int(os.environ.get("SLR_TEST_CASES", 24))):
        N, C = int(rng.integers(1, 3)), int(rng.integers(1, 12))
        H, W = int(rng.integers(1, 70)), int(rng.integers(1, 150))
        kind = case % 4
        if kind == 0:
            fl = rng.uniform(-3, 3, (N, 2, H, W))
        elif kind == 1:
            fl = rng.uniform(-80, 80, (N, 2, H, W))
        elif kind == 2:
            fl = rng.integers(-4, 5, (N, 2, H, W)).astype(np.float64)
        else:
            fl = rng.uniform(-1, 1, (N, 2, H, W)) + np.array([W / 3.0, -H / 4.0]).reshape(1, 2, 1, 1)
        fl = fl.astype(np.float32)
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        go = rng.standard_normal((N, C, H, W)).astype(np.float32)
        gi, gf = oracle.softsplat_backward(x, fl, go)
        a, b = dev(x).requires_grad_(True), dev(fl).requires_grad_(True)
        S.FunctionSoftsplat(a, b, None, "summation").backward(dev(go))
        assert np.array_equal(host(a.grad), gi), (case, N, C, H, W, kind)
        scale = max(1.0, float(np.abs(gf).max()))
        np.testing.assert_allclose(host(b.grad), gf, rtol=1e-6, atol=1e-6 * scale, err_msg=str((case, N, C, H, W, kind)))


def test_fused_synthesis_with_sink_motion_vs_oracle(S, oracle):
    """Motion field pointing at a sink: after a few Euler steps thousands of sources share a few
    output pixels in both splat directions (multi-segment tiles, long record lists, whole-tile
    path) -- fused two-direction kernel against the oracle, baseline and SLR-v1 packing."""
    H, W, N = 120, 200, 16
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    dx, dy = W * 0.6 - x, H * 0.4 - y
    r = np.sqrt(dx * dx + dy * dy) + 1e-3
    m = np.stack([dx / r * np.minimum(r, 4.0), dy / r * np.minimum(r, 4.0)])[None].astype(np.float32)
    rng = np.random.default_rng(17)
    fs = rng.standard_normal((1, 64, H, W)).astype(np.float32)
    Z = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    a = rng.standard_normal((1, 2, H, W)).astype(np.float32)
    abg = (1 / (1 + np.exp(-a[:, 0:1]))).astype(np.float32)
    cs = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N)
    cv = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N, alpha_fluid_logit=dev(a[:, 1:2]), alpha_bg=dev(abg))
    for t in (1, 8, 15):
        ref = oracle.synth_baseline(fs, Z, m, t, N)
        np.testing.assert_allclose(host(cs.features(t)), ref, rtol=2e-4, atol=2e-5)
        g, afl, _ = oracle.synth_v1(fs, Z, a[:, 1:2], abg, m, t, N)
        gg, aa = cv.features(t)
        np.testing.assert_allclose(host(gg), g, rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(host(aa), afl, rtol=2e-4, atol=5e-5)


def test_two_weight_groups_whole_tile_items_and_underflowing_weights(S, oracle):
    """The 2-layer model's alpha plane rides in the feature launch as a second weight group (shared records, pure
    bilinear weights).  (1) every source pixel onto one corner: whole-tile items (tiles over the partial-slot budget are
    walked segment by segment by one workgroup) next to ordinary frames of the batch; (2) Z spread over 400: e^(Z - Zmax)
    underflows to 0 for most pixels -- their features vanish as in the reference, their alpha (weights e^alpha0 = O(1)) must
    not."""
    H, W, N = 320, 640, 3
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    m = np.stack([W / 2 - x - 0.5, H / 2 - y - 0.5])[None].astype(np.float32)
    rng = np.random.default_rng(28)
    fs = rng.standard_normal((1, 6, H, W)).astype(np.float32)
    Z = (rng.standard_normal((1, 1, H, W)) * 0.3).astype(np.float32)
    a = rng.standard_normal((1, 2, H, W)).astype(np.float32)
    abg = (1 / (1 + np.exp(-a[:, 0:1]))).astype(np.float32)
    cv = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N, alpha_fluid_logit=dev(a[:, 1:2]), alpha_bg=dev(abg))
    ts = [1, 0, 2]
    out, outa = torch.empty(3, 6, H, W, device="cuda"), torch.empty(3, 1, H, W, device="cuda")
    cv.features_batch(ts, out, outa)
    for k, t in enumerate(ts):
        g, afl, _ = oracle.synth_v1(fs, Z, a[:, 1:2], abg, m, t, N)
        np.testing.assert_allclose(host(out[k:k + 1]), g, rtol=1e-3, atol=1e-4 * max(1.0, float(np.abs(g).max())), err_msg=str(t))
        np.testing.assert_allclose(host(outa[k:k + 1]), afl, rtol=1e-3, atol=1e-4, err_msg=str(t))
    # (2)
    H, W, N = 96, 200, 8
    fs = rng.standard_normal((1, 9, H, W)).astype(np.float32)
    Z = (rng.uniform(-400, 0, (1, 1, H, W))).astype(np.float32)
    a = rng.standard_normal((1, 2, H, W)).astype(np.float32)
    abg = (1 / (1 + np.exp(-a[:, 0:1]))).astype(np.float32)
    m = smooth_motion(H, W, 3, amp=2.0)
    cv = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(m), N, alpha_fluid_logit=dev(a[:, 1:2]), alpha_bg=dev(abg))
    for t in (1, 5):
        g, afl, _ = oracle.synth_v1(fs, Z, a[:, 1:2], abg, m, t, N)
        gg, aa = cv.features(t)
        assert float(np.abs(afl).max()) > 0.5 and (g == 0).mean() > 0.2          # features mostly gone, alpha plane alive
        np.testing.assert_allclose(host(aa), afl, rtol=2e-4, atol=5e-5)
        np.testing.assert_allclose(host(gg), g, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("tag", ["c2", "c3"])
def test_full_size_reference_digests(S, golden_dir, tag):
    """HIP path vs digests of the REFERENCE's own outputs at the C2 / C3 grids (no oracle involved):
    Euler displacement maps bit-exact, summation splat at 4096 sampled positions, plane sums,
    L2 norms, and the exact number of holes."""
    from conftest import large_case
    g, motion, inp, steps = large_case(golden_dir, tag)
    disp, vis = S.euler_integration(dev(motion), steps)
    hd = host(disp)
    assert np.array_equal(hd.ravel()[g[f"{tag}_disp_pos"]], g[f"{tag}_disp_val"])
    assert np.array_equal(hd.astype(np.float64).sum(axis=(2, 3)), g[f"{tag}_disp_sum"])
    assert float(vis.sum()) == float(g[f"{tag}_vis_sum"])
    out = host(S.FunctionSoftsplat(dev(inp), disp, None, "summation"))
    np.testing.assert_allclose(out.ravel()[g[f"{tag}_out_pos"]], g[f"{tag}_out_val"], **TOL)
    np.testing.assert_allclose(out.astype(np.float64).sum(axis=(2, 3)), g[f"{tag}_out_sum"], rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(np.sqrt((out.astype(np.float64) ** 2).sum(axis=(2, 3))), g[f"{tag}_out_l2"], rtol=1e-5)
    assert int((out == 0).sum()) == int(g[f"{tag}_holes"])


@pytest.mark.parametrize("tag,t", [("c3", 1), ("c3", 30), ("c3", 59), ("sq", 30)])
def test_timed_fused_kernel_full_size_vs_oracle_and_reference(S, oracle, golden_dir, tag, t):
    """The kernel bench.py times -- the fused two-flow instantiation behind ClipSynthesizer.features(t) with 64
    features (C3) and its SLR-v1 packing (C4) -- at the size it is timed, 768x1280, N = 60, t in {1, 30, 59}:
      * every element against the oracle (animating_softmax_splating.py:847-924,
        ..._2layers_alpha_seperate.py:950-1045);
      * against digests of the REFERENCE's own forward_flow on the same grid (4096 sampled positions, plane sums,
        exact hole count; tests/golden/pipeline_a6_large.npz, tools/make_golden_pipeline.py)."""
    from conftest import a6_large_inputs
    from test_oracle_golden import check_a6_digest
    g = load(golden_dir, "pipeline_a6_large")
    _, _, H, W = [int(v) for v in g[f"{tag}_shape"]]
    N = int(g["N"])
    fs, Z, motion, a = a6_large_inputs(H, W)
    cs = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(motion), N)
    gen = host(cs.features(t))
    ref = oracle.synth_baseline(fs, Z, motion, t, N)
    np.testing.assert_allclose(gen, ref, rtol=1e-4, atol=1e-5)
    assert_same_holes(gen, ref)
    check_a6_digest(g, tag, "baseline", t, gen, rtol=1e-4, atol=1e-5, hole_slack=4)
    abg = torch.sigmoid(dev(a[:, 0:1]))
    cv = S.synthesis.ClipSynthesizer(dev(fs), dev(Z), dev(motion), N, alpha_fluid_logit=dev(a[:, 1:2]), alpha_bg=abg)
    gen, afl = cv.features(t)
    gen, afl = host(gen), host(afl)
    rg, ra, _ = oracle.synth_v1(fs, Z, a[:, 1:2], host(abg), motion, t, N)
    np.testing.assert_allclose(gen, rg, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(afl, ra, rtol=1e-4, atol=2e-5)
    assert_same_holes(gen, rg)
    check_a6_digest(g, tag, "v1", t, gen, afl, rtol=1e-4, atol=2e-5, hole_slack=4)


def test_decoder_matrix_core_conv_vs_fp64(S):
    """Partial-conv decoder on the device (every 3x3 convolution = ONE fused split-f16 matrix-core kernel,
    csrc/conv.hip) vs the torch composition of the same modules evaluated in fp64 on the CPU (the
    definition that tests/test_nets_vs_reference.py validates against the reference's classes), next to
    the error of that composition in fp32.  Tolerance 5e-5 on outputs of magnitude ~5."""
    import copy
    from slr_sfs_amd import nets
    torch.manual_seed(3)
    dec = nets.DecoderPconv2(64, 3).eval()
    with torch.no_grad():
        for m in dec.modules():
            if hasattr(m, "stored_mean"):
                m.stored_mean.normal_(0, 0.3)
                m.stored_var.uniform_(0.5, 1.5)
        x = torch.randn(1, 64, 72, 136)
        x[:, :, 20:50, 30:80] = 0
        with nets.cpu_reference():
            y32 = dec(x)
            y64 = copy.deepcopy(dec).double()(x.double())
        y = dec.cuda()(x.cuda()).cpu()
    e_hip, e_f32 = (y.double() - y64).abs().max().item(), (y32.double() - y64).abs().max().item()
    assert y64.abs().max().item() > 1.0
    assert e_hip < 5e-5, (e_hip, e_f32)
    assert e_hip < 10 * e_f32 + 1e-6, (e_hip, e_f32)


@pytest.mark.parametrize("cin,cout,h,w,bias", [(16, 64, 9, 33, False), (32, 128, 19, 45, True), (64, 64, 64, 96, False),
                                               (48, 192, 8, 32, True), (16, 64, 1, 1, True), (3, 32, 17, 40, True),
                                               (128, 3, 24, 70, True), (3, 3, 16, 32, True), (20, 70, 11, 35, False)])
def test_conv3x3_matrix_core_kernel(S, cin, cout, h, w, bias):
    """slr_conv3x3_forward through the C ABI vs an fp64 convolution: ragged sizes (blocks cut by the image
    border, zero padding), channel counts that are not multiples of 16 / 32 (zero-padded weights), the
    128- / 64- / 32-channel workgroup variants, optional bias, BN + ReLU prologue, batch of 2."""
    import torch.nn.functional as F
    from slr_sfs_amd import nets
    torch.manual_seed(cin + h)
    conv = nets.Conv(cin, cout, 3, bias=bias).cuda()
    if bias:
        conv.bias.data.normal_()
    x = torch.randn(2, cin, h, w, device="cuda") * 3
    sc, sh = torch.rand(cin, device="cuda") + 0.5, torch.randn(cin, device="cuda")
    with torch.no_grad():
        y = conv(x)
        ref = F.conv2d(x.double(), conv.weight.double(), conv.bias.double() if bias else None, padding=1)
        yb = conv(x, (sc, sh))
        xb = F.relu(x * sc.view(1, -1, 1, 1) - sh.view(1, -1, 1, 1))          # fp32, as the prologue computes it
        refb = F.conv2d(xb.double(), conv.weight.double(), conv.bias.double() if bias else None, padding=1)
        res = torch.randn_like(y)
        yr, refr = conv(x, None, res), ref + res.double()      # residual joins the epilogue (ResNet_Block x_a + x_b)
    assert conv.__dict__.get("_wsplit") is not None          # the matrix-core path ran
    for got, want in ((y, ref), (yb, refb), (yr, refr)):
        assert (got - want).abs().max().item() < 4e-6 * max(want.abs().max().item(), 1.0)


@pytest.mark.parametrize("cin,cout,h,w,mode", [(64, 64, 24, 70, "derived"), (65, 128, 12, 40, "derived"), (64, 128, 16, 64, "plane"),
                                               (128, 3, 9, 40, "plane"), (32, 32, 20, 33, "chain")])
def test_pconv3x3_fused_equals_staged(S, cin, cout, h, w, mode):
    """The one-kernel partial convolution (prologue + matrix-core convolution + epilogue) against the
    staged path through the separately tested kernels: slr_bn_relu_mask -> slr_conv3x3_forward (bias-free)
    -> slr_pconv_epilogue.  Same operations in the same order on the same accumulators: bit-exact,
    including the update mask, with residual and with next-BN fusion."""
    from slr_sfs_amd import nets
    import torch.nn.functional as F
    torch.manual_seed(cout + w)
    pc = nets.PartialConv(cin, cout, 3).cuda()
    pc.bias.data.normal_()
    x = torch.randn(2, cin, h, w, device="cuda")
    x[:, :, 3:8, 5:20] = 0
    sc, sh = torch.rand(cin, device="cuda") + 0.5, torch.randn(cin, device="cuda") * 0.3
    nsc, nsh = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda") * 0.3
    res = torch.randn(2, cout, h, w, device="cuda")
    mask = None if mode == "derived" else (torch.rand(2, 1, h, w, device="cuda") > 0.3).float()
    pre = None if mode == "chain" else (sc, sh)
    with torch.no_grad():
        for kw in ({"residual": res}, {"next_bn": (nsc, nsh)}, {}):
            out, um = pc(x, mask, pre_bn=pre, **kw)
            # staged
            xin = nets.bn_relu_mask(x, sc, sh, mask) if pre is not None else x
            mplane, mscale = ((x != 0).sum(1, keepdim=True).float(), 1.0) if mask is None else (mask, float(cin))
            box = F.avg_pool2d(mplane, 3, stride=1, padding=1, divisor_override=1)
            raw0 = nets.Conv.conv(pc, xin, None)
            out2, um2 = nets.pconv_epilogue(raw0, pc.bias, box, mscale, cin * 9, kw.get("residual"), kw.get("next_bn"))
            assert torch.equal(um, um2)
            assert torch.equal(out, out2), (out - out2).abs().max().item()


@pytest.mark.parametrize("c,h,w", [(3, 7, 9), (5, 16, 32), (2, 33, 70), (4, 1, 1)])
def test_resample_kernels(S, c, h, w):
    """slr_avgpool3x3s2 / slr_upsample_bilinear2x vs torch's nn.AvgPool2d(3,2,1) / bilinear x2 on odd and even sizes."""
    import torch.nn.functional as F
    from slr_sfs_amd import nets
    torch.manual_seed(h)
    x = torch.randn(2, c, h, w, device="cuda")
    d = nets.avgpool_down(x)
    ref = F.avg_pool2d(x.cpu().double(), 3, stride=2, padding=1)
    assert d.shape == ref.shape
    np.testing.assert_allclose(host(d), ref.numpy(), rtol=0, atol=2e-6)
    u = nets.upsample_up(x)
    refu = F.interpolate(x.cpu().double(), scale_factor=2, mode="bilinear", align_corners=False)
    assert u.shape == refu.shape
    np.testing.assert_allclose(host(u), refu.numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("cin,cout,bias", [(128, 3, False), (7, 1, True), (64, 4, True)])
def test_conv1x1_small(S, cin, cout, bias):
    import torch.nn.functional as F
    from slr_sfs_amd import nets
    torch.manual_seed(cin)
    conv = nets.Conv(cin, cout, 1, bias=bias).cuda()
    if bias:
        conv.bias.data.normal_()
    x = torch.randn(2, cin, 12, 34, device="cuda")
    with torch.no_grad():
        y = conv(x)
        ref = F.conv2d(x.double(), conv.weight.double(), conv.bias.double() if bias else None)
    assert (y - ref).abs().max().item() < 5e-6


def test_conv3x3_saturates_instead_of_nan(S):
    """Activations beyond the f16 range of the split (|x| * 2^6 > 65504) saturate; no inf / NaN escapes -- and the
    clamp is never silent: the device counter behind slr_conv_saturation_count moves and nets.check_saturation raises
    (the reference's fp32 convolution has no such limit, so a clamped frame is an error, not a result)."""
    from slr_sfs_amd import nets
    torch.manual_seed(1)
    dev0 = torch.device("cuda", torch.cuda.current_device())
    conv = nets.Conv(16, 64, 3, bias=False).cuda()
    x = torch.randn(1, 16, 8, 32, device="cuda")
    with torch.no_grad():
        conv(x)
    assert nets.check_saturation(dev0) == 0                 # O(1) activations: nothing clamped (also resets the counter)
    x[0, 3, 4, 7] = 5.0e4
    x[0, 5, 2, 9] = -3.0e38
    with torch.no_grad():
        y = conv(x)
    assert bool(torch.isfinite(y).all())
    with pytest.raises(RuntimeError, match="1023"):
        nets.check_saturation(dev0)
    assert nets.check_saturation(dev0) == 0                 # the check reset the counter
    # activations of ~1e4 through every kernel family: 3x3 with the BN prologue (NCHW and channel-blocked), partial
    # convolution, 1x1 skip -- each must report
    big = torch.randn(1, 64, 16, 40, device="cuda") * 1.0e4
    mask = torch.ones(1, 1, 16, 40, device="cuda")
    sc, sh = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    with torch.no_grad():
        for run in (lambda: nets.Conv(64, 128, 3).cuda()(big, pre_bn=(sc, sh)),
                    lambda: nets.Conv(64, 128, 3).cuda()(big, layout=nets.IN_B8 | nets.OUT_B8),
                    lambda: nets.PartialConv(64, 64, 3).cuda()(big, mask, pre_bn=(sc, sh)),
                    lambda: nets.Conv(64, 128, 1).cuda()(big)):
            out = run()
            out = out[0] if isinstance(out, tuple) else out
            assert bool(torch.isfinite(out).all())
            with pytest.raises(RuntimeError):
                nets.check_saturation(dev0)
        # 1000 is inside the range: exact-domain, no report, and the result is right
        ok = torch.full((1, 16, 8, 32), 1000.0, device="cuda")
        c2 = nets.Conv(16, 32, 3, bias=False).cuda()
        y = c2(ok)
        ref = torch.nn.functional.conv2d(ok.double(), c2.weight.double(), padding=1)
        assert nets.check_saturation(dev0) == 0
        assert float((y.double() - ref).abs().max() / ref.abs().max()) < 1e-5


class _ScaledEncoder(torch.nn.Module):
    """An encoder whose features are `gain` times the wrapped one's: activations far outside the exact range of the
    split-f16 convolutions at their default scale (|x| < 1023), as an untrained / badly normalised checkpoint produces."""

    def __init__(self, enc, gain):
        super().__init__()
        self.enc, self.gain = enc, gain
        self.blocks = enc.blocks

    def forward(self, x):
        fs, Z = self.enc(x)
        return fs * self.gain, Z


@pytest.mark.parametrize("gain,rung", [(1.5e3, 1), (3.0e6, 2)])
def test_large_activations_are_rendered_not_refused(S, gain, rung):
    """The reference's decoder is plain fp32 with no magnitude limit (models/layers/partialconv2d.py:61-74,
    models/networks/architectures.py:345-375).  With the default policy (convs="auto") a clip whose decoder activations
    leave the exact range of the split-f16 kernels is rendered again one rung up -- activation scale 1 (exact to 65472),
    then fp32 convolutions through torch -- instead of raising: frames within 1e-4 of the fp64 definition of the same
    networks, the raw decoder output within 1e-4 of its range.  convs="split" still refuses such a clip loudly."""
    import copy
    import warnings
    from slr_sfs_amd import nets, pipeline
    torch.manual_seed(11)
    H, W, N = 64, 96, 5
    base = pipeline.BaselineAnimator()
    an = pipeline.BaselineAnimator(encoder=_ScaledEncoder(base.encoder, gain), decoder=base.projector).cuda().eval()
    img = torch.rand(1, 3, H, W, device="cuda") * 2 - 1
    m = torch.randn(1, 2, H, W, device="cuda")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        frames = an.synthesize(img, m, N)                              # no exception
    assert an._conv_rung == rung and any("exact range" in str(x.message) for x in w)
    assert bool(torch.isfinite(frames).all())
    # the fp64 definition of the same decoder on the same decoder inputs.  With decoder outputs of magnitude ~gain in
    # front of the tanh, "within 1e-4" is a statement about the RAW output (relative to its range: 1e-5 here); on the
    # frames themselves fp32 arithmetic of any kind is only good to eps * |raw| where raw crosses zero, so the frames are
    # held to the error the all-fp32 route (convs="fp32": torch / MIOpen) makes against the same fp64 reference.
    clip = an.begin_clip(img, m, N)
    dec64 = copy.deepcopy(an.projector).double()
    f32 = an.synthesize(img, m, N, convs="fp32")
    worst_raw, err_auto, err_f32 = 0.0, 0.0, 0.0
    for t in range(N):
        gen = clip.features(t)
        assert float(gen.abs().max()) > 1023.0                         # really outside the default exact range
        with nets.torch_convolutions(), torch.no_grad():
            raw64 = dec64(gen.double())
        raw = nets.guarded(lambda: an.projector(gen), gen.device, "auto", "decoder", an)
        worst_raw = max(worst_raw, float((raw.double() - raw64).abs().max() / raw64.abs().max()))
        err_auto = max(err_auto, float((frames[t:t + 1].double() - torch.tanh(raw64)).abs().max()))
        err_f32 = max(err_f32, float((f32[t:t + 1].double() - torch.tanh(raw64)).abs().max()))
    assert worst_raw < 1e-5, worst_raw
    assert err_auto <= max(1e-4, 4.0 * err_f32), (err_auto, err_f32)
    # a second clip starts on the rung that worked: no further warning, same frames
    with warnings.catch_warnings(record=True) as w2:
        warnings.simplefilter("always")
        again = an.synthesize(img, m, N)
    assert not w2 and float((again - frames).abs().max()) <= max(1e-4, 8.0 * err_f32)    # (the encoder now runs on that rung too)
    # frames leaving the rank one by one (multi-GPU rounds form) are checked before they go
    an._conv_rung = 0
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        an.synthesize(img, m, N, on_frame=lambda f: seen.append(f.clone()))
    assert len(seen) == N and all(float((a - b).abs().max()) <= max(1e-4, 8.0 * err_f32) for a, b in zip(seen, frames))
    # the explicit policies
    with pytest.raises(RuntimeError, match="exact range"):
        an.synthesize(img, m, N, convs="split")
    assert float((f32 - frames).abs().max()) <= max(1e-4, 8.0 * err_f32)


def test_saturation_counter_follows_the_callers_stream(S):
    """slr_conv_saturation_count is ordered on the stream it is given (torch's side streams are non-blocking streams:
    the legacy null stream does not wait for them), and slr_conv_saturation_record leaves asynchronous per-piece records."""
    from slr_sfs_amd import nets
    dev0 = torch.device("cuda", torch.cuda.current_device())
    nets.saturation_count(dev0)
    conv = nets.Conv(16, 32, 3, bias=False).cuda()
    big = torch.full((1, 16, 64, 128), 5.0e4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(20):
            conv(big)
        assert nets.saturation_count(dev0) > 0                         # read on `side`, right behind its convolutions
        log = nets.SaturationLog(dev0, 3)
        conv(torch.ones(1, 16, 8, 32, device="cuda")); log.mark()
        conv(big); log.mark()
        conv(torch.ones(1, 16, 8, 32, device="cuda")); log.mark()
        assert log.bad() == [1]
        assert nets.saturation_count(dev0) > 0                         # (records do not reset the counter; this read does)
        with nets.activation_scale(1.0):                               # 5e4 is inside the exact range at scale 1
            y = conv(big)
            assert nets.saturation_count(dev0) == 0
        ref = torch.nn.functional.conv2d(big.double(), conv.weight.double(), padding=1)
        assert float((y.double() - ref).abs().max() / ref.abs().max()) < 1e-5
    torch.cuda.current_stream().wait_stream(side)
    nets.saturation_count(dev0)


@pytest.mark.parametrize("cin,cout,h,w,bias", [(64, 128, 16, 40, False), (128, 256, 9, 33, True), (3, 32, 7, 19, True),
                                               (256, 128, 8, 16, False), (64, 65, 5, 27, True), (20, 300, 6, 10, True)])
def test_conv1x1_matrix_core_kernel(S, cin, cout, h, w, bias):
    """slr_conv1x1_forward (skip branches) vs an fp64 convolution: all workgroup variants (32..256 channels per
    row and more than 256), ragged pixel counts and channel counts, batch of 2."""
    import torch.nn.functional as F
    from slr_sfs_amd import nets
    torch.manual_seed(cin + cout)
    conv = nets.Conv(cin, cout, 1, bias=bias).cuda()
    if bias:
        conv.bias.data.normal_()
    x = torch.randn(2, cin, h, w, device="cuda") * 2
    with torch.no_grad():
        y = conv(x)
        ref = F.conv2d(x.double(), conv.weight.double(), conv.bias.double() if bias else None)
    assert conv.__dict__.get("_wsplit") is not None
    assert (y - ref).abs().max().item() < 4e-6 * max(ref.abs().max().item(), 1.0)


@pytest.mark.parametrize("which", ["encoder_z", "bg_decoder", "alpha_encoder"])
def test_plain_resnet_nets_vs_fp64_definition(S, which):
    """Encoder / background decoder / alpha encoder on the device (matrix-core 3x3 with BN+ReLU prologue, bias and
    residual epilogue; split-f16 1x1 skips; HIP resampling) vs the torch definition of the same modules in fp64."""
    import copy
    from slr_sfs_amd import nets
    torch.manual_seed(11)
    net = {"encoder_z": lambda: nets.EncoderWithZ(), "bg_decoder": lambda: nets.BGDecoder(),
           "alpha_encoder": lambda: nets.Encoder(3, 2)}[which]().eval()
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "stored_mean"):
                m.stored_mean.normal_(0, 0.3)
                m.stored_var.uniform_(0.5, 1.5)
            if isinstance(m, nets.Conv) and m.bias is not None:
                m.bias.normal_(0, 0.1)
        x = torch.rand(1, 3, 40, 72) * 2 - 1
        with nets.cpu_reference():
            ref = copy.deepcopy(net).double()(x.double())
        out = net.cuda()(x.cuda())
    ref = ref if isinstance(ref, tuple) else (ref,)
    out = out if isinstance(out, tuple) else (out,)
    for o, r in zip(out, ref):
        scale = max(r.abs().max().item(), 1.0)
        assert (o.cpu().double() - r).abs().max().item() < 2e-5 * scale


def test_conv_kernels_randomised_sweep(S):
    """30 random (Cin, Cout, H, W, N, options) cases: plain 3x3 (bias / BN prologue / residual), 1x1, and the
    one-kernel partial convolution vs its staged definition (bit-exact)."""
    import torch.nn.functional as F
    from slr_sfs_amd import nets
    rng = np.random.default_rng(int(os.environ.get("SLR_TEST_SEED", 2024)))               # env: soak runs
    for case in range(int(os.environ.get("SLR_TEST_CASES", 30))):
        cin, cout = int(rng.integers(1, 70)), int(rng.integers(1, 140))
        h, w, n = int(rng.integers(1, 20)), int(rng.integers(1, 70)), int(rng.integers(1, 3))
        torch.manual_seed(case)
        x = torch.randn(n, cin, h, w, device="cuda") * float(rng.uniform(0.1, 4))
        x[:, :, : h // 2, : w // 3] = 0
        with torch.no_grad():
            # plain 3x3
            use_bias, use_pre, use_res = (bool(v) for v in rng.integers(0, 2, 3))
            conv = nets.Conv(cin, cout, 3, bias=use_bias).cuda()
            if use_bias:
                conv.bias.data.normal_()
            sc, sh = torch.rand(cin, device="cuda") + 0.5, torch.randn(cin, device="cuda") * 0.5
            res = torch.randn(n, cout, h, w, device="cuda") if use_res else None
            y = conv(x, (sc, sh) if use_pre else None, res)
            xin = F.relu(x * sc.view(1, -1, 1, 1) - sh.view(1, -1, 1, 1)) if use_pre else x
            ref = F.conv2d(xin.double(), conv.weight.double(), conv.bias.double() if use_bias else None, padding=1)
            if use_res:
                ref = ref + res.double()
            assert (y - ref).abs().max().item() < 5e-6 * max(ref.abs().max().item(), 1.0), ("3x3", case, cin, cout, h, w)
            # 1x1
            c1 = nets.Conv(cin, cout, 1, bias=use_bias).cuda()
            y1 = c1(x)
            r1 = F.conv2d(x.double(), c1.weight.double(), c1.bias.double() if use_bias else None)
            assert (y1 - r1).abs().max().item() < 5e-6 * max(r1.abs().max().item(), 1.0), ("1x1", case, cin, cout, h, w)
            # partial convolution: fused vs staged, bit-exact
            pc = nets.PartialConv(cin, cout, 3).cuda()
            pc.bias.data.normal_()
            mode = ("derived", "plane", "chain")[int(rng.integers(0, 3))]
            mask = None if mode == "derived" else (torch.rand(n, 1, h, w, device="cuda") > 0.3).float()
            pre = None if mode == "chain" else (sc, sh)
            nsc, nsh = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda") * 0.3
            kw = ({"residual": torch.randn(n, cout, h, w, device="cuda")}, {"next_bn": (nsc, nsh)}, {})[int(rng.integers(0, 3))]
            out, um = pc(x, mask, pre_bn=pre, **kw)
            xs_ = nets.bn_relu_mask(x, sc, sh, mask) if pre is not None else x
            mplane, mscale = ((x != 0).sum(1, keepdim=True).float(), 1.0) if mask is None else (mask, float(cin))
            box = F.avg_pool2d(mplane, 3, stride=1, padding=1, divisor_override=1)
            out2, um2 = nets.pconv_epilogue(nets.Conv.conv(pc, xs_, None), pc.bias, box, mscale, cin * 9,
                                            kw.get("residual"), kw.get("next_bn"))
            assert torch.equal(um, um2), ("um", case, mode, cin, cout, h, w)
            assert torch.equal(out, out2), ("pconv", case, mode, cin, cout, h, w, (out - out2).abs().max().item())


@pytest.mark.parametrize("cin,cout,h,w", [(64, 128, 16, 64), (32, 64, 9, 33), (128, 72, 11, 40)])
def test_conv_channel_blocked_intermediate(S, cin, cout, h, w):
    """The channel-blocked ([N,C/8,H,W,8]) layout of the activation between a block's two convolutions: writing it
    (SLR_CONV_OUT_B8) and reading it (SLR_CONV_IN_B8) is bit-identical to the NCHW path -- plain and partial
    convolution, with prologue / next-BN / residual."""
    from slr_sfs_amd import nets
    torch.manual_seed(cin + w)

    def to_b8(t):
        n, c, hh, ww = t.shape
        return t.view(n, c // 8, 8, hh, ww).permute(0, 1, 3, 4, 2).contiguous().view(n, c, hh, ww)

    x = torch.randn(2, cin, h, w, device="cuda")
    mask = (torch.rand(2, 1, h, w, device="cuda") > 0.3).float()
    sc, sh = torch.rand(cin, device="cuda") + 0.5, torch.randn(cin, device="cuda") * 0.3
    nsc, nsh = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda") * 0.3
    with torch.no_grad():
        conv = nets.Conv(cin, cout, 3).cuda()
        conv.bias.data.normal_()
        ref = conv(x, (sc, sh))
        assert torch.equal(conv(x, (sc, sh), layout=nets.OUT_B8), to_b8(ref))                     # producer
        res = torch.randn_like(ref)
        assert torch.equal(conv(to_b8(x), (sc, sh), res, layout=nets.IN_B8), conv(x, (sc, sh), res))   # consumer
        pc = nets.PartialConv(cin, cout, 3).cuda()
        pc.bias.data.normal_()
        o1, m1 = pc(x, mask, next_bn=(nsc, nsh), pre_bn=(sc, sh))
        o2, m2 = pc(x, mask, next_bn=(nsc, nsh), pre_bn=(sc, sh), layout=nets.OUT_B8)
        assert torch.equal(o2, to_b8(o1)) and torch.equal(m1, m2)
        r2 = torch.randn_like(o1)
        o3, m3 = pc(x, mask, residual=r2)
        o4, m4 = pc(to_b8(x), mask, residual=r2, layout=nets.IN_B8)
        assert torch.equal(o3, o4) and torch.equal(m3, m4)


def test_channel_blocked_resample_and_skip_kernels(S):
    """The channel-blocked ([N,C/8,H,W,8]) variants of the stages between the blocks against their NCHW kernels:
    3x3/2 average pooling, x2 bilinear up-sampling, the 1x1 skip convolutions (split-f16 and the <= 4-channel one),
    and the 3x3 convolution writing a blocked output on top of a blocked / NCHW residual -- bit-identical."""
    from slr_sfs_amd import nets
    torch.manual_seed(17)

    def to_b8(t):
        n, c, hh, ww = t.shape
        return t.view(n, c // 8, 8, hh, ww).permute(0, 1, 3, 4, 2).contiguous().view(n, c, hh, ww)

    x = torch.randn(2, 24, 13, 34, device="cuda")
    xb = to_b8(x)
    with torch.no_grad():
        assert torch.equal(nets.avgpool_down(xb, True), to_b8(nets.avgpool_down(x)))
        assert torch.equal(nets.upsample_up(xb, True), to_b8(nets.upsample_up(x)))
        c1 = nets.Conv(24, 72, 1, bias=False).cuda()
        ref1 = c1(x)
        assert torch.equal(c1(xb, layout=nets.IN_B8), ref1)
        assert torch.equal(c1(x, layout=nets.OUT_B8), to_b8(ref1))
        assert torch.equal(c1(xb, layout=nets.IN_B8 | nets.OUT_B8), to_b8(ref1))
        x4 = torch.randn(2, 24, 12, 32, device="cuda")
        c3 = nets.Conv(24, 3, 1, bias=True).cuda()
        c3.bias.data.normal_()
        assert torch.equal(c3(to_b8(x4), layout=nets.IN_B8), c3(x4))
        conv = nets.Conv(24, 40, 3).cuda()
        res = torch.randn(2, 40, 13, 34, device="cuda")
        ref = conv(x, None, res)
        assert torch.equal(conv(x, None, res, layout=nets.OUT_B8), to_b8(ref))                                  # NCHW residual
        assert torch.equal(conv(xb, None, to_b8(res), layout=nets.IN_B8 | nets.OUT_B8 | nets.RES_B8), to_b8(ref))   # blocked residual


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pconv", "plain"])
@pytest.mark.parametrize("cin,cout,h,w,resample", [(64, 128, 16, 64, "Down"), (128, 256, 9, 33, "Down"), (256, 128, 11, 40, "Up"),
                                                   (128, 128, 8, 32, "Up"), (3, 32, 13, 70, None), (24, 72, 21, 37, None),
                                                   (40, 64, 5, 96, None), (64, 128, 21, 70, "Down"), (72, 136, 17, 33, "Down"),
                                                   (32, 72, 40, 100, "Down"), (16, 64, 12, 40, "Down"), (128, 128, 13, 45, "Up"),
                                                   (72, 136, 17, 33, "Up"), (256, 128, 9, 70, "Up"), (64, 72, 1, 5, "Up"), (64, 72, 3, 1, "Down")])
def test_skip_branch_inside_the_second_convolution(S, kind, cin, cout, h, w, resample):
    """slr_conv3x3_forward_skip / slr_pconv3x3_forward_skip (ABI 10): a residual block's 1x1 skip convolution as extra
    K chunks of its second 3x3 kernel (models/layers/blocks.py:83-87, :237-248) against the two-kernel form (staged_skips(): 1x1 kernel ->
    residual of the 3x3 epilogue).  Same products; only the order of the LAST additions differs (the skip's products join the finished
    3x3 value one chunk at a time instead of as one sum), so the two agree to fp32 rounding: <= 2e-6 of the output scale (the split-f16
    arithmetic itself is 2-5e-6 against fp64, test_conv3x3_matrix_core_kernel).  Update masks are bit-identical.  "Down" blocks with
    more than 64 output channels also pool in that kernel's epilogue (SLR_CONV_POOL_OUT: interior pooled pixels in registers, tile-border
    ones completed by pool_fix_kernel) -- against the pool kernel on the fused convolution's output: <= 1e-6; "Up" blocks up-sample there
    (SLR_CONV_UP_OUT, borders by upsample_fix_kernel): bit-identical to the up-sampling kernel on the fused convolution's output.  Down / Up blocks,
    a 3-channel NCHW skip input (the encoders' first block), ragged sizes, padded channel counts; and against an fp64 definition."""
    import torch.nn.functional as F
    from slr_sfs_amd import nets
    torch.manual_seed(cin * 7 + w)
    n = 2
    with torch.no_grad():
        if kind == "pconv":
            blk = nets.PconvResBlock(cin, cout, resample).cuda()
        else:
            blk = nets.ResBlock(cin, cout, resample).cuda()
        for m in blk.modules():
            if isinstance(m, nets.AffineBN):
                m.stored_mean.normal_(0, 0.3); m.stored_var.uniform_(0.5, 1.5)
            if isinstance(m, nets.Conv) and m.bias is not None:
                m.bias.normal_()
        x = torch.randn(n, cin, h, w, device="cuda")
        b8_in = cin % 8 == 0

        def to_b8(t):
            nn_, c, hh, ww = t.shape
            return t.view(nn_, c // 8, 8, hh, ww).permute(0, 1, 3, 4, 2).contiguous().view(nn_, c, hh, ww)

        def from_b8(t):
            nn_, c, hh, ww = t.shape
            return t.view(nn_, c // 8, hh, ww, 8).permute(0, 1, 4, 2, 3).contiguous().view(nn_, c, hh, ww)

        xin = to_b8(x) if b8_in else x
        mask = (torch.rand(n, 1, h, w, device="cuda") > 0.3).float()
        L = nets._lib.lib()
        name = "slr_pconv3x3_forward_skip" if kind == "pconv" else "slr_conv3x3_forward_skip"
        entry, calls = getattr(L, name), []

        def counted(*a):
            calls.append(1)
            return entry(*a)

        def run():
            if kind == "pconv":
                y, m, b8 = blk(xin, mask, b8_in)
            else:
                (y, b8), m = blk(xin, b8_in), None
            assert b8
            return from_b8(y), m

        rname = {"Down": "slr_avgpool3x3s2", "Up": "slr_upsample_bilinear2x"}.get(resample, "slr_avgpool3x3s2")
        pool_entry, pool_calls = getattr(L, rname), []

        def counted_pool(*a):
            pool_calls.append(1)
            return pool_entry(*a)

        setattr(L, name, counted)
        setattr(L, rname, counted_pool)
        try:
            y1, m1 = run()
            fused = 1 if b8_in else 0                  # (an NCHW block input keeps the two-kernel form)
            assert len(calls) == fused, "the fused entry point was not called"
            # resampling blocks with more than 64 output channels: the average pool / the up-sampling happened in that kernel's epilogue
            res_fused = bool(resample) and fused and cout > 64
            assert len(pool_calls) == (1 if resample and not res_fused else 0)
            if res_fused:
                with nets.staged_skips(pools_only=True):               # fused skip, resampling kernel
                    y2, _ = run()
                assert len(calls) == 2 and len(pool_calls) == 1
                if resample == "Up":
                    assert torch.equal(y1, y2), (y1 - y2).abs().max().item()
                else:
                    assert (y1 - y2).abs().max().item() <= 1e-6 * max(y2.abs().max().item(), 1.0)
            calls.clear()
            with nets.staged_skips():
                y0, m0 = run()
            assert len(calls) == 0
        finally:
            setattr(L, name, entry)
            setattr(L, rname, pool_entry)
        if m1 is not None:
            assert torch.equal(m1, m0)
        scale = y0.abs().max().item()
        err = (y1 - y0).abs().max().item()
        assert err <= 2e-6 * max(scale, 1.0), (kind, cin, cout, err, scale)
        # fp64 definition of the block
        xd = x.double()
        def bn(t, b):
            sc, sh = b.scale_shift()
            return t * sc.double().view(1, -1, 1, 1) - sh.double().view(1, -1, 1, 1)
        wa, wb_, ws_ = blk.conv_aa.weight.double(), blk.conv_ab.weight.double(), blk.conv_b.weight.double()
        if kind == "plain":
            a = F.conv2d(F.relu(bn(xd, blk.bn1)), wa, blk.conv_aa.bias.double(), padding=1)
            a = F.conv2d(F.relu(bn(a, blk.bn2)), wb_, blk.conv_ab.bias.double(), padding=1)
            a = a + F.conv2d(xd, ws_, blk.conv_b.bias.double())
        else:
            md = mask.double()
            def pconv(t, msk, wt, bias, c_in):
                box = F.avg_pool2d(msk, 3, stride=1, padding=1, divisor_override=1) * c_in
                um = box.clamp(0, 1)
                ratio = (c_in * 9) / (box + 1e-8) * um
                return (F.conv2d(t, wt, None, padding=1) * ratio + bias.double().view(1, -1, 1, 1)) * um, um
            a, um = pconv(F.relu(bn(xd, blk.bn1)) * md, md, wa, blk.conv_aa.bias, cin)
            a, um = pconv(F.relu(bn(a, blk.bn2)) * um, um, wb_, blk.conv_ab.bias, cout)
            a = a + F.conv2d(xd, ws_, None)
        if resample == "Down":
            a = F.avg_pool2d(a, 3, stride=2, padding=1)
        elif resample == "Up":
            a = F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=False)
        e64 = (y1.double() - a).abs().max().item()
        assert e64 <= 3e-5 * max(a.abs().max().item(), 1.0), (kind, cin, cout, e64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pconv", "plain"])
@pytest.mark.parametrize("cin,cout,h,w,resample", [(64, 128, 21, 70, "Down"), (256, 128, 9, 70, "Up"), (128, 136, 17, 33, None), (72, 256, 8, 32, "Down")])
def test_skip_branch_inside_the_second_convolution_fp32_rung(S, kind, cin, cout, h, w, resample):
    """The fused residual-block kernels on the fp32 rung (SLR_CONV_F32: v_mfma_f32_32x32x2_f32, more than 64 output channels): against the
    two-kernel forms inside the same rung -- skip <= 2e-6 of the output scale, pooled <= 1e-6, up-sampled bit-identical, masks bit-identical."""
    from slr_sfs_amd import nets
    torch.manual_seed(cin + w)
    n = 2
    with torch.no_grad(), nets.fp32_kernels(winograd=False):
        blk = (nets.PconvResBlock if kind == "pconv" else nets.ResBlock)(cin, cout, resample).cuda()
        for m in blk.modules():
            if isinstance(m, nets.AffineBN):
                m.stored_mean.normal_(0, 0.3); m.stored_var.uniform_(0.5, 1.5)
            if isinstance(m, nets.Conv) and m.bias is not None:
                m.bias.normal_()
        x = torch.randn(n, cin, h, w, device="cuda")
        xin = x.view(n, cin // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().view(n, cin, h, w)
        mask = (torch.rand(n, 1, h, w, device="cuda") > 0.3).float()
        L = nets._lib.lib()
        name = "slr_pconv3x3_forward_skip" if kind == "pconv" else "slr_conv3x3_forward_skip"
        entry, calls = getattr(L, name), []

        def counted(*a):
            calls.append(1)
            return entry(*a)

        def run():
            if kind == "pconv":
                y, m, b8 = blk(xin, mask, True)
            else:
                (y, b8), m = blk(xin, True), None
            return y, m

        setattr(L, name, counted)
        try:
            y1, m1 = run()
            assert len(calls) == 1
            with nets.staged_skips(pools_only=True):
                y2, _ = run()
            with nets.staged_skips():
                y0, m0 = run()
            assert len(calls) == 2
        finally:
            setattr(L, name, entry)
        if m1 is not None:
            assert torch.equal(m1, m0)
        scale = max(y0.abs().max().item(), 1.0)
        assert (y1 - y0).abs().max().item() <= 2e-6 * scale
        if resample == "Up":
            assert torch.equal(y1, y2)
        else:
            assert (y1 - y2).abs().max().item() <= 1e-6 * scale


@pytest.mark.gpu
def test_fused_residual_blocks_randomised_sweep(S):
    """48 random residual blocks (channel counts in steps of 8 up to 160, sizes 1 .. 70 x 1 .. 150, Down / Up / none, plain / partial, both
    rungs): the fused kernels (skip, pool, up-sampling in the second convolution; narrow-end skip in the first) against the two-kernel forms
    -- tile borders, images smaller than a tile, cut tiles, padded channel tiles."""
    from slr_sfs_amd import nets
    rng = np.random.default_rng(20260929)
    torch.manual_seed(5)
    for case in range(48):
        cin = int(rng.integers(1, 21)) * 8
        cout = int(rng.choice([1, 2, 3, 4])) if case % 6 == 5 else int(rng.integers(1, 21)) * 8
        h, w = int(rng.integers(1, 71)), int(rng.integers(1, 151))
        resample = None if cout <= 4 else [None, "Down", "Up"][int(rng.integers(0, 3))]
        kind = "pconv" if rng.integers(0, 2) else "plain"
        f32 = case % 4 == 3
        n = int(rng.integers(1, 3))
        with torch.no_grad():
            blk = (nets.PconvResBlock if kind == "pconv" else nets.ResBlock)(cin, cout, resample).cuda()
            for m in blk.modules():
                if isinstance(m, nets.AffineBN):
                    m.stored_mean.normal_(0, 0.3); m.stored_var.uniform_(0.5, 1.5)
                if isinstance(m, nets.Conv) and m.bias is not None:
                    m.bias.normal_()
            x = torch.randn(n, cin, h, w, device="cuda")
            xin = x.view(n, cin // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().view(n, cin, h, w)
            mask = (torch.rand(n, 1, h, w, device="cuda") > 0.3).float()

            def run():
                if kind == "pconv":
                    y, m, _ = blk(xin, mask, True)
                    return y, m
                return blk(xin, True)[0], None

            import contextlib
            with (nets.fp32_kernels(winograd=False) if f32 else contextlib.nullcontext()):
                y1, m1 = run()
                with nets.staged_skips():
                    y0, m0 = run()
            what = (case, kind, cin, cout, h, w, resample, f32)
            if m1 is not None:
                assert torch.equal(m1, m0), what
            if blk.conv_b is None:
                assert torch.equal(y1, y0), what
            else:
                err, scale = (y1 - y0).abs().max().item(), max(y0.abs().max().item(), 1.0)
                assert err <= 3e-6 * scale, what + (err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pconv", "plain"])
@pytest.mark.parametrize("cin,cout,h,w", [(128, 3, 21, 70), (64, 3, 16, 64), (24, 2, 9, 33), (8, 4, 40, 131), (16, 1, 1, 3)])
def test_narrow_end_skip_from_the_same_pass(S, kind, cin, cout, h, w):
    """slr_conv3x3_forward_skipout / slr_pconv3x3_forward_skipout (ABI 10): the decoders' 128 -> 3 end -- the block's first convolution and the
    block's 1x1 skip convolution of the same input from ONE pass over it (models/layers/blocks.py:192-193, 229-248).  Against the
    two-kernel form (staged_skips(): slr_conv1x1_small): bit-identical block output and update mask."""
    from slr_sfs_amd import nets
    torch.manual_seed(cin + 3 * w)
    n = 2
    with torch.no_grad():
        blk = (nets.PconvResBlock if kind == "pconv" else nets.ResBlock)(cin, cout).cuda()
        for m in blk.modules():
            if isinstance(m, nets.AffineBN):
                m.stored_mean.normal_(0, 0.3); m.stored_var.uniform_(0.5, 1.5)
            if isinstance(m, nets.Conv) and m.bias is not None:
                m.bias.normal_()
        x = torch.randn(n, cin, h, w, device="cuda")
        xin = x.view(n, cin // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().view(n, cin, h, w)
        mask = (torch.rand(n, 1, h, w, device="cuda") > 0.3).float()
        L = nets._lib.lib()
        name = "slr_pconv3x3_forward_skipout" if kind == "pconv" else "slr_conv3x3_forward_skipout"
        entry, calls = getattr(L, name), []

        def counted(*a):
            calls.append(1)
            return entry(*a)

        def run():
            if kind == "pconv":
                y, m, b8 = blk(xin, mask, True)
            else:
                (y, b8), m = blk(xin, True), None
            assert not b8
            return y, m

        setattr(L, name, counted)
        try:
            y1, m1 = run()
            assert len(calls) == 1, "the skip-out entry point was not called"
            with nets.staged_skips():
                y0, m0 = run()
            assert len(calls) == 1
        finally:
            setattr(L, name, entry)
        assert torch.equal(y1, y0), (y1 - y0).abs().max().item()
        if m1 is not None:
            assert torch.equal(m1, m0)


@pytest.mark.gpu
def test_clip_kernels_on_plane_blocked_values(S):
    """SLR_SYNTH_VALUES_B4 (ABI 8): slr_pack_planes4 writes [C/4][H][W][4]; the clip kernels then read a chunk's 4 planes of a source pixel
    with one 16-byte load.  Same arithmetic as on the planar tensor: the two agree to the run-to-run noise of the summation order
    (pieces whose entry slots come from atomics), and with the oracle; a ragged grid, both models' packings, one frame and a batch."""
    from slr_sfs_amd import synthesis
    torch.manual_seed(5)
    H, W, N = 88, 200, 9
    fs = torch.randn(1, 64, H, W, device="cuda")
    Z = torch.randn(1, 1, H, W, device="cuda")
    motion = torch.from_numpy(smooth_motion(H, W, 3, amp=2.0)).cuda()
    p4 = synthesis.pack_planes4(fs)
    assert torch.equal(p4.view(1, 16, H, W, 4), fs.view(1, 16, 4, H, W).permute(0, 1, 3, 4, 2))
    af, abg = torch.randn(1, 1, H, W, device="cuda"), torch.rand(1, 1, H, W, device="cuda")
    for kw in ({}, {"alpha_fluid_logit": af, "alpha_bg": abg}):
        res = {}
        for b4 in (True, False):
            old = synthesis.USE_B4
            synthesis.USE_B4 = b4
            try:
                cs = synthesis.ClipSynthesizer(fs, Z, motion, N, **kw)
            finally:
                synthesis.USE_B4 = old
            assert (cs.fs4 is not None) == b4
            ts = [1, 4, 5, 8]
            out = torch.empty(len(ts), 64, H, W, device="cuda")
            oa = torch.empty(len(ts), 1, H, W, device="cuda") if kw else None
            cs.features_batch(ts, out, oa)
            one = cs.features(4)
            res[b4] = (out, oa, one[0] if isinstance(one, tuple) else one)
        for a, b in zip(res[True], res[False]):
            if a is not None:
                assert float((a - b).abs().max()) < 2e-5 * max(1.0, float(b.abs().max()))
        assert float((res[True][0][1] - res[True][2][0]).abs().max()) < 2e-5 * max(1.0, float(res[True][0].abs().max()))     # batch == single call

