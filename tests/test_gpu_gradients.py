"""The gradients of the splat on the GPU, at the shapes bench.py times and in every mode of FunctionSoftsplat.

  1. slr_softsplat_backward_ws at [1,65,768,1280] (identity, Euler t=30, t=59: bench.py's backward_roofline) against the oracle:
     channel groups with a tail pass, group-major launch order, the partial gradFlow sums, every path of grad_tile_kernel in one launch.
  2. d/d(input, flow, metric) of summation / average / linear / softmax against torch autograd through the float64 definition of
     tests/splat_f64.py, judged by the error of the same definition run in float32.
  3. the training step as a chain (EulerIntegration -> exp(Z - Z.max()) -> two summation splats -> sum, clamp, divide), differentiated
     w.r.t. features, Z and the motion field, without a host synchronisation.
  4. the Euler backward at the training shape, with a bound derived from its structure (a scatter with coefficient 1).

Criterion of 2. and 3. per gradient tensor: E = max|got - ref64| / max|ref64|, and E_gpu <= 10 * E_plain32 + 1e-6 where E_plain32 is the
same quantity for the plain definition in float32 on the CPU (form and factor: test_decoder_matrix_core_conv_vs_fp64; the factor covers
another summation order over the same float32 terms).  Every figure is printed before it is asserted (run with -s)."""
import itertools

import numpy as np
import pytest
import torch

import splat_f64 as F64

pytestmark = pytest.mark.gpu

MODES = ("summation", "average", "linear", "softmax")


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


def smooth_motion(H, W, seed=0, amp=1.5):
    rng = np.random.default_rng(seed)
    p1, p2 = rng.uniform(0, 2 * np.pi, 2)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    u = amp * np.sin(2 * np.pi * (2 * x / W + y / H) + p1)
    v = amp * np.cos(2 * np.pi * (x / W - 1.5 * y / H) + p2)
    m = (x >= 0.35 * W).astype(np.float32)
    return np.stack([u * m, v * m])[None].astype(np.float32)


# ------------------------------------------------------------------------------ 1. the backward bench.py times

TH, TW = 768, 1280


@pytest.fixture(scope="module")
def timed(oracle):
    """The three flows of bench.py's backward_roofline at 768x1280 -- the Euler t=59 one with the edge cases of
    test_backward_blocks_whose_boxes_do_not_fit planted inside a block of the corner-pair path -- and 65 planes of input / gradOutput."""
    m = smooth_motion(TH, TW)
    flows = {"identity": np.zeros_like(m), "t30": oracle.euler_integration(m, 30)[0], "t59": oracle.euler_integration(m, 59)[0]}
    f = flows["t59"]
    cls = F64.backward_block_classes(f)
    j, i = [int(v) for v in np.argwhere(cls[0] == F64.CLASSES.index("bent_no_fit"))[0]]
    y0, x0 = j * F64.TILE_H, i * F64.TILE_W
    targets = [(-0.5, 0.25),                    # x0 = -1, y0 = 0: only NE / SE, the top pair starts before the plane
               (TW - 0.5, TH - 0.75),           # x0 + 1 = W in the last row: only NW, the top pair ends past the plane
               (TW - 0.25, TH - 1.5),           # x0 + 1 = W, y0 = H - 2: the bottom pair ends past the plane
               (-0.75, -0.5),                   # x0 = y0 = -1: only SE = the plane's first pixel
               (-7.0, 3.0), (12.0, TH + 4.0)]   # destinations outside the image
    planted = []
    for k, (tx, ty) in enumerate(targets):
        y, x = y0 + 1 + k, x0 + 5 + 9 * k
        f[0, 0, y, x], f[0, 1, y, x] = tx - x, ty - y
        assert np.float32(x) + f[0, 0, y, x] == np.float32(tx) and np.float32(y) + f[0, 1, y, x] == np.float32(ty)
        planted.append((y, x))
    f[0, 0, y0 + 7, x0 + 60] = np.nan
    planted.append((y0 + 7, x0 + 60))
    paths = {k: F64.backward_block_paths(v) for k, v in flows.items()}
    assert paths["identity"]["straight"] == 1920
    assert F64.backward_block_classes(f)[0, j, i] == F64.CLASSES.index("bent_no_fit")
    assert all(paths["t59"][k] > 0 for k in F64.CLASSES), paths["t59"]          # every loop of the kernel in one launch
    assert all(paths["t30"][k] > 0 for k in ("straight", "staged1", "staged2", "staged3", "staged4", "staged6", "empty")), paths["t30"]
    rng = np.random.default_rng(65)
    x = rng.standard_normal((1, 65, TH, TW), dtype=np.float32)
    go = rng.standard_normal((1, 65, TH, TW), dtype=np.float32)
    return dict(flows=flows, x=x, go=go, planted=planted, paths=paths)


def group_split(C):
    """Channels per group as slr_softsplat_backward_ws deals them on a grid larger than the chip (csrc/grad.hip: grad_groups, cper)."""
    groups = max(1, min(2, C // 8))
    cper = -(-(-(-C // groups)) // 4) * 4 if groups > 1 else C
    return [min(cper, C - b) for b in range(0, C, cper)]


def backward_all_routes(S, oracle, x, flow, go, tag):
    """Both gradients / input only / flow only through slr_softsplat_backward_ws with its workspace, the autograd route, and
    slr_softsplat_backward without scratch (one group), against the oracle.  -> worst gradFlow deviation / scale."""
    from slr_sfs_amd._lib import check, lib, ptr, stream_of
    L = lib()
    N, C, H, W = x.shape
    nb = int(L.slr_softsplat_backward_ws_bytes(N, C, H, W))
    split = group_split(C)
    assert nb == (len(split) - 1) * N * 2 * H * W * 4, (nb, split)
    X, F, G = dev(x), dev(flow), dev(go)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    st = stream_of(X)
    gi, gf = [torch.full_like(X, float("nan")) for _ in range(3)], [torch.full_like(F, float("nan")) for _ in range(3)]
    check(L.slr_softsplat_backward_ws(ptr(X), ptr(F), ptr(G), ptr(gi[0]), ptr(gf[0]), N, C, H, W, ptr(ws), nb, st), "both")
    check(L.slr_softsplat_backward_ws(ptr(X), ptr(F), ptr(G), ptr(gi[1]), None, N, C, H, W, ptr(ws), nb, st), "input")
    check(L.slr_softsplat_backward_ws(ptr(X), ptr(F), ptr(G), None, ptr(gf[1]), N, C, H, W, ptr(ws), nb, st), "flow")
    check(L.slr_softsplat_backward(ptr(X), ptr(F), ptr(G), ptr(gi[2]), ptr(gf[2]), N, C, H, W, st), "one group")
    a, b = X.clone().requires_grad_(True), F.clone().requires_grad_(True)
    S.softsplat._FunctionSoftsplat.apply(a, b).backward(G)
    torch.cuda.synchronize()
    ogi, ogf = oracle.softsplat_backward(x, flow, go)
    scale = max(1.0, float(np.abs(ogf).max()))
    d_ws, d_one = float(np.abs(host(gf[0]) - ogf).max()), float(np.abs(host(gf[2]) - ogf).max())
    print(f"backward {tag} [{N},{C},{H},{W}] groups {split}: gradFlow max|dev| with groups {d_ws:.3e}, one group {d_one:.3e}, "
          f"max|gradFlow| {float(np.abs(ogf).max()):.3e}")
    assert torch.equal(gi[0], gi[1]) and torch.equal(gf[0], gf[1]), "one launch for both != the single launches"
    assert torch.equal(a.grad, gi[0]) and torch.equal(b.grad, gf[0]), "autograd route != C ABI"
    assert torch.equal(gi[2], gi[0]), "gradInput depends on the grouping"
    assert np.array_equal(host(gi[0]), ogi)
    np.testing.assert_allclose(host(gf[0]), ogf, rtol=2e-6, atol=2e-6 * scale)
    np.testing.assert_allclose(host(gf[2]), ogf, rtol=1e-6, atol=1e-6 * scale)
    return ogi, ogf, host(gi[0]), host(gf[0])


@pytest.mark.parametrize("kind,C", [("identity", 65), ("t30", 65), ("t59", 65), ("identity", 16), ("t30", 17), ("t59", 15)])
def test_backward_at_the_timed_shapes(S, oracle, timed, kind, C):
    """[1,C,768,1280], the flows of bench.py's backward_roofline.  C = 65: two channel groups of 36 + 29 planes, the second with a
    one-channel tail pass, group 0 writes gradFlow, group 1 goes through the partial sums; 16: 8 + 8, no tail; 17: 12 + 5; 15: one group.
    gradInput bit-identical to the oracle's, gradFlow within 2e-6 (groups) / 1e-6 (one group) of max(1, max|ref|)."""
    assert group_split(65) == [36, 29] and group_split(16) == [8, 8] and group_split(17) == [12, 5] and group_split(15) == [15]
    flow = timed["flows"][kind]
    x, go = np.ascontiguousarray(timed["x"][:, 65 - C:]), np.ascontiguousarray(timed["go"][:, 65 - C:])
    ogi, ogf, gi, gf = backward_all_routes(S, oracle, x, flow, go, kind)
    if kind == "t59":
        (ya, xa), (yb, xb), (yc, xc), (yd, xd), (ye, xe), (yf, xf), (yn, xn) = timed["planted"]
        for (y, x_) in ((ya, xa), (yb, xb), (yc, xc), (yd, xd)):               # the planted corners carry gradient ...
            assert np.abs(ogi[0, :, y, x_]).max() > 0 and np.abs(ogf[0, :, y, x_]).max() > 0
        for (y, x_) in ((ye, xe), (yf, xf), (yn, xn)):                          # ... outside the image and NaN: exactly none
            assert (gi[0, :, y, x_] == 0).all() and (gf[0, :, y, x_] == 0).all()


def test_backward_at_the_timed_shape_batch_of_two(S, oracle, timed):
    """[2,16,768,1280]: two channel groups per sample (blockIdx.y with groups), sample 0 on the Euler t=30 flow, sample 1 on t=59."""
    flow = np.concatenate([timed["flows"]["t30"], timed["flows"]["t59"]])
    x = np.ascontiguousarray(timed["x"][0, :32].reshape(2, 16, TH, TW))
    go = np.ascontiguousarray(timed["go"][0, 32:64].reshape(2, 16, TH, TW))
    backward_all_routes(S, oracle, x, flow, go, "t30+t59")


# ------------------------------------------------------------------------------ 2. the modes' gradients against float64

LEDGER = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for key in sorted(LEDGER):
        e_gpu, e_32, scale, where = LEDGER[key]
        print(f"worst {key[0]:>9s} d/d{key[1]:<6s}: E_gpu {e_gpu:.2e}  E_plain32 {e_32:.2e}  scale {scale:.2e}  ({where})")


def judge(group, name, got_gpu, got32, ref64, where):
    """E_gpu <= 10 * E_plain32 + 1e-6, E relative to max|ref64|.  A gradient that is identically zero (the metric's and, in the
    normalised modes, the flow's where every destination has one source: the output then depends on neither, and |ref64| is the
    float64 noise of terms that cancel, below 1e-9) has no scale of its own: the same inequality then holds on the scale 1 of the
    terms."""
    ref64 = ref64.double()
    scale = float(ref64.abs().max())
    err_gpu, err_32 = float((got_gpu.double().cpu() - ref64).abs().max()), float((got32.double() - ref64).abs().max())
    s = scale if scale > 1e-9 else 1.0
    e_gpu, e_32 = err_gpu / s, err_32 / s
    print(f"  {where} {group} d/d{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_32:.3e}  scale {scale:.3e}")
    if (group, name) not in LEDGER or e_gpu > LEDGER[(group, name)][0]:
        LEDGER[(group, name)] = (e_gpu, e_32, scale, where)
    assert e_gpu <= 10 * e_32 + 1e-6, (where, group, name, e_gpu, e_32, scale)


def reference_grads(x, flow, met, mode, go, dtype, cot=None):
    """Gradients of the plain definition in `dtype`.  The cotangent (made once, from the float64 run) is go * clamp(norm, max=1) with
    the float64 normaliser as a constant: without it a handful of barely reached pixels with 1/norm ~ 1e3 set the scale of the whole
    gradFlow tensor and hide everything else."""
    leaves = {"input": torch.from_numpy(x).to(dtype).requires_grad_(True), "flow": torch.from_numpy(flow).to(dtype).requires_grad_(True)}
    if mode in ("linear", "softmax"):
        leaves["metric"] = torch.from_numpy(met).to(dtype).requires_grad_(True)
    threads = torch.get_num_threads()
    if x.size < 2 ** 20:                        # (small cases: a thread team costs more than the work)
        torch.set_num_threads(1)
    try:
        out, norm = F64.function_softsplat(leaves["input"], leaves["flow"], leaves.get("metric"), mode, dtype, return_norm=True)
        if cot is None:
            cot = torch.from_numpy(go).double()
            if norm is not None:
                cot = cot * norm.detach().clamp(max=1.0)
            cot = cot.float()
        grads = torch.autograd.grad(out, list(leaves.values()), cot.to(dtype))
    finally:
        torch.set_num_threads(threads)
    return dict(zip(leaves, grads)), cot


def gpu_grads(S, x, flow, met, mode, cot, subset):
    leaves = {"input": dev(x), "flow": dev(flow)}
    if mode in ("linear", "softmax"):
        leaves["metric"] = dev(met)
    for k in subset:
        leaves[k].requires_grad_(True)
    out = S.FunctionSoftsplat(leaves["input"], leaves["flow"], leaves.get("metric"), mode)
    out.backward(cot.cuda())
    return {k: v.grad for k, v in leaves.items()}


class pinned_forward:
    """The forward splat hands out its entry slots with atomics: its sums differ in the last bits from call to call (the reference's
    own order is unspecified: racing atomicAdds), and in the normalised modes the gradients are functions of that forward result.
    So that runs with different sets of inputs requiring grad can be compared bit for bit, the forward result is pinned inside this
    context: a second call of softsplat._splat_sum on the same bits returns the first call's result.  Everything else -- the torch
    composition, _FunctionSoftsplat.backward and the kernel variant its needs_input_grad selects -- runs as it is."""

    def __init__(self, S):
        self.mod, self.seen = S.softsplat, []

    def __enter__(self):
        self.orig = orig = self.mod._splat_sum
        bits = lambda t: t.detach().contiguous().view(torch.int32)

        def pinned(input, flow):
            for (i, f, o) in self.seen:
                if i.shape == input.shape and torch.equal(i, bits(input)) and torch.equal(f, bits(flow)):
                    return o.clone()
            out = orig(input, flow)
            self.seen.append((bits(input).clone(), bits(flow).clone(), out.clone()))
            return out
        self.mod._splat_sum = pinned
        return self

    def __exit__(self, *exc):
        self.mod._splat_sum = self.orig


def check_mode_gradients(S, x, flow, met, mode, go, where):
    """One case of FunctionSoftsplat(mode) with autograd: the three gradients against float64 by the criterion above, exact zeros at
    dropped pixels, and every subset of the inputs that requires grad gives the same bits.  Returns False (nothing asserted) when the
    inputs do not meet the condition stated with the reference alone: per gradient tensor at least 30 % of the elements at or above
    1e-3 * max|ref64|, ref64 finite, gradInput not identically zero (something lands in the image)."""
    ref, cot = reference_grads(x, flow, met, mode, go, torch.float64)
    for k, r in ref.items():
        if not bool(torch.isfinite(r).all()):
            return False
        mx = float(r.abs().max())
        if mx <= 1e-9 and k == "input":
            return False
        if mx > 1e-9 and float((r.abs() >= 1e-3 * mx).double().mean()) < 0.30:
            return False
    p32, _ = reference_grads(x, flow, met, mode, go, torch.float32, cot)
    names = list(ref)
    with pinned_forward(S) as pin:
        full = gpu_grads(S, x, flow, met, mode, cot, names)
        for k in names:
            judge(mode, k, full[k], p32[k], ref[k], where)
        dropped = torch.from_numpy(~np.isfinite(flow).all(axis=1))[:, None].cuda()
        for k in ("input", "flow"):
            assert bool((full[k][dropped.expand_as(full[k])] == 0).all()), (where, mode, k, "gradient at a pixel with a non-finite flow")
        for r in range(1, len(names)):
            for subset in itertools.combinations(names, r):
                g = gpu_grads(S, x, flow, met, mode, cot, subset)
                for k in names:
                    if k in subset:
                        assert torch.equal(g[k], full[k]), (where, mode, subset, k)
                    else:
                        assert g[k] is None, (where, mode, subset, k)
        assert len(pin.seen) == 1               # (every run splatted the same bits)
    # the same without the pin (another summation order of the forward): still the float64 gradients, by the same criterion
    again = gpu_grads(S, x, flow, met, mode, cot, names[:1])
    judge(mode, names[0], again[names[0]], p32[names[0]], ref[names[0]], where + " (again)")
    return True


FAMILIES = ("uniform3", "uniform60", "integer", "collapse", "euler30", "euler59", "nan", "zero_norm")
SHAPES = ((1, 1, 1, 1), (2, 3, 5, 1), (1, 17, 9, 65), (2, 6, 40, 72), (1, 64, 256, 480), (2, 65, 256, 256))


def family_case(oracle, kind, shape, mode, seed, s):
    """Seeded inputs of one case; `s` scales the family's amplitude (1, then halved while the condition on the inputs is not met).
    The families are those of tests/test_gpu_frontends.py::test_randomised_sweep; the Euler flows integrate smooth_motion at the
    amplitude bench.py's flows have (1.5); the metric has spread 0.7 (with spread 2 too few elements carry gradient)."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    met = (rng.standard_normal((N, 1, H, W)) * 0.7).astype(np.float32)
    if mode == "linear":
        met = np.abs(met) + np.float32(0.1)
    if kind == "uniform3":
        fl = rng.uniform(-3 * s, 3 * s, (N, 2, H, W))
    elif kind == "uniform60":
        fl = rng.uniform(-60 * s, 60 * s, (N, 2, H, W))
    elif kind == "integer":
        r = int(round(5 * s))
        fl = rng.integers(-r, r + 1, (N, 2, H, W)).astype(np.float32)
    elif kind == "collapse":
        fl = np.stack([(W / 2 - x) * rng.uniform(0.5, 1.0) * s, (H / 2 - y) * rng.uniform(0.5, 1.0) * s])[None].repeat(N, 0)
    elif kind in ("euler30", "euler59"):
        fl = np.concatenate([oracle.euler_integration(smooth_motion(H, W, seed + n, amp=1.5 * s), int(kind[-2:]))[0] for n in range(N)])
    elif kind == "nan":
        fl = rng.uniform(-2 * s, 2 * s, (N, 2, H, W))
        fl[rng.random(fl.shape) < 0.02] = np.nan
        if H * W >= 64:
            fl[0, 0, H // 2, W // 2], fl[N - 1, 1, H // 3, W // 3], fl[0, :, H - 1, W - 1] = np.nan, np.inf, (3.0e9, -np.inf)
    else:
        # every source stays within half a pixel of itself, except around two destinations: P receives exactly its own source and its
        # right neighbour's (integer flows, weight 1 each) with metrics +a and -a in linear mode -- a normaliser of exactly 0 --, and
        # nobody reaches Q; their other neighbours leave the image
        assert H >= 7 and W >= 9
        fl = rng.uniform(-0.45 * s, 0.45 * s, (N, 2, H, W))
        py, px, qy, qx = 2, 3, H - 3, W - 4
        for n in range(N):
            fl[n, :, py - 1:py + 2, px - 1:px + 2] = 1.0e4
            fl[n, :, py, px] = 0.0
            fl[n, :, py, px + 1] = (-1.0, 0.0)
            fl[n, :, qy - 1:qy + 2, qx - 1:qx + 2] = 1.0e4
            if mode == "linear":
                met[n, 0, py, px], met[n, 0, py, px + 1] = 0.5, -0.5
    v = rng.standard_normal((N, C, H, W)).astype(np.float32)
    go = rng.standard_normal((N, C, H, W)).astype(np.float32)
    return v, fl.astype(np.float32), met, go


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("kind", FAMILIES)
def test_mode_gradients_vs_float64(S, oracle, kind, shape):
    """FunctionSoftsplat with autograd in every mode, gradients w.r.t. input, flow and metric.  A case whose inputs do not meet the
    condition of check_mode_gradients is re-seeded, then re-scaled (three seeds per amplitude, the amplitude halved after them)."""
    case = SHAPES.index(shape)
    if kind == "zero_norm" and (shape[2] < 7 or shape[3] < 9):
        shape = shape[:2] + (7, 9)              # (the planted destinations and their neighbourhoods need 7 x 9 pixels)
    H, W = shape[2:]
    for mode in MODES:
        for attempt in range(60):
            seed, s = 1000 * FAMILIES.index(kind) + 10 * case + 100000 * attempt, 0.5 ** (attempt // 3)
            v, fl, met, go = family_case(oracle, kind, shape, mode, seed, s)
            where = f"{kind} {'x'.join(str(n) for n in shape)} seed {seed} amplitude {s:g}"
            if check_mode_gradients(S, v, fl, met, mode, go, where):
                break
        else:
            raise AssertionError(f"no seed / amplitude of {kind} {shape} {mode} meets the condition on the inputs")
        if kind == "zero_norm":
            out = S.FunctionSoftsplat(dev(v), dev(fl), dev(met), mode)
            assert bool((out[:, :, H - 3, W - 4] == 0).all())                  # nobody reaches Q
            if mode == "linear":                # P: the normaliser is exactly 0 and divides as 1
                assert np.array_equal(host(out[:, :, 2, 3]), v[:, :, 2, 3] * np.float32(0.5) + v[:, :, 2, 4] * np.float32(-0.5))


# ------------------------------------------------------------------------------ 4. Euler backward at the training shape

def euler_bound(oracle, m, n, weight):
    """The backward of the integration is a pure scatter with coefficient 1 (csrc/euler.hip): a cell of grad_motion is the sum of the K
    output gradients of the paths that gathered from it.  Two float32 summations of the same K terms in different orders differ by at
    most 2 (K - 1) 2^-24 A, A the sum of their magnitudes.  -> (A, K) for `weight` = |gradient of the displacements|."""
    return oracle.euler_backward(m, n, np.abs(weight)), oracle.euler_backward(m, n, np.ones_like(weight))


@pytest.mark.parametrize("steps", [(30, 59), (1, 0)])
def test_euler_backward_at_the_training_shape(S, oracle, steps):
    """[2,2,256,256], per-sample step counts, through EulerIntegration (one launch for the batch) and per sample through
    euler_integration, against oracle.euler_backward within 2 (K - 1) 2^-24 A + 1e-7 per cell."""
    H = W = 256
    mo = np.concatenate([smooth_motion(H, W, 11 + b, amp=2.0) for b in range(2)])
    go = np.random.default_rng(7).standard_normal((2, 2, H, W)).astype(np.float32)
    m = dev(mo).requires_grad_(True)
    d = S.EulerIntegration()(m, torch.tensor(steps).cuda())
    d.backward(dev(go))
    gm = host(m.grad)
    for b, n in enumerate(steps):
        ref = oracle.euler_backward(mo[b:b + 1], n, go[b:b + 1])
        A, K = euler_bound(oracle, mo[b:b + 1], n, go[b:b + 1])
        bound = 2.0 * np.maximum(K - 1.0, 0.0) * 2.0 ** -24 * A + 1e-7
        m1 = dev(mo[b:b + 1]).requires_grad_(True)
        d1, _ = S.euler_integration(m1, n)
        assert np.array_equal(host(d1), oracle.euler_integration(mo[b:b + 1], n)[0]) and torch.equal(d1, d[b:b + 1])
        d1.backward(dev(go[b:b + 1]))
        for name, got in (("batch", gm[b:b + 1]), ("one sample", host(m1.grad))):
            dev_ = np.abs(got - ref)
            print(f"euler backward {name} sample {b} n={n}: max|dev| {float(dev_.max()):.3e}, max K {float(K.max()):.0f}, max|ref| "
                  f"{float(np.abs(ref).max()):.3e}, max dev/bound {float((dev_ / bound).max()):.3f}")
            assert (dev_ <= bound).all(), (name, b, n, float((dev_ - bound).max()))
        if n == 0:
            assert not gm[b].any()


# ------------------------------------------------------------------------------ 3. the training step as a chain

def test_training_step_chain_gradients(S, oracle):
    """models/animating_softmax_splating.py:579-606, 628, 651, 672-678, 691-692 built from the package's drop-ins as the reference's
    forward() builds it, on [2,65,256,256]-shaped data with step counts (30, 59) of 60 on the device: gradients of a seeded linear
    loss w.r.t. fs, Z and the motion field.  Reference: the oracle's displacement fields (the GPU's are bit-equal), splat_f64.
    training_step in float64 for d/dfs, d/dZ and d/d(both fields), oracle.euler_backward of the two field gradients for d/dmotion.
    The whole step runs without a host synchronisation."""
    B, C, H, W, NF = 2, 64, 256, 256, 60
    t = (30, 59)
    rng = np.random.default_rng(2024)
    fs = rng.standard_normal((B, C, H, W)).astype(np.float32)
    Z = rng.standard_normal((B, 1, H, W)).astype(np.float32)
    mo = np.concatenate([smooth_motion(H, W, 21 + b, amp=2.0) for b in range(B)])
    go = rng.standard_normal((B, C, H, W)).astype(np.float32)
    of = np.concatenate([oracle.euler_integration(mo[b:b + 1], t[b])[0] for b in range(B)])
    op = np.concatenate([oracle.euler_integration(-mo[b:b + 1], NF - t[b])[0] for b in range(B)])
    start, middle, end = torch.zeros(B).cuda(), torch.tensor([float(v) for v in t]).cuda(), torch.full((B,), NF - 1.0).cuda()

    def blend():                                # :585-586
        return (1.0 - (middle.float() - start.float()).float() / (end.float() - start.float() + 1.0).float()).view(B, 1, 1, 1)
    alpha = blend().cpu()
    assert alpha[0].item() == 0.5 and abs(alpha[1].item() - 1.0 / 60.0) < 1e-6

    def plain(dtype, cot=None):
        lv = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (fs, Z, of, op)]
        out, norm = F64.training_step(lv[0], lv[1], lv[2], lv[3], alpha, dtype, return_norm=True)
        if cot is None:                         # (the damped cotangent of check_mode_gradients: a seeded linear loss)
            cot = (torch.from_numpy(go).double() * norm.detach().clamp(max=1.0)).float()
        return torch.autograd.grad(out, lv, cot.to(dtype)), cot
    r64, cot = plain(torch.float64)
    r32, _ = plain(torch.float32, cot)
    for name, r in zip(("fs", "Z", "flow_f", "flow_p"), r64):
        mx = float(r.abs().max())
        assert bool(torch.isfinite(r).all()) and float((r.abs() >= 1e-3 * mx).double().mean()) >= 0.30, (name, mx)

    euler, splat = S.EulerIntegration(), S.ModuleSoftsplat("summation")
    fs_d, Z_d, mo_d = dev(fs).requires_grad_(True), dev(Z).requires_grad_(True), dev(mo).requires_grad_(True)
    cot_d, alpha_ref = cot.cuda(), alpha.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        flow_f = euler(mo_d, middle.long() - start.long())                                         # :579
        flow_p = euler(-mo_d, end.long() + 1 - middle.long())                                      # :580
        a = blend()
        Z_norm = torch.clamp(Z_d - Z_d.max(), min=-20.0, max=20.0)                                 # :601-605
        ones = fs_d.new_ones((B, 1, H, W))
        ten_f = torch.cat([fs_d * Z_norm.exp() * a, Z_norm.exp() * a], 1)                          # :606
        gen_f = splat(tenInput=ten_f, tenFlow=flow_f, tenMetric=ones)                              # :628
        ten_norm, gen = gen_f[:, -1:, :, :], gen_f[:, :-1, :, :]                                   # :632-634
        ten_p = torch.cat([fs_d * Z_norm.exp() * (1 - a), Z_norm.exp() * (1 - a)], 1)              # :651
        gen_p = splat(tenInput=ten_p, tenFlow=flow_p, tenMetric=ones)                              # :672
        ten_norm += gen_p[:, -1:, :, :]                                                            # :676 (in place on the view, as upstream)
        gen += gen_p[:, :-1, :, :]                                                                 # :678
        gen = gen / torch.clamp(ten_norm, min=1e-8)                                                # :691-692
        flow_f.retain_grad()
        flow_p.retain_grad()
        (gen * cot_d).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, alpha_ref)
    assert np.array_equal(host(flow_f), of) and np.array_equal(host(flow_p), op)
    out64 = F64.training_step(torch.from_numpy(fs), torch.from_numpy(Z), torch.from_numpy(of), torch.from_numpy(op), alpha)
    np.testing.assert_allclose(host(gen), out64.numpy(), rtol=1e-4, atol=1e-5)
    judge("training", "fs", fs_d.grad, r32[0], r64[0], "chain")
    judge("training", "Z", Z_d.grad, r32[1], r64[1], "chain")
    judge("training", "flow_f", flow_f.grad, r32[2], r64[2], "chain")
    judge("training", "flow_p", flow_p.grad, r32[3], r64[3], "chain")
    # d/dmotion: the two field gradients carried back along the paths of the integration (the second field integrates -motion).
    # Bound per cell: the summation-order bound of test_euler_backward_at_the_training_shape over both directions' terms, plus the
    # difference between the GPU's field gradients and the reference's (the rounding of the splat backward) carried along the same paths.
    gf_ref, gp_ref = r64[2].float().numpy(), r64[3].float().numpy()
    gf_gpu, gp_gpu = host(flow_f.grad), host(flow_p.grad)
    gm = host(mo_d.grad)
    for b in range(B):
        mb, nf, np_ = mo[b:b + 1], t[b], NF - t[b]
        ref = oracle.euler_backward(mb, nf, gf_ref[b:b + 1]) - oracle.euler_backward(-mb, np_, gp_ref[b:b + 1])
        Af, Kf = euler_bound(oracle, mb, nf, gf_ref[b:b + 1])
        Ap, Kp = euler_bound(oracle, -mb, np_, gp_ref[b:b + 1])
        carried = oracle.euler_backward(mb, nf, np.abs(gf_gpu[b:b + 1] - gf_ref[b:b + 1])) + \
            oracle.euler_backward(-mb, np_, np.abs(gp_gpu[b:b + 1] - gp_ref[b:b + 1]))
        bound = 2.0 * np.maximum(Kf + Kp - 1.0, 0.0) * 2.0 ** -24 * (Af + Ap) + 1e-7 + carried
        dev_ = np.abs(gm[b:b + 1] - ref)
        print(f"chain d/dmotion sample {b}: max|dev| {float(dev_.max()):.3e}, max|ref| {float(np.abs(ref).max()):.3e}, "
              f"max dev/bound {float((dev_ / bound).max()):.3f}, max carried {float(carried.max()):.3e}")
        assert float(np.abs(ref).max()) > 1.0
        assert (dev_ <= bound).all(), (b, float((dev_ - bound).max()))
