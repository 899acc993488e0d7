"""The two-direction Euler operator on the GPU (csrc/euler.hip, ABI 28): slr_euler_pair_forward / slr_euler_pair_backward and
``euler_integration_pair``.

Shapes [2,2,20,24] and [1,2,33,31] (H != W, pixel counts that are no multiple of 256, one and two workgroups per plane) and one case at
[2,2,256,256]; step counts from {0, 1, 30, 59}, different between directions and samples.  Motion fields: zero, a constant that drives
every pixel out, smooth, incoherent random, and a sink (a field converging on one point: every path ends in a few cells; the second sample
of a batch carries the negated sink, which converges in the backward direction).

  1. forward: the bits of EulerIntegration on motion and on -motion.
  2. backward against oracle.euler_backward per direction, combined with the signs in float64.  Per cell with K visits and exact sum s the
     kernel's bound is  Q + 2^-24 (|s| + Q),  Q = K 2^(e-F-1)  (csrc/euler.hip, RESOLUTION), written out below from the {e, F} the kernel
     leaves in its workspace.  The oracle sums each direction in float32, one term after the other, which at a cell with a million visits
     is off by far more than the kernel: ``exact_backward`` calls it on pieces of the gradient that float32 adds exactly and adds the
     pieces in float64, so the reference's own error is zero (it is carried in the bound all the same).  With gradients that are
     multiples of 2^-6 (2^-1 at 256 x 256) the oracle's plain result is exact as well, and the kernel's must equal it bit for bit.
  3. reproducibility: twenty calls, a sample alone and in a batch, the directions exchanged.
  4. one NaN / one +Inf: non-finite exactly on that pixel's path, every other element the bits of the clean run.
  5. autograd: the entry point's bits; no backward launch without a gradient to compute.
Every figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = [((2, 2, 20, 24), (30, 1), (0, 59)), ((1, 2, 33, 31), (59,), (30,))]
BIG = ((2, 2, 256, 256), (30, 1), (0, 59))
KINDS = ("zero", "out", "smooth", "random", "sink")


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


def steps_dev(steps):
    return torch.tensor(steps, dtype=torch.int64).cuda()


def motion_of(kind, shape, seed):
    B, _, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    out = np.zeros(shape, np.float32)
    for b in range(B):
        if kind == "out":
            out[b] = float(H + W)
        elif kind == "smooth":
            p1, p2 = rng.uniform(0, 2 * np.pi, 2)
            out[b, 0] = 1.5 * np.sin(2 * np.pi * (2 * x / W + y / H) + p1) * (x >= 0.35 * W)
            out[b, 1] = 1.5 * np.cos(2 * np.pi * (x / W - 1.5 * y / H) + p2) * (x >= 0.35 * W)
        elif kind == "random":
            out[b] = rng.uniform(-3.0, 3.0, (2, H, W))
        elif kind == "sink":
            cx, cy = 0.37 * W + 0.3, 0.58 * H + 0.2
            sign = 1.0 if b == 0 else -1.0                      # sample 1 converges in the backward direction
            out[b, 0], out[b, 1] = sign * 0.3 * (cx - x), sign * 0.3 * (cy - y)
    return out


def gradients_of(shape, seed, dyadic=0):
    rng = np.random.default_rng(seed)
    if dyadic:                                                  # multiples of 1 / dyadic in [-1, 1]
        return [(rng.integers(-dyadic, dyadic + 1, shape) / float(dyadic)).astype(np.float32) for _ in range(2)]
    return [rng.standard_normal(shape).astype(np.float32) for _ in range(2)]


def pair_backward(S, motion, steps_f, steps_p, gf, gp):
    """The entry point on device tensors -> (grad_motion, [(e, F, largest finite |g|)] per sample, read from the workspace's header)."""
    B, _, H, W = motion.shape
    nbytes = int(S._lib.lib().slr_euler_pair_workspace_bytes(B, H, W))
    assert nbytes == B * (1280 + 24 * H * W)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=motion.device)
    out = torch.full_like(motion, float("nan"))                 # (every element must be written)
    S._lib.call("slr_euler_pair_backward", motion.device, motion, steps_f, steps_p, B, H, W, gf, gp, out, ws, nbytes)
    head = ws[:B * 160].cpu().numpy().view(np.int32).reshape(B, 320)[:, :4]
    info = [(int(h[0]), int(h[1]), float(np.array([h[2]], np.int32).view(np.float32)[0])) for h in head]
    return out, info


def expected_scale(gf, gp, nf, np_, HW):
    """{e, F} as include/slr_splat.h documents them."""
    g = np.abs(np.concatenate([gf.ravel(), gp.ravel()]).astype(np.float64))
    g = g[np.isfinite(g)]
    M = float(g.max()) if g.size else 0.0
    e = int(np.frexp(M)[1]) if M > 0 else 0
    A = (nf + np_) * HW
    L = 0 if A <= 1 else int(A - 1).bit_length()
    return e, min(60, 63 - L), M


def exact_backward(oracle, m, n, g, K):
    """oracle.euler_backward(m, n, g) without its float32 summation error.  g is cut into pieces of a few bits each -- multiples of 2^-s of
    at most 2^bits units, with K 2^bits <= 2^23 for the direction's largest visit count K -- so that every partial sum of the oracle's
    float32 accumulation is an integer below 2^24 in the piece's unit: each call is exact, and the pieces are added in float64.  What is
    left of g after 48 pieces (nothing, for float32 values of ordinary range) is summed as it is and its error bound returned.
    -> (sum [2,H,W] float64, bound on its error [2,H,W])"""
    bits = max(1, 23 - int(np.ceil(np.log2(max(float(K.max()), 1.0)))))
    r = g.astype(np.float64)
    total = np.zeros(g.shape[1:], np.float64)
    top = float(np.abs(r).max())
    if top == 0.0 or n == 0:
        return total, total.copy()
    s = bits - int(np.ceil(np.log2(top))) - 1
    for _ in range(48):
        piece = np.round(np.ldexp(r, s))
        assert np.abs(piece).max() <= 2 ** bits
        piece = np.ldexp(piece, -s)
        assert np.array_equal(piece.astype(np.float32).astype(np.float64), piece)
        total += oracle.euler_backward(m, n, piece.astype(np.float32))[0].astype(np.float64)
        r = r - piece
        if not r.any():
            return total, np.zeros_like(total)
        s += bits
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r)
    total += oracle.euler_backward(m, n, r.astype(np.float32))[0].astype(np.float64)
    left = np.maximum(K - 1.0, 0.0) * 2.0 ** -24 * oracle.euler_backward(m, n, np.abs(r).astype(np.float32))[0].astype(np.float64) * (1 + 2.0 ** -10)
    return total, left


_cases = {}


def case(oracle, kind, shape, steps_f, steps_p, dyadic=0):
    """Inputs and the float64 reference of one case, computed once."""
    key = (kind, shape, dyadic)
    if key in _cases:
        return _cases[key]
    B, _, H, W = shape
    seed = 9100 + 17 * KINDS.index(kind) + H
    mo = motion_of(kind, shape, seed)
    gf, gp = gradients_of(shape, seed + 1, dyadic)
    ref, K, err = np.zeros(shape, np.float64), np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    for b in range(B):
        for m, n, g, sign in ((mo[b:b + 1], steps_f[b], gf[b:b + 1], 1.0), (-mo[b:b + 1], steps_p[b], gp[b:b + 1], -1.0)):
            Kd = oracle.euler_backward(m, n, np.ones_like(g))[0].astype(np.float64)
            assert Kd.max() < 2 ** 23                           # the visit counts are exact in the oracle's float32
            total, left = exact_backward(oracle, m, n, g, Kd)
            ref[b] += sign * total
            K[b] += Kd
            err[b] += left
    c = dict(motion=mo, gf=gf, gp=gp, ref=ref, K=K, ref_err=err, steps_f=steps_f, steps_p=steps_p, shape=shape)
    _cases[key] = c
    return c


ALL = [(kind,) + s for kind in KINDS for s in SMALL] + [("sink",) + BIG]
IDS = [f"{k}-{'x'.join(map(str, s))}" for k, s, _, _ in ALL]


@pytest.mark.parametrize("kind,shape,steps_f,steps_p", ALL, ids=IDS)
def test_forward_is_euler_integration_on_both_signs(S, kind, shape, steps_f, steps_p):
    mo = dev(motion_of(kind, shape, 9100 + 17 * KINDS.index(kind) + shape[2]))
    sf, sp = steps_dev(steps_f), steps_dev(steps_p)
    flow_f, flow_p = S.euler_integration_pair(mo, sf, sp)
    E = S.EulerIntegration()
    want_f, vis_f = E(mo, sf, show_visible_pixels=True)
    want_p, vis_p = E(-mo, sp, show_visible_pixels=True)
    assert torch.equal(flow_f.view(torch.int32), want_f.view(torch.int32)) and torch.equal(flow_p.view(torch.int32), want_p.view(torch.int32))
    B, _, H, W = shape
    got_vf, got_vp = torch.empty(B, 1, H, W, device="cuda"), torch.empty(B, 1, H, W, device="cuda")
    d_f, d_p = torch.empty_like(mo), torch.empty_like(mo)
    S._lib.call("slr_euler_pair_forward", mo.device, mo, sf, sp, B, H, W, d_f, d_p, got_vf, got_vp)
    assert torch.equal(d_f, flow_f) and torch.equal(d_p, flow_p) and torch.equal(got_vf, vis_f) and torch.equal(got_vp, vis_p)
    valid = float(vis_f.mean()), float(vis_p.mean())
    print(f"{kind} {shape}: valid forward {valid[0]:.3f}, backward {valid[1]:.3f}")
    if kind == "out":
        assert valid == (0.0, 0.0) or 0 in steps_f + steps_p
    if kind == "zero":
        assert valid == (1.0, 1.0) and not flow_f.any() and not flow_p.any()


@pytest.mark.parametrize("kind,shape,steps_f,steps_p", ALL, ids=IDS)
def test_backward_within_the_derived_bound_of_float64(S, oracle, kind, shape, steps_f, steps_p):
    c = case(oracle, kind, shape, steps_f, steps_p)
    B, _, H, W = shape
    out, info = pair_backward(S, dev(c["motion"]), steps_dev(steps_f), steps_dev(steps_p), dev(c["gf"]), dev(c["gp"]))
    got = host(out).astype(np.float64)
    assert np.isfinite(got).all()
    worst = 0.0
    for b in range(B):
        e, F, M = info[b]
        assert (e, F, M) == expected_scale(c["gf"][b], c["gp"][b], steps_f[b], steps_p[b], H * W), (info[b], b)
        assert 2.0 ** (e - 1) <= M < 2.0 ** e and F >= 33            # 2 n H W <= 2^30 here: at least 32 bits below the largest |g|
        Q = c["K"][b] * 2.0 ** (e - F - 1)
        kernel = Q + 2.0 ** -24 * (np.abs(c["ref"][b]) + Q) + 2.0 ** -149
        bound = kernel + c["ref_err"][b]
        dev_ = np.abs(got[b] - c["ref"][b])
        ratio = float((dev_ / bound).max())
        worst = max(worst, ratio)
        print(f"{kind} {shape} sample {b}: e {e} F {F} max K {c['K'][b].max():.0f} max|ref| {np.abs(c['ref'][b]).max():.3e} max|dev| {dev_.max():.3e} "
              f"max dev/bound {ratio:.3f} (kernel's share of the bound at that cell {float((kernel / bound).ravel()[np.argmax(dev_ / bound)]):.3f}, "
              f"max dev / kernel's bound alone {float((dev_ / kernel).max()):.3f})")
        assert (dev_ <= bound).all(), (b, float((dev_ - bound).max()))
        assert not got[b][c["K"][b] == 0].any()                       # a cell nobody gathered from is exactly zero
    print(f"{kind} {shape}: worst ratio to the bound {worst:.3f}")
    if kind in ("zero", "out"):
        # zero motion: every pixel gathers from itself at every step; all out: nothing arrives anywhere
        want = np.stack([steps_f[b] * c["gf"][b].astype(np.float64) - steps_p[b] * c["gp"][b].astype(np.float64)
                         for b in range(B)]) if kind == "zero" else 0.0
        assert np.array_equal(got, np.broadcast_to(want, got.shape).astype(np.float32))


@pytest.mark.parametrize("kind,shape,steps_f,steps_p", [a for a in ALL if a[0] in ("smooth", "random", "sink")],
                         ids=[i for i, a in zip(IDS, ALL) if a[0] in ("smooth", "random", "sink")])
def test_backward_is_exact_where_the_oracle_is(S, oracle, kind, shape, steps_f, steps_p):
    """Gradients that are multiples of 1 / D within [-1, 1] (D = 64; 2 at 256 x 256, where millions of visits meet in the sink): every
    partial sum of a cell is a multiple of 1 / D below K, and float32 holds it exactly while K D < 2^24 -- the oracle's result is the
    exact sum, and so must the fixed-point sum's be."""
    D = 2 if shape == BIG[0] else 64
    c = case(oracle, kind, shape, steps_f, steps_p, dyadic=D)
    assert c["K"].max() * D < 2 ** 24
    out, _ = pair_backward(S, dev(c["motion"]), steps_dev(steps_f), steps_dev(steps_p), dev(c["gf"]), dev(c["gp"]))
    print(f"{kind} {shape} dyadic: max K {c['K'].max():.0f}, cells that differ {int((host(out) != c['ref']).sum())}")
    assert np.array_equal(host(out).astype(np.float64), c["ref"])


def test_twenty_calls_on_the_sink_are_the_same_bits(S, oracle):
    shape, steps_f, steps_p = BIG
    c = case(oracle, "sink", shape, steps_f, steps_p)
    assert c["K"].max() >= 1000                                      # thousands of paths end in one cell
    args = (dev(c["motion"]), steps_dev(steps_f), steps_dev(steps_p), dev(c["gf"]), dev(c["gp"]))
    first, _ = pair_backward(S, *args)
    for _ in range(19):
        again, _ = pair_backward(S, *args)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("kind", ("smooth", "sink"))
def test_a_sample_alone_and_in_a_batch(S, oracle, kind):
    shape, steps_f, steps_p = SMALL[0]
    c = case(oracle, kind, shape, steps_f, steps_p)
    both, info = pair_backward(S, dev(c["motion"]), steps_dev(steps_f), steps_dev(steps_p), dev(c["gf"]), dev(c["gp"]))
    for b in range(2):
        one = [dev(c[k][b:b + 1]) for k in ("motion", "gf", "gp")]
        alone, info1 = pair_backward(S, one[0], steps_dev(steps_f[b:b + 1]), steps_dev(steps_p[b:b + 1]), one[1], one[2])
        assert info1[0] == info[b] and torch.equal(alone[0].view(torch.int32), both[b].view(torch.int32))
        # ... and as the other sample of the batch
        order = [1 - b, b]
        swapped, _ = pair_backward(S, dev(c["motion"][order]), steps_dev([steps_f[i] for i in order]), steps_dev([steps_p[i] for i in order]),
                                   dev(c["gf"][order]), dev(c["gp"][order]))
        assert torch.equal(swapped[1].view(torch.int32), both[b].view(torch.int32))


@pytest.mark.parametrize("kind", ("random", "sink"))
def test_exchanging_the_directions_negates_the_gradient(S, oracle, kind):
    """(-motion, steps_p, steps_f, gdisp_p, gdisp_f) walks the same paths with every contribution's sign reversed: the negated gradient,
    bit for bit (a zero stays +0: it is compared as a number)."""
    shape, steps_f, steps_p = SMALL[0]
    c = case(oracle, kind, shape, steps_f, steps_p)
    out, info = pair_backward(S, dev(c["motion"]), steps_dev(steps_f), steps_dev(steps_p), dev(c["gf"]), dev(c["gp"]))
    neg, info_n = pair_backward(S, dev(-c["motion"]), steps_dev(steps_p), steps_dev(steps_f), dev(c["gp"]), dev(c["gf"]))
    assert info == info_n and bool(out.any())
    assert torch.equal((-neg + 0.0).view(torch.int32), (out + 0.0).view(torch.int32))


@pytest.mark.parametrize("value", (float("nan"), float("inf")), ids=("nan", "inf"))
@pytest.mark.parametrize("kind", ("smooth", "sink"))
def test_a_non_finite_gradient_stays_on_its_path(S, oracle, kind, value):
    shape, steps_f, steps_p = SMALL[0]
    c = case(oracle, kind, shape, steps_f, steps_p)
    B, _, H, W = shape
    b, ch, n = 0, 1, steps_f[0]
    vis = oracle.euler_integration(c["motion"][b:b + 1], n)[1][0, 0]
    biggest = max(np.abs(c["gf"][b]).max(), np.abs(c["gp"][b]).max())
    ys, xs = np.nonzero((vis == 1) & (np.abs(c["gf"][b, ch]) < biggest) & (c["gf"][b, ch] != 0))
    y, x = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])
    onehot = np.zeros((1, 2, H, W), np.float32)
    onehot[0, ch, y, x] = 1.0
    path = oracle.euler_backward(c["motion"][b:b + 1], n, onehot)[0] != 0
    assert path[ch].any() and not path[1 - ch].any()
    args = (dev(c["motion"]), steps_dev(steps_f), steps_dev(steps_p))
    clean, info = pair_backward(S, *args, dev(c["gf"]), dev(c["gp"]))
    gf = c["gf"].copy()
    gf[b, ch, y, x] = value
    got, info_p = pair_backward(S, *args, dev(gf), dev(c["gp"]))
    assert info_p == info                                                # the planted value is no part of the scale
    mask = np.zeros(shape, bool)
    mask[b] = path
    g, cl = host(got), host(clean)
    print(f"{kind} {value}: pixel ({y}, {x}), {int(mask.sum())} cells on its path, {int((~np.isfinite(g)).sum())} non-finite in the result")
    assert np.array_equal(~np.isfinite(g), mask)
    assert np.array_equal(g.view(np.int32)[~mask], cl.view(np.int32)[~mask])
    if np.isnan(value):
        assert (g.view(np.uint32)[mask] == 0x7FC00000).all()            # canonical
    else:
        assert (g[mask] == np.inf).all()
        # ... and -Inf through the backward direction (its sign is -1)
        gp = c["gp"].copy()
        b1 = 1                                                           # (sample 1 walks 59 steps backwards)
        vis_p = oracle.euler_integration(-c["motion"][b1:b1 + 1], steps_p[b1])[1][0, 0]
        yy, xx = [int(v[0]) for v in np.nonzero(vis_p == 1)]
        gp[b1, 0, yy, xx] = np.inf
        onehot[:] = 0
        onehot[0, 0, yy, xx] = 1.0
        path_p = np.zeros(shape, bool)
        path_p[b1] = oracle.euler_backward(-c["motion"][b1:b1 + 1], steps_p[b1], onehot)[0] != 0
        g2 = host(pair_backward(S, *args, dev(gf), dev(gp))[0])
        assert (g2[path_p] == -np.inf).all() and np.array_equal(~np.isfinite(g2), mask | path_p)


def test_autograd_gives_the_entry_points_bits_and_launches_nothing_without_a_gradient(S, oracle, monkeypatch):
    shape, steps_f, steps_p = SMALL[0]
    c = case(oracle, "smooth", shape, steps_f, steps_p)
    sf, sp = steps_dev(steps_f), steps_dev(steps_p)
    want, _ = pair_backward(S, dev(c["motion"]), sf, sp, dev(c["gf"]), dev(c["gp"]))
    calls = []
    real = S.euler_integration_manipulator.call
    monkeypatch.setattr(S.euler_integration_manipulator, "call", lambda name, *a: calls.append(name) or real(name, *a))
    m = dev(c["motion"]).requires_grad_(True)
    flow_f, flow_p = S.euler_integration_pair(m, sf, sp)
    assert flow_f.grad_fn is flow_p.grad_fn and flow_f.requires_grad
    grad, = torch.autograd.grad([flow_f, flow_p], [m], [dev(c["gf"]), dev(c["gp"])])
    assert calls == ["slr_euler_pair_forward", "slr_euler_pair_backward"]
    assert torch.equal(grad.view(torch.int32), want.view(torch.int32))
    # one direction unused: its gradient is zero, not missing
    m2 = dev(c["motion"]).requires_grad_(True)
    only_f, = torch.autograd.grad([S.euler_integration_pair(m2, sf, sp)[0]], [m2], [dev(c["gf"])])
    want_f, _ = pair_backward(S, dev(c["motion"]), sf, sp, dev(c["gf"]), torch.zeros_like(m2))
    assert torch.equal(only_f, want_f)
    # no gradient asked for: the forward launch and nothing else, with and without grad mode
    calls.clear()
    plain = S.euler_integration_pair(dev(c["motion"]), list(steps_f), list(steps_p))
    with torch.no_grad():
        quiet = S.euler_integration_pair(m, sf, sp)
    assert calls == ["slr_euler_pair_forward"] * 2
    assert not plain[0].requires_grad and plain[0].grad_fn is None and quiet[0].grad_fn is None
    assert torch.equal(plain[0], flow_f) and torch.equal(quiet[1], flow_p)


def test_training_synthesis_with_the_pair_has_the_defaults_output_bits(S):
    """TrainingSynthesis(euler_pair=True): the output of the default module; the gradient w.r.t. the motion field within the summation
    order of the default's float atomics (checked against float64 above), and the same bits on a second run."""
    rng = np.random.default_rng(77)
    N, C, H, W = 2, 8, 20, 24
    fs, fe = dev(rng.standard_normal((N, C, H, W))), dev(rng.standard_normal((N, C, H, W)))
    mo = motion_of("smooth", (N, 2, H, W), 5)
    go = dev(rng.standard_normal((N, C, H, W)))
    start, mid, end = (torch.tensor(v).cuda() for v in ([0.0, 3.0], [30.0, 4.0], [59.0, 62.0]))
    grads = []
    for pair in (False, True, True):
        m = dev(mo).requires_grad_(True)
        out = S.TrainingSynthesis({"train_Z": False}, deterministic=True, euler_pair=pair)(fs, None, fe, None, m, start, mid, end)
        g, = torch.autograd.grad(out, m, go)
        grads.append((out, g))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[1][0], grads[2][0])
    assert torch.equal(grads[1][1].view(torch.int32), grads[2][1].view(torch.int32))
    scale = float(grads[0][1].abs().max())
    dev_ = float((grads[0][1] - grads[1][1]).abs().max())
    print(f"TrainingSynthesis d/dmotion: pair against the two atomic backwards: max|dev| {dev_:.3e} of max|g| {scale:.3e}")
    assert scale > 0 and dev_ <= 1e-4 * scale


def test_both_infinities_in_one_cell_make_a_nan(S, oracle):
    """Zero motion: a pixel gathers from its own cell in both directions, so +Inf in both displacement gradients meets as +Inf and -Inf."""
    shape, steps_f, steps_p = SMALL[0]
    c = case(oracle, "zero", shape, steps_f, steps_p)
    b, spots = 1, ((3, 5), (4, 6), (5, 7))                               # (sample 1 takes steps in both directions)
    assert steps_f[b] > 0 and steps_p[b] > 0
    gf, gp = c["gf"].copy(), c["gp"].copy()
    for y, x in spots:
        gf[b, 0, y, x] = gp[b, 0, y, x] = 0.5
    args = (dev(c["motion"]), steps_dev(steps_f), steps_dev(steps_p))
    clean, info = pair_backward(S, *args, dev(gf), dev(gp))
    gf[b, 0, 3, 5] = gp[b, 0, 3, 5] = gf[b, 0, 4, 6] = gp[b, 0, 5, 7] = np.inf
    got, info_p = pair_backward(S, *args, dev(gf), dev(gp))
    g, cl = host(got), host(clean)
    assert info_p == info
    assert g[b, 0, 3, 5].view(np.uint32) == 0x7FC00000 and g[b, 0, 4, 6] == np.inf and g[b, 0, 5, 7] == -np.inf
    mask = np.zeros(shape, bool)
    for y, x in spots:
        mask[b, 0, y, x] = True
    assert np.array_equal(~np.isfinite(g), mask) and np.array_equal(g.view(np.int32)[~mask], cl.view(np.int32)[~mask])
