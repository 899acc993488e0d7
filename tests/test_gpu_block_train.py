"""The trainable decoder block on the device (slr_sfs_amd.trainable, csrc/block_grad.hip) against the float64 definitions of
tests/block_train_f64.py.

Criterion (tests/test_gpu_conv_train.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the
same written-out definition evaluated by torch in float32 on the CPU against float64, computed in the test from the test's inputs and
never from the kernels.  One tensor is measured against the magnitude of its terms instead of max|ref64| (block_train_f64.E_terms): the
gradient to conv_aa's bias with batch statistics, which cancels to ~1e-6 of its terms by construction.  What is elementwise must be
BIT-equal to the float32 expression; everything here is deterministic by construction and must have the same bits in two runs and in
both layouts.  Gradients through a ReLU gate are compared on inputs where no float64 pre-activation lies within 1e-4 of zero
(constructed on the CPU and asserted).  Every test prints its figures (run with -s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import block_train_f64 as B64
import conv_train_f64 as C64
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda"
X_B8, G_B8 = 1, 2
# (2, 8, 3, 2751): H W = 8253, where the reductions with eight items per thread need more than one workgroup per plane (2 in NCHW, 5
# channel-blocked), the plane ends in a one-pixel item and most threads of the last workgroup have no item -- over two images
BN_SHAPES = ((1, 8, 5, 7), (2, 24, 33, 20), (2, 64, 37, 51), (2, 130, 4, 4), (2, 8, 3, 2751))
W1_SHAPES = ((1, 8, 3, 5, 7), (2, 3, 32, 16, 16), (2, 40, 72, 33, 20), (2, 64, 64, 37, 51), (1, 128, 256, 16, 24))     # N, Cin, Cout, H, W
_id = lambda s: "x".join(map(str, s))                                     # noqa: E731


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def bound(e_plain):
    return 10.0 * e_plain + 1e-6


def held(name, got, ref64, plain32, terms=None):
    err = C64.E if terms is None else (lambda a, b: B64.E_terms(a, b, terms))
    e_gpu, e_plain = err(got, ref64), err(plain32, ref64)
    print(f"{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    assert e_gpu <= bound(e_plain), (name, e_gpu, e_plain)
    return e_gpu


class _no_sync:
    """Inside: anything that synchronises the host with the device raises (inputs are placed before, results fetched after)."""

    def __enter__(self):
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


def _placed(t, blocked):
    return (to_blocked(t) if blocked else t).to(DEV)


def _back(t, blocked):
    t = t.detach().cpu()
    return from_blocked(t) if blocked else t


def _layouts(C):
    return (False, True) if C % 8 == 0 else (False,)


# ------------------------------------------------------------------ 1. statistics, forward, backward of the batch-norm

@functools.lru_cache(maxsize=None)
def _bn_case(shape, masked, stored):
    """Seeded inputs (float32, CPU) with gates at least 1e-4 from zero in float64, and the written-out definition in float64 and float32."""
    N, C, H, W = shape
    mask = C64.holed_mask(N, H, W, seed=C + W) if masked else None
    x, gain, bias, ga = B64.bn_inputs(N, C, H, W, seed=C * 10 + H, mask=mask)
    gen = torch.Generator().manual_seed(C)
    st = (torch.randn(C, generator=gen), 0.3 + 2 * torch.rand(C, generator=gen)) if stored else None
    x = B64.nudged(x, mask, gain, bias, stored=st)
    assert B64.gate_margin(x, mask, gain, bias, stored=st) > 1e-4
    addend = torch.randn(N, C, H, W, generator=gen)

    def run(dt):
        a = lambda t: None if t is None else t.to(dt)                     # noqa: E731
        s = None if st is None else (a(st[0]), a(st[1]))
        act, mean, var = B64.bn_train(a(x), a(mask), a(gain), a(bias), stored=s)
        scale, shift = B64.bn_tables(mean, var, a(gain), a(bias))
        dx, dgain, dbias = B64.bn_train_grads(a(x), a(mask), a(gain), a(bias), a(ga), stored=s)
        return dict(a=act, mean=mean, var=var, scale=scale, shift=shift, dx=dx, dgain=dgain, dbias=dbias, dx_add=dx + a(addend))
    return dict(x=x, mask=mask, gain=gain, bias=bias, ga=ga, st=st, addend=addend, r64=run(torch.float64), r32=run(torch.float32))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=_id)
def test_statistics_and_forward(S, shape, masked):
    N, C, H, W = shape
    c, cs = _bn_case(shape, masked, False), _bn_case(shape, masked, True)
    mask = None if c["mask"] is None else c["mask"].to(DEV)
    first = None
    for b8 in _layouts(C):
        x, xs, gain, bias, sgain, sbias = (_placed(c["x"], b8), _placed(cs["x"], b8), c["gain"].to(DEV), c["bias"].to(DEV),
                                           cs["gain"].to(DEV), cs["bias"].to(DEV))
        with _no_sync():
            a, mean, var = S.bn_relu_mask_train(x, mask, gain, bias, b8=b8)
        a = _back(a, b8)
        for name, got in (("mean", mean), ("var", var), ("a", a)):
            held(f"{name} b8={b8}", got.cpu(), c["r64"][name], c["r32"][name])
        first = a if first is None else first
        assert torch.equal(a, first)                      # (mean and var: the layouts add their partial sums in different orders)
        # stored statistics: the tables from the library, then a bit-equal to the float32 expression
        m, v = cs["st"][0].to(DEV), cs["st"][1].to(DEV)
        scale, shift = torch.full((N, C), float("nan"), device=DEV), torch.full((N, C), float("nan"), device=DEV)
        S._lib.call("slr_bn_train_tables", torch.device(DEV), m, v, sgain, sbias, 1e-5, scale, shift, N, C)
        held("scale", scale.cpu(), cs["r64"]["scale"], cs["r32"]["scale"])
        held("shift", shift.cpu(), cs["r64"]["shift"], cs["r32"]["shift"])
        with _no_sync():
            a2, m2, v2 = S.bn_relu_mask_train(xs, mask, sgain, sbias, mean=m, var=v, b8=b8)
        assert m2.data_ptr() == m.data_ptr() and v2.data_ptr() == v.data_ptr()
        expr = torch.relu(cs["x"] * scale.cpu()[:, :, None, None] - shift.cpu()[:, :, None, None])
        assert torch.equal(_back(a2, b8), expr if cs["mask"] is None else expr * cs["mask"])


def _run_bn(S, c, b8, need=(True, True, True), addend=False):
    x = _placed(c["x"], b8).requires_grad_(need[0])
    gain, bias = c["gain"].to(DEV).requires_grad_(need[1]), c["bias"].to(DEV).requires_grad_(need[2])
    mask = None if c["mask"] is None else c["mask"].to(DEV)
    ga, add = _placed(c["ga"], b8), _placed(c["addend"], b8)
    st = {} if c["st"] is None else dict(mean=c["st"][0].to(DEV), var=c["st"][1].to(DEV))
    with _no_sync():
        out = S.bn_relu_mask_train(x, mask, gain, bias, b8=b8, fork=addend, **st)
        if addend:                                       # the block's fork: x comes back as a second output, its gradient is the addend
            torch.autograd.backward([out[0], out[3]], [ga, add])
        else:
            out[0].backward(ga)
    return (None if x.grad is None else _back(x.grad, b8), None if gain.grad is None else gain.grad.cpu(),
            None if bias.grad is None else bias.grad.cpu())


@pytest.mark.parametrize("stored", [False, True], ids=["batch", "stored"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=_id)
def test_bn_backward(S, shape, masked, stored):
    c = _bn_case(shape, masked, stored)
    first = None
    for b8 in _layouts(shape[1]):
        dx, dgain, dbias = _run_bn(S, c, b8)
        again = _run_bn(S, c, b8)
        dx_add = _run_bn(S, c, b8, addend=True)[0]
        for name, got in (("dx", dx), ("dgain", dgain), ("dbias", dbias), ("dx_add", dx_add)):
            held(f"{name} b8={b8}", got, c["r64"][name], c["r32"][name])
        assert all(torch.equal(p, q) for p, q in zip((dx, dgain, dbias), again))
        x_only, tables_only = _run_bn(S, c, b8, (True, False, False)), _run_bn(S, c, b8, (False, True, True))
        assert x_only[1] is None and x_only[2] is None and torch.equal(x_only[0], dx)
        assert tables_only[0] is None and torch.equal(tables_only[1], dgain) and torch.equal(tables_only[2], dbias)
        if first is None:
            first = dx
        elif stored:                                     # elementwise, no sum in it: the layouts give the same bits
            assert torch.equal(dx, first)


# ------------------------------------------------------------------ 2. the 1x1 convolution

@functools.lru_cache(maxsize=None)
def _w1_case(shape):
    N, cin, cout, H, W = shape
    gen = torch.Generator().manual_seed(cin * 1000 + cout * 10 + H)
    r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    x, w, b, g = r(N, cin, H, W), r(cout, cin, 1, 1) / cin ** 0.5, r(cout), r(N, cout, H, W) * (1.0 + torch.arange(W) / W)

    def run(dt):
        a = lambda t: t.to(dt)                                             # noqa: E731
        return dict(out=B64.conv1x1(a(x), a(w), a(b)), dx=B64.conv1x1_dx(a(g), a(w)), dw=B64.conv1x1_dw(a(x), a(g)), db=C64.conv_db(a(g)))
    return dict(x=x, w=w, b=b, g=g, r64=run(torch.float64), r32=run(torch.float32))


def _w1_grad(S, x, g, cout, layout, splits=0):
    N, cin, H, W = x.shape
    dw = torch.full((cout, cin, 1, 1), float("nan"), device=DEV)
    nbytes = int(S._lib.lib().slr_conv1x1_grad_ws_bytes(N, cin, cout, H, W, splits))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    S._lib.call("slr_conv1x1_weight_grad", x.device, x, g, dw, N, cin, cout, H, W, splits, layout, ws, nbytes)
    return dw.cpu()


@pytest.mark.parametrize("shape", W1_SHAPES, ids=_id)
def test_conv1x1_weight_gradient(S, shape):
    N, cin, cout, H, W = shape
    c = _w1_case(shape)
    layouts = [lay for lay in (0, X_B8, G_B8, X_B8 | G_B8) if not (lay & X_B8 and cin % 8) and not (lay & G_B8 and cout % 8)]
    first = None
    for lay in layouts:
        dw = _w1_grad(S, _placed(c["x"], lay & X_B8), _placed(c["g"], lay & G_B8), cout, lay)
        held(f"dW layout {lay}", dw, c["r64"]["dw"], c["r32"]["dw"])
        first = dw if first is None else first
        assert torch.equal(dw, first), lay                # the layout changes where a value is read from, not the order of any sum


@pytest.mark.parametrize("splits", [1, 3, 0], ids=["one", "three", "auto"])
def test_conv1x1_split_counts_are_accurate_and_deterministic(S, splits):
    """1887 pixels = 59 chunks per image, 118 in all: 3 slabs of 39 / 39 / 40 chunks; the library's own choice is one slab per chunk."""
    c = _w1_case((2, 64, 64, 37, 51))
    x, g = _placed(c["x"], True), _placed(c["g"], True)
    a, b = _w1_grad(S, x, g, 64, X_B8 | G_B8, splits), _w1_grad(S, x, g, 64, X_B8 | G_B8, splits)
    held(f"dW splits {splits}", a, c["r64"]["dw"], c["r32"]["dw"])
    assert torch.equal(a, b)


@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("shape", [(2, 40, 72, 33, 20), (2, 64, 64, 37, 51), (1, 8, 3, 5, 7)], ids=_id)
def test_conv1x1_operator(S, shape, b8):
    N, cin, cout, H, W = shape
    c = _w1_case(shape)
    ob8 = b8 and cout % 8 == 0

    def run(need):
        x, w, b = _placed(c["x"], b8).requires_grad_(need[0]), c["w"].to(DEV).requires_grad_(need[1]), c["b"].to(DEV).requires_grad_(need[2])
        g = _placed(c["g"], ob8)
        with _no_sync():
            out = S.conv1x1(x, w, b, in_b8=b8, out_b8=ob8)
            out.backward(g)
        grad = lambda t: None if t.grad is None else t.grad.cpu()          # noqa: E731
        return _back(out, ob8), None if x.grad is None else _back(x.grad, b8), grad(w), grad(b)
    out, dx, dw, db = run((True, True, True))
    for name, got in (("out", out), ("dx", dx), ("dw", dw), ("db", db)):
        held(f"conv1x1 {name}", got, c["r64"][name], c["r32"][name])
    w_only, x_only = run((False, True, False)), run((True, False, False))
    assert w_only[1] is None and w_only[3] is None and torch.equal(w_only[2], dw)
    assert x_only[2] is None and x_only[3] is None and torch.equal(x_only[1], dx)


# ------------------------------------------------------------------ 3. the adjoints of the resampling stages

@pytest.mark.parametrize("kind", ["Down", "Up"])
@pytest.mark.parametrize("hw", [(5, 7), (33, 20), (16, 24), (1, 1)], ids=_id)
def test_resampling_backward(S, hw, kind):
    H, W = hw
    N, C = 2, 8
    gen = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, C, H, W, generator=gen)
    fn = (lambda t: F.avg_pool2d(t, 3, stride=2, padding=1)) if kind == "Down" else \
        (lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False))
    op = S.avgpool_down if kind == "Down" else S.upsample_up
    g = torch.randn(fn(x).shape, generator=gen) * (1.0 + torch.arange(fn(x).shape[3]) / W)

    def autograd(dt):
        xa = x.to(dt).clone().requires_grad_(True)         # (a copy: x itself stays a plain tensor)
        out = fn(xa)
        return out.detach(), torch.autograd.grad(out, xa, g.to(dt))[0]
    (y64, d64), (y32, d32) = autograd(torch.float64), autograd(torch.float32)
    first = None
    for b8 in (False, True):
        xd, gd = _placed(x, b8).requires_grad_(True), _placed(g, b8)
        with _no_sync():
            y = op(xd, b8)
            y.backward(gd)
        y, gin = _back(y, b8), _back(xd.grad, b8)
        held(f"{kind} forward b8={b8}", y, y64, y32)
        e = held(f"{kind} backward b8={b8}", gin, d64, d32)
        # <A x, g> = <x, A^T g> in float64 on the host from the device's A x and A^T g, to the same bound (against |A x| |g|)
        lhs, rhs = (y.double() * g.double()).sum(), (x.double() * gin.double()).sum()
        rel = float((lhs - rhs).abs() / (y.double().norm() * g.double().norm()))
        print(f"{kind} adjoint identity b8={b8}: {rel:.3e} (backward E_gpu {e:.3e})")
        assert rel <= bound(C64.E(d32, d64))
        first = gin if first is None else first
        assert torch.equal(gin, first)                    # same order of every sum in both layouts


# ------------------------------------------------------------------ 4. the block

BLOCKS = ((2, 16, 24, 13, 10, None), (2, 24, 24, 12, 10, None), (2, 16, 40, 12, 12, "Down"), (2, 40, 16, 6, 5, "Up"), (2, 16, 3, 8, 8, None))


@functools.lru_cache(maxsize=None)
def _block_case(spec):
    """Seeded inputs, weights and noise of a block (float32, CPU) -- the first seed at which no float64 pre-activation of either BN lies
    within 1e-4 of zero -- and the written-out definition, forward and gradients, in float64 and float32."""
    N, cin, cout, H, W, kind = spec
    for seed in range(200):
        gen = torch.Generator().manual_seed(seed * 7919 + cin * 100 + cout)
        r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
        mask = C64.holed_mask(N, H, W, seed=cin + H)
        x = B64.bn_inputs(N, cin, H, W, seed, mask)[0]
        p = dict(w_aa=r(cout, cin, 3, 3) / (3.0 * cin ** 0.5), b_aa=0.3 * r(cout), w_ab=r(cout, cout, 3, 3) / (3.0 * cout ** 0.5),
                 b_ab=0.3 * r(cout), w_b=r(cout, cin, 1, 1) / cin ** 0.5 if (kind or cin != cout) else None)
        noise = r(N, 20), r(N, 20)
        lin = dict(g1=0.1 * r(cin, 20), b1=0.2 * r(cin, 20), g2=0.1 * r(cout, 20), b2=0.2 * r(cout, 20))
        OH, OW = {None: (H, W), "Down": ((H - 1) // 2 + 1, (W - 1) // 2 + 1), "Up": (2 * H, 2 * W)}[kind]
        g = r(N, cout, OH, OW) * (1.0 + torch.arange(OW) / OW)

        def run(dt, p=p, stored=None):
            a = lambda t: None if t is None else t.to(dt)                 # noqa: E731
            pp = {k: a(v) for k, v in p.items()}
            gains = [1.0 + a(noise[0]) @ a(lin["g1"]).t(), 1.0 + a(noise[1]) @ a(lin["g2"]).t()]
            biases = [a(noise[0]) @ a(lin["b1"]).t(), a(noise[1]) @ a(lin["b2"]).t()]
            st = None if stored is None else tuple((a(m), a(v)) for m, v in stored)
            f = B64.block(a(x), a(mask), pp, kind, gains, biases, stored=st)
            if stored is not None:
                return f
            d = B64.block_grads(a(x), a(mask), pp, kind, gains, biases, a(g))
            for i in (1, 2):                             # gain = 1 + noise W^T, bias = noise W^T: dW = d(table)^T noise
                d[f"dlin_g{i}"], d[f"dlin_b{i}"] = d[f"dgain{i}"].t() @ a(noise[i - 1]), d[f"dbias{i}"].t() @ a(noise[i - 1])
            f.update(d, gains=gains, biases=biases)
            return f
        r64 = run(torch.float64)
        margins = (B64.gate_margin(x, mask, r64["gains"][0], r64["biases"][0]),
                   B64.gate_margin(r64["o1"], r64["um1"], r64["gains"][1], r64["biases"][1]))
        if min(margins) > 1e-4:
            return dict(x=x, mask=mask, p=p, noise=noise, lin=lin, g=g, kind=kind, r64=r64, r32=run(torch.float32), run=run, margins=margins)
    raise AssertionError("no seed keeps the gates away from zero")


def _module(S, spec, c, p=None):
    N, cin, cout, H, W, kind = spec
    p = c["p"] if p is None else p
    blk = S.TrainablePconvResBlock(cin, cout, kind).to(DEV).train()
    with torch.no_grad():
        blk.conv_aa.weight.copy_(p["w_aa"]), blk.conv_aa.bias.copy_(p["b_aa"]), blk.conv_ab.weight.copy_(p["w_ab"]), blk.conv_ab.bias.copy_(p["b_ab"])
        if p["w_b"] is not None:
            blk.conv_b.weight.copy_(p["w_b"])
        blk.bn1.gain.weight.copy_(c["lin"]["g1"]), blk.bn1.bias.weight.copy_(c["lin"]["b1"])
        blk.bn2.gain.weight.copy_(c["lin"]["g2"]), blk.bn2.bias.weight.copy_(c["lin"]["b2"])
    assert (blk.conv_b is None) == (p["w_b"] is None)
    return blk


@pytest.mark.parametrize("b8_in", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("spec", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_block(S, spec, b8_in):
    N, cin, cout, H, W, kind = spec
    c = _block_case(spec)
    assert min(c["margins"]) > 1e-4
    blk = _module(S, spec, c)
    x = _placed(c["x"], b8_in).requires_grad_(True)
    mask, noise = c["mask"].to(DEV), tuple(t.to(DEV) for t in c["noise"])
    want_b8 = cout % 8 == 0 if blk.conv_b is not None else b8_in
    g = _placed(c["g"], want_b8)
    with _no_sync():
        y, um, b8_out = blk(x, mask, b8_in, noise=noise)
        y.backward(g)
    assert b8_out == want_b8 and not um.requires_grad
    r64, r32 = c["r64"], c["r32"]
    assert torch.equal(um.cpu(), r32["um"]) and torch.equal(r32["um"].double(), r64["um"])
    held("y", _back(y, b8_out), r64["y"], r32["y"])
    held("dx", _back(x.grad, b8_in), r64["dx"], r32["dx"])
    got = dict(dw_aa=blk.conv_aa.weight.grad, db_aa=blk.conv_aa.bias.grad, dw_ab=blk.conv_ab.weight.grad, db_ab=blk.conv_ab.bias.grad,
               dlin_g1=blk.bn1.gain.weight.grad, dlin_b1=blk.bn1.bias.weight.grad, dlin_g2=blk.bn2.gain.weight.grad,
               dlin_b2=blk.bn2.bias.weight.grad)
    if blk.conv_b is not None:
        got["dw_b"] = blk.conv_b.weight.grad
    for name, t in got.items():
        held(name, t.cpu(), r64[name], r32[name], r64["db_aa_terms"] if name == "db_aa" else None)
    for i, bn in ((1, blk.bn1), (2, blk.bn2)):           # stored = 0.9 * (0 | 1) + 0.1 * batch
        held(f"stored_mean{i}", bn.stored_mean.cpu(), 0.1 * r64[f"mean{i}"], 0.1 * r32[f"mean{i}"])
        held(f"stored_var{i}", bn.stored_var.cpu(), 0.9 + 0.1 * r64[f"var{i}"], 0.9 + 0.1 * r32[f"var{i}"])
    # eval mode: the stored statistics the step left, against the stored-statistics definition
    stored = tuple((bn.stored_mean.cpu(), bn.stored_var.cpu()) for bn in (blk.bn1, blk.bn2))
    blk.eval()
    with _no_sync(), torch.no_grad():
        ye, ume, _ = blk(x.detach(), mask, b8_in, noise=noise)
    e64, e32 = c["run"](torch.float64, stored=stored), c["run"](torch.float32, stored=stored)
    held("y eval", _back(ye, b8_out), e64["y"], e32["y"])
    assert torch.equal(ume.cpu(), e32["um"])


def test_block_sees_its_optimizer_step_and_draws_its_noise(S):
    """One SGD step by hand, then a second forward: the cached weight buffers of the three convolutions follow the weights' versions."""
    spec = (2, 16, 40, 12, 12, "Down")
    c = _block_case(spec)
    blk = _module(S, spec, c)
    x, mask, noise, g = _placed(c["x"], True), c["mask"].to(DEV), tuple(t.to(DEV) for t in c["noise"]), _placed(c["g"], True)
    with _no_sync():
        y1 = blk(x, mask, True, noise=noise)[0]
        y1.backward(g)
        with torch.no_grad():
            for prm in (blk.conv_aa.weight, blk.conv_ab.weight, blk.conv_b.weight, blk.conv_aa.bias):
                prm -= 0.5 * prm.grad
        y2 = blk(x, mask, True, noise=noise)[0]
        y3 = blk(x, mask, True)[0]                        # noise drawn by torch.randn on the device: still nothing synchronises
    assert not torch.equal(y1, y2) and y3.shape == y1.shape and bool(torch.isfinite(y3).all())
    p2 = dict(c["p"], w_aa=blk.conv_aa.weight.detach().cpu(), w_ab=blk.conv_ab.weight.detach().cpu(), w_b=blk.conv_b.weight.detach().cpu(),
              b_aa=blk.conv_aa.bias.detach().cpu())
    held("y after the step", _back(y2, True), c["run"](torch.float64, p=p2, stored=None)["y"], c["run"](torch.float32, p=p2, stored=None)["y"])


def test_block_fills_from_a_reference_state_dict(S):
    """Same sub-module names as nets.PconvResBlock: load_reference_state_dict's block branch fills it, the noise layers included."""
    blk = S.TrainablePconvResBlock(16, 24, "Down")
    assert isinstance(blk, S.nets.PconvResBlock) and set(S.nets.PconvResBlock(16, 24, "Down").state_dict()) <= set(blk.state_dict())
    gen = torch.Generator().manual_seed(1)
    b = "model.module.projector.eblocks.0."
    sd = {}
    for i, ch in ((1, 16), (2, 24)):
        sd.update({f"{b}bn_noise{i}.pbn.stored_mean": torch.randn(ch, generator=gen), f"{b}bn_noise{i}.pbn.stored_var": torch.rand(ch, generator=gen),
                   f"{b}bn_noise{i}.gain.weight": torch.randn(ch, 20, generator=gen), f"{b}bn_noise{i}.bias.weight": torch.randn(ch, 20, generator=gen)})
    for k, shp in (("conv_aa", (24, 16, 3, 3)), ("conv_ab", (24, 24, 3, 3)), ("conv_b", (24, 16, 1, 1))):
        sd[f"{b}{k}.weight"] = torch.randn(*shp, generator=gen)
        if k != "conv_b":
            sd[f"{b}{k}.bias"] = torch.randn(shp[0], generator=gen)
    net = torch.nn.Module()
    net.blocks = torch.nn.ModuleList([blk])
    S.nets.load_reference_state_dict(net, sd, "model.module.projector.")
    assert torch.equal(blk.bn2.gain.weight, sd[b + "bn_noise2.gain.weight"]) and torch.equal(blk.bn1.stored_var, sd[b + "bn_noise1.pbn.stored_var"])
    assert torch.equal(blk.conv_b.weight, sd[b + "conv_b.weight"]) and blk.conv_ab.weight.requires_grad


# ------------------------------------------------------------------ 5. bad inputs

def test_bad_inputs_raise_before_the_device_is_touched(S):
    z = lambda *s: torch.zeros(*s, device=DEV)                             # noqa: E731
    blk = S.TrainablePconvResBlock(8, 8).to(DEV)
    with _no_sync():
        with pytest.raises(NotImplementedError):
            S.bn_relu_mask_train(torch.zeros(1, 8, 4, 4), None, None, None)
        with pytest.raises(NotImplementedError):
            S.conv1x1(z(1, 8, 4, 4), torch.zeros(8, 8, 1, 1))
        with pytest.raises(NotImplementedError):
            S.avgpool_down(torch.zeros(1, 8, 4, 4))
        with pytest.raises(TypeError):
            S.bn_relu_mask_train(z(1, 8, 4, 4).double(), None, None, None)
        with pytest.raises(TypeError):
            S.bn_relu_mask_train(z(1, 8, 4, 4), None, z(1, 8).half(), None)
        with pytest.raises(TypeError):
            S.conv1x1(z(1, 8, 4, 4), z(8, 8, 1, 1).double())
        with pytest.raises(TypeError):
            S.upsample_up(z(1, 8, 4, 4).half())
        with pytest.raises(ValueError, match="contiguous"):
            S.bn_relu_mask_train(z(1, 8, 4, 8)[..., ::2], None, None, None)
        with pytest.raises(ValueError, match="contiguous"):
            S.conv1x1(z(1, 8, 4, 8)[..., ::2], z(8, 8, 1, 1))
        with pytest.raises(ValueError, match="contiguous"):
            S.avgpool_down(z(1, 8, 4, 8)[..., ::2])
        with pytest.raises(ValueError, match="C % 8"):
            S.bn_relu_mask_train(z(1, 12, 4, 4), None, None, None, b8=True)
        with pytest.raises(ValueError, match="C % 8"):
            S.upsample_up(z(1, 12, 4, 4), b8=True)
        with pytest.raises(ValueError, match="Cin % 8"):
            S.conv1x1(z(1, 12, 4, 4), z(8, 12, 1, 1), in_b8=True)
        with pytest.raises(ValueError, match="Cout % 8"):
            S.conv1x1(z(1, 8, 4, 4), z(12, 8, 1, 1), out_b8=True)
        with pytest.raises(ValueError, match="mask"):
            S.bn_relu_mask_train(z(1, 8, 4, 4), z(1, 8, 4, 4), None, None)
        with pytest.raises(ValueError, match="gain / bias"):
            S.bn_relu_mask_train(z(1, 8, 4, 4), None, z(8), None)
        with pytest.raises(ValueError, match="mean and var"):
            S.bn_relu_mask_train(z(1, 8, 4, 4), None, None, None, mean=z(8))
        with pytest.raises(ValueError, match="weight"):
            S.conv1x1(z(1, 8, 4, 4), z(8, 8, 3, 3))
        with pytest.raises(ValueError, match="mask"):
            blk(z(1, 8, 4, 4), z(1, 8, 4, 4))
        with pytest.raises(ValueError, match="mask"):
            blk(z(1, 8, 4, 4), None)
