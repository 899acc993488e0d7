"""The trainable 3x3 convolutions on the device (slr_sfs_amd.trainable, csrc/conv_grad.hip) against the float64 definitions of
tests/conv_train_f64.py.

Criterion (tests/test_gpu_splat_blend.py, tests/test_gpu_losses.py): per tensor E = max|got - ref64| / max|ref64| and
E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the same written-out definition evaluated by torch in float32 on the CPU against float64,
computed in the test from the test's inputs and never from the kernels.  What is elementwise (Gr = G * r) must be BIT-equal to the
float32 expression; what is deterministic by construction (every result here) must have the same bits in two runs.  Every test prints
its figures (run with -s)."""
import functools

import pytest
import torch

import conv_train_f64 as C64
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda"
X_B8, G_B8 = 1, 2
# N, Cin, Cout, H, W: channel counts below, between and across the 64-channel tiles; grids below a chunk (2 x 32) and odd; N > 1
ABI_SHAPES = ((1, 8, 3, 5, 7), (2, 3, 32, 16, 16), (2, 40, 72, 33, 20), (2, 64, 64, 37, 51), (1, 128, 256, 16, 24), (1, 256, 128, 8, 8))
OP_SHAPES = ((2, 64, 64, 37, 51), (2, 40, 72, 33, 20))
_id = lambda s: "x".join(map(str, s))                                     # noqa: E731


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def bound(e_plain):
    return 10.0 * e_plain + 1e-6


def held(name, got, ref64, plain32):
    e_gpu, e_plain = C64.E(got, ref64), C64.E(plain32, ref64)
    print(f"{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    assert e_gpu <= bound(e_plain), (name, e_gpu, e_plain)
    return e_gpu


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded inputs of ``shape`` (float32, on the CPU) and the written-out definition in float64 and in float32, computed once and
    shared.  x and g are dense normal values: the border rows and columns are non-zero, which is where a wrong halo shows."""
    N, cin, cout, H, W = shape
    gen = torch.Generator().manual_seed(cin * 1000 + cout * 10 + H)
    r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    x, w, b, g = r(N, cin, H, W), r(cout, cin, 3, 3) / (3.0 * cin ** 0.5), r(cout), r(N, cout, H, W)
    g = g * (1.0 + torch.arange(W) / W)                                     # (an incoming gradient that is not constant in any direction)
    assert (x[:, :, 0] != 0).all() and (x[:, :, -1] != 0).all() and (x[..., 0] != 0).all() and (x[..., -1] != 0).all()
    mask = C64.holed_mask(N, H, W, seed=cin + H)
    xm = x * mask

    def plain(dt):
        a = lambda t: t.to(dt)                                             # noqa: E731
        return dict(out=C64.conv(a(x), a(w), a(b)), dx=C64.conv_dx(a(g), a(w)), dw=C64.conv_dw(a(x), a(g)), db=C64.conv_db(a(g)))

    def partial(dt):
        a = lambda t: t.to(dt)                                             # noqa: E731
        out, um = C64.pconv(a(xm), a(mask), a(w), a(b))
        dx, dw, db = C64.pconv_grads(a(xm), a(mask), a(w), a(g))
        return dict(out=out, um=um, dx=dx, dw=dw, db=db)
    return dict(x=x, w=w, b=b, g=g, mask=mask, xm=xm, p64=plain(torch.float64), p32=plain(torch.float32),
                q64=partial(torch.float64), q32=partial(torch.float32))


def _weight_grad(S, x, g, cout, layout, splits=0, bias=True):
    """slr_conv3x3_weight_grad through the C ABI on device tensors laid out as ``layout`` says; outputs start as NaN."""
    N, cin, H, W = x.shape
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV) if bias else None
    nbytes = int(S._lib.lib().slr_conv3x3_grad_ws_bytes(N, cin, cout, H, W, splits))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    S._lib.call("slr_conv3x3_weight_grad", x.device, x, g, dw, db, N, cin, cout, H, W, splits, layout, ws, nbytes)
    return dw.cpu(), None if db is None else db.cpu()


def _layouts(cin, cout):
    return [lay for lay in (0, X_B8, G_B8, X_B8 | G_B8) if not (lay & X_B8 and cin % 8) and not (lay & G_B8 and cout % 8)]


def _placed(t, blocked):
    return (to_blocked(t) if blocked else t).to(DEV)


# ------------------------------------------------------------------ 1. weight and bias gradient through the C ABI

@pytest.mark.parametrize("shape", ABI_SHAPES, ids=_id)
def test_weight_and_bias_gradient(S, shape):
    N, cin, cout, H, W = shape
    c = _case(shape)
    layouts = _layouts(cin, cout)
    assert 0 in layouts and (len(layouts) == 4 or cin % 8 or cout % 8)
    first = None
    for lay in layouts:
        dw, db = _weight_grad(S, _placed(c["x"], lay & X_B8), _placed(c["g"], lay & G_B8), cout, lay)
        held(f"dW layout {lay}", dw, c["p64"]["dw"], c["p32"]["dw"])
        held(f"db layout {lay}", db, c["p64"]["db"], c["p32"]["db"])
        if first is None:
            first = dw, db
        else:                                            # the layout changes where a value is read from, not the order of any sum
            assert torch.equal(dw, first[0]), lay
            if bool(lay & G_B8) == 0:
                assert torch.equal(db, first[1]), lay


# ------------------------------------------------------------------ 2. the split

@pytest.mark.parametrize("splits", [1, 3, 0], ids=["one", "three", "auto"])
def test_split_counts_are_accurate_and_deterministic(S, splits):
    """76 chunks at this shape: 3 slabs of 25 / 25 / 26 chunks; the library's own choice is one slab per chunk."""
    shape = (2, 64, 64, 37, 51)
    c = _case(shape)
    x, g = _placed(c["x"], True), _placed(c["g"], True)
    a = _weight_grad(S, x, g, 64, X_B8 | G_B8, splits)
    b = _weight_grad(S, x, g, 64, X_B8 | G_B8, splits)
    held(f"dW splits {splits}", a[0], c["p64"]["dw"], c["p32"]["dw"])
    held(f"db splits {splits}", a[1], c["p64"]["db"], c["p32"]["db"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    dw_only, none = _weight_grad(S, x, g, 64, X_B8 | G_B8, splits, bias=False)
    assert none is None and torch.equal(dw_only, a[0])


# ------------------------------------------------------------------ 3. the scale / bias pass

@pytest.mark.parametrize("blocked", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("nchw", [(2, 40, 33, 20), (1, 8, 5, 7), (2, 64, 37, 51)], ids=_id)
def test_scale_bias_pass(S, nchw, blocked):
    """33 x 20 = 660 pixels (a multiple of 4: the 16-byte NCHW path), 35 and 1887 (odd: the scalar path, more than one workgroup)."""
    N, C, H, W = nchw
    gen = torch.Generator().manual_seed(C + H)
    g = torch.randn(N, C, H, W, generator=gen)
    _, um, r = C64.partial_factors(C64.holed_mask(N, H, W, seed=C), 16)
    assert (um == 0).any() and (r == 0).any() and (r > 1).any()
    lay = G_B8 if blocked else 0
    gr = torch.full((N, C, H, W), float("nan"), device=DEV)
    db = torch.full((C,), float("nan"), device=DEV)
    nbytes = int(S._lib.lib().slr_conv3x3_grad_ws_bytes(N, 0, C, H, W, 0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    S._lib.call("slr_conv_grad_scale_bias", torch.device(DEV), _placed(g, blocked), r.to(DEV), um.to(DEV), gr, db, N, C, H, W, lay, ws, nbytes)
    got = from_blocked(gr.cpu()) if blocked else gr.cpu()
    assert torch.equal(got, g * r)
    held("db", db.cpu(), C64.conv_db((g * um).double()), C64.conv_db(g * um))
    # without um and r: the plain convolution's bias gradient; without db: gr alone, the same bits
    db2 = torch.full((C,), float("nan"), device=DEV)
    S._lib.call("slr_conv_grad_scale_bias", torch.device(DEV), _placed(g, blocked), None, None, None, db2, N, C, H, W, lay, ws, nbytes)
    held("db plain", db2.cpu(), C64.conv_db(g.double()), C64.conv_db(g))
    gr2 = torch.full((N, C, H, W), float("nan"), device=DEV)
    S._lib.call("slr_conv_grad_scale_bias", torch.device(DEV), _placed(g, blocked), r.to(DEV), None, gr2, None, N, C, H, W, lay, None, 0)
    assert torch.equal(gr2, gr)


# ------------------------------------------------------------------ 4. the operators end to end

class _no_sync:
    """Inside: anything that synchronises the host with the device raises (inputs are placed before, results fetched after)."""

    def __enter__(self):
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


def _run_conv(S, c, need=(True, True, True), b8=False):
    x, w, b = (_placed(c["x"], b8).requires_grad_(need[0]), c["w"].to(DEV).requires_grad_(need[1]), c["b"].to(DEV).requires_grad_(need[2]))
    g = _placed(c["g"], b8)
    with _no_sync():
        out = S.conv3x3(x, w, b, in_b8=b8, out_b8=b8)
        out.backward(g)
    un = (lambda t: from_blocked(t.cpu())) if b8 else (lambda t: t.cpu())
    return un(out.detach()), None if x.grad is None else un(x.grad), None if w.grad is None else w.grad.cpu(), \
        None if b.grad is None else b.grad.cpu()


@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=_id)
def test_conv3x3_operator(S, shape, b8):
    c = _case(shape)
    out, dx, dw, db = _run_conv(S, c, b8=b8)
    w_only = _run_conv(S, c, (False, True, False), b8)
    x_only = _run_conv(S, c, (True, False, False), b8)
    for name, got in (("out", out), ("dx", dx), ("dw", dw), ("db", db)):
        held(f"conv3x3 {name}", got, c["p64"][name], c["p32"][name])
    assert w_only[1] is None and w_only[3] is None and torch.equal(w_only[2], dw)
    assert x_only[2] is None and x_only[3] is None and torch.equal(x_only[1], dx)


def _run_pconv(S, c, need=(True, True, True)):
    xm, w, b = c["xm"].to(DEV).requires_grad_(need[0]), c["w"].to(DEV).requires_grad_(need[1]), c["b"].to(DEV).requires_grad_(need[2])
    mask, g = c["mask"].to(DEV), c["g"].to(DEV)
    with _no_sync():
        out, um = S.partial_conv3x3(xm, mask, w, b)
        out.backward(g)
    assert not um.requires_grad and mask.grad is None
    grad = lambda t: None if t.grad is None else t.grad.cpu()            # noqa: E731
    return out.detach().cpu(), um.cpu(), grad(xm), grad(w), grad(b)


@pytest.mark.parametrize("shape", OP_SHAPES, ids=_id)
def test_partial_conv3x3_operator(S, shape):
    c = _case(shape)
    assert (c["q64"]["um"] == 0).any()                   # whole-window holes
    out, um, dx, dw, db = _run_pconv(S, c)
    w_only = _run_pconv(S, c, (False, True, False))
    x_only = _run_pconv(S, c, (True, False, False))
    assert torch.equal(um, c["q32"]["um"])
    for name, got in (("out", out), ("dx", dx), ("dw", dw), ("db", db)):
        held(f"partial_conv3x3 {name}", got, c["q64"][name], c["q32"][name])
    assert w_only[2] is None and w_only[4] is None and torch.equal(w_only[3], dw)
    assert x_only[3] is None and x_only[4] is None and torch.equal(x_only[2], dx)


# ------------------------------------------------------------------ 5. modules

def test_module_sees_its_optimizer_step(S):
    """One SGD step by hand, then a second forward: the cached fragment buffers follow the weight's version, forward and backward."""
    shape = (2, 40, 72, 33, 20)
    c = _case(shape)
    m = S.TrainableConv3x3(40, 72).to(DEV)
    with torch.no_grad():
        m.weight.copy_(c["w"]), m.bias.copy_(c["b"])
    x, g = c["x"].to(DEV).requires_grad_(True), c["g"].to(DEV)
    y1 = m(x)
    y1.backward(g)
    held("module out", y1.detach().cpu(), c["p64"]["out"], c["p32"]["out"])
    held("module dw", m.weight.grad.cpu(), c["p64"]["dw"], c["p32"]["dw"])
    lr = 0.5
    with torch.no_grad():
        m.weight -= lr * m.weight.grad
        m.bias -= lr * m.bias.grad
    w2, b2 = m.weight.detach().cpu(), m.bias.detach().cpu()
    x.grad = None
    y2 = m(x)
    y2.backward(g)
    assert not torch.equal(y1, y2)
    held("module out after the step", y2.detach().cpu(), C64.conv(c["x"].double(), w2.double(), b2.double()), C64.conv(c["x"], w2, b2))
    held("module dx after the step", x.grad.cpu(), C64.conv_dx(c["g"].double(), w2.double()), C64.conv_dx(c["g"], w2))


def test_state_dict_round_trip_with_nets_conv(S):
    conv = S.nets.Conv(16, 24, 3)
    for cls in (S.TrainableConv3x3, S.TrainablePartialConv3x3):
        m = cls(16, 24)
        m.load_state_dict(conv.state_dict())
        assert torch.equal(m.weight, conv.weight) and torch.equal(m.bias, conv.bias) and m.weight.requires_grad and m.bias.requires_grad
        back = S.nets.Conv(16, 24, 3)
        back.load_state_dict(m.state_dict())
        assert torch.equal(back.weight, conv.weight) and torch.equal(back.bias, conv.bias) and not back.weight.requires_grad
    # the trainable partial convolution is nets.PartialConv's forward on the fp32 rung, bit for bit
    c = _case((2, 40, 72, 33, 20))
    m, ref = S.TrainablePartialConv3x3(40, 72).to(DEV), S.nets.PartialConv(40, 72, 3).to(DEV)
    with torch.no_grad():
        m.weight.copy_(c["w"]), m.bias.copy_(c["b"])
    ref.load_state_dict(m.state_dict())
    out, um = m(c["xm"].to(DEV), c["mask"].to(DEV))
    with torch.no_grad(), S.nets.fp32_kernels(winograd=False):
        rout, rum = ref(c["xm"].to(DEV), c["mask"].to(DEV))
    assert torch.equal(out, rout) and torch.equal(um, rum)


# ------------------------------------------------------------------ 6. bad inputs

def test_bad_inputs_raise_before_the_device_is_touched(S):
    z = lambda *s: torch.zeros(*s, device=DEV)                             # noqa: E731
    with _no_sync():
        with pytest.raises(NotImplementedError):
            S.conv3x3(torch.zeros(1, 8, 4, 4), z(8, 8, 3, 3), z(8))
        with pytest.raises(NotImplementedError):
            S.partial_conv3x3(z(1, 8, 4, 4), torch.zeros(1, 1, 4, 4), z(8, 8, 3, 3), z(8))
        with pytest.raises(TypeError):
            S.conv3x3(z(1, 8, 4, 4).double(), z(8, 8, 3, 3), z(8))
        with pytest.raises(TypeError):
            S.conv3x3(z(1, 8, 4, 4), z(8, 8, 3, 3).half(), None)
        with pytest.raises(TypeError):
            S.conv3x3(z(1, 8, 4, 4), [1.0], None)
        for x, w, b in ((z(8, 4, 4), z(8, 8, 3, 3), None), (z(1, 8, 4, 4), z(8, 4, 3, 3), None), (z(1, 8, 4, 4), z(8, 8, 1, 1), None),
                        (z(1, 8, 4, 4), z(8, 8, 3, 3), z(7)), (z(1, 8, 4, 4)[:, :, ::2], z(8, 8, 3, 3), None)):
            with pytest.raises(ValueError):
                S.conv3x3(x, w, b)
        with pytest.raises(ValueError, match="Cin % 8"):
            S.conv3x3(z(1, 12, 4, 4), z(8, 12, 3, 3), None, in_b8=True)
        with pytest.raises(ValueError, match="Cout % 8"):
            S.conv3x3(z(1, 8, 4, 4), z(12, 8, 3, 3), None, out_b8=True)
        with pytest.raises(ValueError, match="mask"):
            S.partial_conv3x3(z(1, 8, 4, 4), z(1, 8, 4, 4), z(8, 8, 3, 3), z(8))
        with pytest.raises(ValueError, match="bias"):
            S.partial_conv3x3(z(1, 8, 4, 4), z(1, 1, 4, 4), z(8, 8, 3, 3), None)
    L = S._lib.lib()
    P = 0x10000
    assert L.slr_conv3x3_weight_grad(P, P, P, None, 1, 12, 8, 4, 4, 0, X_B8, P, 1 << 20, None) == -1 and b"Cin % 8" in L.slr_last_error()
    assert L.slr_conv_grad_scale_bias(P, P, P, P, None, 1, 12, 4, 4, G_B8, None, 0, None) == -1 and b"C % 8" in L.slr_last_error()
