"""The trainable generator networks on the device (slr_sfs_amd.trainable, csrc/decoder_grad.hip) against the float64 definitions of
tests/decoder_train_f64.py: the batch-norm with the per-element mask (x != 0), the partial convolution of a count plane, the decoder's
first block, ResNet_Block, and the decoder and an encoder as wholes.

Criterion (tests/test_gpu_block_train.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the
same written-out definition evaluated by torch in float32 on the CPU, computed here from the test's inputs and never from the kernels.
The gradient to a convolution's bias is measured against the magnitude of its terms (block_train_f64.E_terms) where, and only where, a
batch-norm with batch statistics follows the convolution: that batch-norm removes a per-channel constant, so the gradient cancels to
rounding (behind manual_bn exactly to zero) and max|ref64| is no scale for it.  That is db_aa of every block, and in the wholes db_ab and
db_b of every block but the last; every other bias gradient holds the plain E.  What is elementwise must be BIT-equal to the float32 expression; everything is deterministic and must
have the same bits in two runs.  Gradients through a ReLU gate are compared on inputs whose float64 pre-activations keep 1e-4 from zero at
every kept element (zero elements are exempt: their gate is multiplied by k = 0); constructed on the CPU and asserted.  Every test prints
its figures (run with -s)."""
import functools

import pytest
import torch

import block_train_f64 as B64
import conv_train_f64 as C64
import decoder_train_f64 as D64
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (2, 8, 3, 2751): H W = 8253, where the reductions with eight items per thread need more than one workgroup per plane (2 in NCHW, 5
# channel-blocked), the plane ends in a one-pixel item and most threads of the last workgroup have no item -- over two images
BN_SHAPES = ((1, 8, 5, 7), (2, 24, 33, 20), (2, 64, 37, 51), (2, 130, 4, 4), (2, 8, 3, 2751))
PC_SHAPES = ((2, 16, 24, 13, 10), (2, 64, 64, 37, 51), (1, 8, 3, 5, 7))                # N, Cin, Cout, H, W
IN_BLOCKS = ((2, 16, 24, 13, 10, None), (2, 24, 24, 12, 10, None), (2, 16, 40, 12, 12, "Down"), (2, 40, 16, 6, 5, "Up"), (2, 16, 3, 8, 8, None))
RES_BLOCKS = ((2, 3, 16, 9, 10, None), (2, 16, 16, 8, 8, None), (2, 16, 24, 12, 12, "Down"), (2, 24, 16, 6, 5, "Up"), (2, 16, 9, 8, 8, None))
DEC_WIDTHS, ENC_WIDTHS = [16, 24, 24, 16, 16, 16, 8], [8, 8, 8, 16, 16, 16, 16]
UPDOWN = [None, "Down", "Down", None, "Up", "Up", None, None]
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


def _grad(t):
    return None if t.grad is None else t.grad.cpu()


# ------------------------------------------------------------------ 1. statistics, forward, backward of the per-element batch-norm

@functools.lru_cache(maxsize=None)
def _nz_case(shape, stored):
    """block_train_f64.bn_inputs times decoder_train_f64.keep_pattern (whole-pixel holes, 10 % single zeros, channel 0 zero everywhere,
    channel 1 zero in image 0), kept gates nudged 1e-4 from zero in float64; the definition in float64 and float32."""
    N, C, H, W = shape
    x, gain, bias, ga = B64.bn_inputs(N, C, H, W, seed=C * 10 + H)
    x = x * D64.keep_pattern(N, C, H, W, seed=C + W)
    gen = torch.Generator().manual_seed(C)
    st = (torch.randn(C, generator=gen), 0.3 + 2 * torch.rand(C, generator=gen)) if stored else None
    zero = x == 0
    x = D64.nudged_nz(x, gain, bias, stored=st)
    assert torch.equal(x == 0, zero) and D64.gate_margin_nz(x, gain, bias, stored=st) > 1e-4
    assert float(D64.bn_nz_stats(x.double())[1].min()) >= 0.0
    addend = torch.randn(N, C, H, W, generator=gen)

    def run(dt):
        a = lambda t: t.to(dt)                                             # noqa: E731
        s = None if st is None else (a(st[0]), a(st[1]))
        act, mean, var, msum = D64.bn_nz_train(a(x), a(gain), a(bias), stored=s)
        dx, dgain, dbias = D64.bn_nz_train_grads(a(x), a(gain), a(bias), a(ga), stored=s)
        return dict(a=act, mean=mean, var=var, msum=msum, dx=dx, dgain=dgain, dbias=dbias, dx_add=dx + a(addend))
    return dict(x=x, gain=gain, bias=bias, ga=ga, st=st, addend=addend, r64=run(torch.float64), r32=run(torch.float32))


@pytest.mark.parametrize("shape", BN_SHAPES, ids=_id)
def test_statistics_count_plane_and_forward(S, shape):
    N, C, H, W = shape
    c, cs = _nz_case(shape, False), _nz_case(shape, True)
    ms = c["r64"]["msum"]                                # empty pixels, nearly full ones and many counts in between
    assert float(ms.min()) == 0.0 and float(ms.max()) >= 0.75 * C and len(ms.unique()) >= 4
    nnz = (c["x"] != 0).sum((0, 2, 3)).double()
    first = None
    for b8 in _layouts(C):
        x, xs = _placed(c["x"], b8), _placed(cs["x"], b8)
        gain, bias, sgain, sbias = c["gain"].to(DEV), c["bias"].to(DEV), cs["gain"].to(DEV), cs["bias"].to(DEV)
        with _no_sync():
            a, mean, var, msum = S.bn_relu_nonzero_train(x, gain, bias, b8=b8)
            again = S.bn_relu_nonzero_train(x, gain, bias, b8=b8)
        assert all(torch.equal(p, q) for p, q in zip((a, mean, var, msum), again))
        assert not msum.requires_grad and torch.equal(msum.cpu(), c["r32"]["msum"]) and torch.equal(c["r32"]["msum"].double(), c["r64"]["msum"])
        a = _back(a, b8)
        for name, got in (("mean", mean), ("var", var), ("a", a)):
            held(f"{name} b8={b8}", got.cpu(), c["r64"][name], c["r32"][name])
        assert float(mean[0]) == 0.0 == float(var[0])    # channel 0 has no element: cnt = eps, sums 0
        first = a if first is None else first
        assert torch.equal(a, first)
        # the count through the C ABI: float32(float64(nnz) + eps), per channel
        m_, v_, cnt = (torch.full((C,), float("nan"), device=DEV) for _ in range(3))
        ws = torch.empty(int(S._lib.lib().slr_bn_nonzero_ws_bytes(N, C, H, W)), dtype=torch.uint8, device=DEV)
        S._lib.call("slr_bn_nonzero_stats", torch.device(DEV), x, 1e-5, m_, v_, cnt, N, C, H, W, int(b8), ws, ws.numel())
        assert torch.equal(cnt.cpu(), (nnz + float(torch.tensor(1e-5, dtype=torch.float32))).float()) and torch.equal(m_, mean) and torch.equal(v_, var)
        # stored statistics: bit-equal to the float32 expression with the library's tables
        m, v = cs["st"][0].to(DEV), cs["st"][1].to(DEV)
        scale, shift = torch.full((N, C), float("nan"), device=DEV), torch.full((N, C), float("nan"), device=DEV)
        S._lib.call("slr_bn_train_tables", torch.device(DEV), m, v, sgain, sbias, 1e-5, scale, shift, N, C)
        with _no_sync():
            a2, m2, v2, ms2 = S.bn_relu_nonzero_train(xs, sgain, sbias, mean=m, var=v, b8=b8)
        assert m2.data_ptr() == m.data_ptr() and v2.data_ptr() == v.data_ptr() and torch.equal(ms2.cpu(), cs["r32"]["msum"])
        expr = torch.relu(cs["x"] * scale.cpu()[:, :, None, None] - shift.cpu()[:, :, None, None]) * (cs["x"] != 0).float()
        assert torch.equal(_back(a2, b8), expr)


def _run_nz(S, c, b8, need=(True, True, True), addend=False):
    x = _placed(c["x"], b8).requires_grad_(need[0])
    gain, bias = c["gain"].to(DEV).requires_grad_(need[1]), c["bias"].to(DEV).requires_grad_(need[2])
    ga, add = _placed(c["ga"], b8), _placed(c["addend"], b8)
    st = {} if c["st"] is None else dict(mean=c["st"][0].to(DEV), var=c["st"][1].to(DEV))
    with _no_sync():
        out = S.bn_relu_nonzero_train(x, gain, bias, b8=b8, fork=addend, **st)
        assert not any(t.requires_grad for t in out[1:4])     # mean, var and msum carry no gradient, whatever the inputs do
        if addend:
            torch.autograd.backward([out[0], out[4]], [ga, add])
        else:
            out[0].backward(ga)
    return None if x.grad is None else _back(x.grad, b8), _grad(gain), _grad(bias)


@pytest.mark.parametrize("stored", [False, True], ids=["batch", "stored"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=_id)
def test_per_element_bn_backward(S, shape, stored):
    c = _nz_case(shape, stored)
    first = None
    for b8 in _layouts(shape[1]):
        dx, dgain, dbias = _run_nz(S, c, b8)
        again = _run_nz(S, c, b8)
        dx_add = _run_nz(S, c, b8, addend=True)[0]
        for name, got in (("dx", dx), ("dgain", dgain), ("dbias", dbias), ("dx_add", dx_add)):
            held(f"{name} b8={b8}", got, c["r64"][name], c["r32"][name])
        assert all(torch.equal(p, q) for p, q in zip((dx, dgain, dbias), again))
        if not stored:                                   # the statistics' gradient reaches the zero elements too
            assert float(dx[c["x"] == 0].abs().max()) > 0
        x_only, tables_only = _run_nz(S, c, b8, (True, False, False)), _run_nz(S, c, b8, (False, True, True))
        assert x_only[1] is None and x_only[2] is None and torch.equal(x_only[0], dx)
        assert tables_only[0] is None and torch.equal(tables_only[1], dgain) and torch.equal(tables_only[2], dbias)
        if first is None:
            first = dx
        elif stored:                                     # elementwise, no sum in it: the layouts give the same bits
            assert torch.equal(dx, first)


# ------------------------------------------------------------------ 2. the training epilogue and the partial convolution of a count plane

@functools.lru_cache(maxsize=None)
def _pc_case(shape):
    N, cin, cout, H, W = shape
    gen = torch.Generator().manual_seed(cin * 1000 + cout * 10 + H)
    r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    xm = torch.relu(B64.bn_inputs(N, cin, H, W, seed=cin + H)[0]) * D64.keep_pattern(N, cin, H, W, seed=cin + W)
    msum = D64.kept(xm).sum(1, keepdim=True)
    w, b, res, g = r(cout, cin, 3, 3) / (3.0 * cin ** 0.5), r(cout), r(N, cout, H, W), r(N, cout, H, W) * (1.0 + torch.arange(W) / W)

    def run(dt):
        a = lambda t: t.to(dt)                                             # noqa: E731
        out, um = D64.pconv_counts(a(xm), a(msum), a(w), a(b), a(res))
        dx, dw, db = D64.pconv_counts_grads(a(xm), a(msum), a(w), a(g))
        ratio, _, rr = D64.partial_factors_counts(a(msum), cin)
        return dict(out=out, um=um, dx=dx, dw=dw, db=db, dres=a(g), ratio=ratio, r=rr, raw=C64.conv(a(xm), a(w)))
    return dict(xm=xm, msum=msum, w=w, b=b, res=res, g=g, r64=run(torch.float64), r32=run(torch.float32))


@pytest.mark.parametrize("shape", PC_SHAPES, ids=_id)
def test_training_epilogue(S, shape):
    """out = (raw * ratio + bias) * um (+ residual) is the float32 expression, bit for bit, in both layouts, in place or not."""
    N, cin, cout, H, W = shape
    c = _pc_case(shape)
    raw, ratio, um = c["r32"]["raw"].contiguous(), c["r32"]["ratio"], c["r32"]["um"]      # (the einsums leave raw permuted in memory)
    assert (um == 0).any() and (ratio > 1).any()
    for b8 in _layouts(cout):
        for res in (None, c["res"]):
            expr = (raw * ratio + c["b"].view(1, -1, 1, 1)) * um
            expr = expr if res is None else expr + res
            rd, out = _placed(raw, b8), torch.full((N, cout, H, W), float("nan"), device=DEV)
            args = (ratio.to(DEV), um.to(DEV), c["b"].to(DEV), None if res is None else _placed(res, b8))
            S._lib.call("slr_pconv_train_epilogue", torch.device(DEV), rd, *args, out, N, cout, H, W, int(b8))
            assert torch.equal(_back(out, b8), expr)
            S._lib.call("slr_pconv_train_epilogue", torch.device(DEV), rd, *args, rd, N, cout, H, W, int(b8))
            assert torch.equal(_back(rd, b8), expr)


@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("shape", PC_SHAPES, ids=_id)
def test_partial_conv_of_a_count_plane(S, shape, b8):
    N, cin, cout, H, W = shape
    c = _pc_case(shape)
    ib8, ob8 = b8 and cin % 8 == 0, b8 and cout % 8 == 0
    r32, r64 = c["r32"], c["r64"]

    msum, g = c["msum"].to(DEV), _placed(c["g"], ob8)

    def run(need):
        xm, w, b = _placed(c["xm"], ib8).requires_grad_(need[0]), c["w"].to(DEV).requires_grad_(need[1]), c["b"].to(DEV).requires_grad_(need[2])
        res = _placed(c["res"], ob8).requires_grad_(need[3])
        with _no_sync():
            out, um = S.partial_conv3x3_counts(xm, msum, w, b, residual=res, in_b8=ib8, out_b8=ob8)
            out.backward(g)
        return (_back(out, ob8), um.cpu(), None if xm.grad is None else _back(xm.grad, ib8), _grad(w), _grad(b),
                None if res.grad is None else _back(res.grad, ob8))
    out, um, dx, dw, db, dres = run((True, True, True, True))
    with _no_sync():
        r, um2 = S.partial_conv_factors_counts(msum, cin)
    assert torch.equal(um, r32["um"]) and torch.equal(um2.cpu(), r32["um"]) and torch.equal(r32["um"].double(), r64["um"])
    assert torch.equal(r.cpu(), r32["r"]) and torch.equal(r32["r"], r32["ratio"])
    for name, got in (("out", out), ("dx", dx), ("dw", dw), ("db", db), ("dres", dres)):
        held(f"partial_conv3x3_counts {name}", got, r64[name], r32[name])
    again, w_only = run((True, True, True, True)), run((False, True, False, False))
    assert all(torch.equal(p, q) for p, q in zip((out, um, dx, dw, db, dres), again))
    assert w_only[2] is None and w_only[4] is None and w_only[5] is None and torch.equal(w_only[3], dw)


# ------------------------------------------------------------------ 3. the two blocks

def _tables(noise, lin, i, a):
    return 1.0 + a(noise[0]) @ a(lin[f"g{i}"]).t(), a(noise[1]) @ a(lin[f"b{i}"]).t()


def _block_params(gen, cin, cout, kind, plain):
    r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    p = dict(w_aa=r(cout, cin, 3, 3) / (3.0 * cin ** 0.5), b_aa=0.3 * r(cout), w_ab=r(cout, cout, 3, 3) / (3.0 * cout ** 0.5),
             b_ab=0.3 * r(cout), w_b=r(cout, cin, 1, 1) / cin ** 0.5 if (kind or cin != cout) else None)
    if plain:
        p["b_b"] = 0.3 * r(cout) if p["w_b"] is not None else None
    return p, dict(g1=0.1 * r(cin, 20), b1=0.2 * r(cin, 20), g2=0.1 * r(cout, 20), b2=0.2 * r(cout, 20))


def _cast(p, a):
    return {k: (None if v is None else a(v)) for k, v in p.items()}


def _gains_biases(noise, lin, a):
    gains = [1.0 + a(noise[0]) @ a(lin["g1"]).t(), 1.0 + a(noise[1]) @ a(lin["g2"]).t()]
    return gains, [a(noise[0]) @ a(lin["b1"]).t(), a(noise[1]) @ a(lin["b2"]).t()]


def _lin_grads(d, noise, a):
    for i in (1, 2):                                     # gain = 1 + noise W^T, bias = noise W^T: dW = d(table)^T noise
        d[f"dlin_g{i}"], d[f"dlin_b{i}"] = d[f"dgain{i}"].t() @ a(noise[i - 1]), d[f"dbias{i}"].t() @ a(noise[i - 1])
    return d


@functools.lru_cache(maxsize=None)
def _block_case(spec, plain):
    """Seeded inputs, weights and noise of a block -- the first seed at which every kept float64 pre-activation of both BNs stays 1e-4
    from zero -- and the written-out definition in float64 and float32.  plain: ResNet_Block, else the decoder's first block."""
    N, cin, cout, H, W, kind = spec
    for seed in range(200):
        gen = torch.Generator().manual_seed(seed * 7919 + cin * 100 + cout)
        r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
        x = B64.bn_inputs(N, cin, H, W, seed)[0]
        if not plain:                                    # (no all-zero channel: its rs = eps^-1/2 makes dgain a pure rounding product)
            x = x * D64.keep_pattern(N, cin, H, W, seed=cin + H, zero_channel=False)
        p, lin = _block_params(gen, cin, cout, kind, plain)
        noise = r(N, 20), r(N, 20)
        OH, OW = {None: (H, W), "Down": ((H - 1) // 2 + 1, (W - 1) // 2 + 1), "Up": (2 * H, 2 * W)}[kind]
        g = r(N, cout, OH, OW) * (1.0 + torch.arange(OW) / OW)
        fwd, bwd = (D64.res_block, D64.res_block_grads) if plain else (D64.input_block, D64.input_block_grads)

        def run(dt, p=p, stored=None):
            a = lambda t: None if t is None else t.to(dt)                 # noqa: E731
            gains, biases = _gains_biases(noise, lin, a)
            st = None if stored is None else tuple((a(m), a(v)) for m, v in stored)
            f = fwd(a(x), _cast(p, a), kind, gains, biases, stored=st)
            if stored is not None:
                return f
            f.update(_lin_grads(bwd(a(x), _cast(p, a), kind, gains, biases, a(g)), noise, a), gains=gains, biases=biases)
            return f
        r64 = run(torch.float64)
        if plain:
            margins = (B64.gate_margin(x, None, r64["gains"][0], r64["biases"][0]), B64.gate_margin(r64["o1"], None, r64["gains"][1], r64["biases"][1]))
        else:
            margins = (D64.gate_margin_nz(x, r64["gains"][0], r64["biases"][0]),
                       B64.gate_margin(r64["o1"], r64["um1"], r64["gains"][1], r64["biases"][1]))
        if min(margins) > 1e-4:
            return dict(x=x, p=p, noise=noise, lin=lin, g=g, kind=kind, r64=r64, r32=run(torch.float32), run=run, margins=margins)
    raise AssertionError("no seed keeps the gates away from zero")


def _fill(blk, p, lin):
    with torch.no_grad():
        blk.conv_aa.weight.copy_(p["w_aa"]), blk.conv_aa.bias.copy_(p["b_aa"]), blk.conv_ab.weight.copy_(p["w_ab"]), blk.conv_ab.bias.copy_(p["b_ab"])
        assert (blk.conv_b is None) == (p["w_b"] is None)
        if p["w_b"] is not None:
            blk.conv_b.weight.copy_(p["w_b"])
            if p.get("b_b") is not None:
                blk.conv_b.bias.copy_(p["b_b"])
        blk.bn1.gain.weight.copy_(lin["g1"]), blk.bn1.bias.weight.copy_(lin["b1"])
        blk.bn2.gain.weight.copy_(lin["g2"]), blk.bn2.bias.weight.copy_(lin["b2"])
    return blk


def _block_grads_of(blk):
    got = dict(dw_aa=blk.conv_aa.weight.grad, db_aa=blk.conv_aa.bias.grad, dw_ab=blk.conv_ab.weight.grad, db_ab=blk.conv_ab.bias.grad,
               dlin_g1=blk.bn1.gain.weight.grad, dlin_b1=blk.bn1.bias.weight.grad, dlin_g2=blk.bn2.gain.weight.grad,
               dlin_b2=blk.bn2.bias.weight.grad)
    if blk.conv_b is not None:
        got["dw_b"] = blk.conv_b.weight.grad
        if blk.conv_b.bias is not None:
            got["db_b"] = blk.conv_b.bias.grad
    return got


def _check_block(S, spec, b8_in, plain):
    N, cin, cout, H, W, kind = spec
    c = _block_case(spec, plain)
    assert min(c["margins"]) > 1e-4
    blk = _fill((S.TrainableResBlock if plain else S.TrainablePconvInputBlock)(cin, cout, kind).to(DEV).train(), c["p"], c["lin"])
    x = _placed(c["x"], b8_in).requires_grad_(True)
    noise = tuple(t.to(DEV) for t in c["noise"])
    want_b8 = cout % 8 == 0 if blk.conv_b is not None else b8_in
    g = _placed(c["g"], want_b8)
    with _no_sync():
        out = blk(x, b8_in, noise=noise)
        out[0].backward(g)
    y, b8_out = out[0], out[-1]
    r64, r32 = c["r64"], c["r32"]
    assert b8_out == want_b8
    if not plain:
        assert not out[1].requires_grad and torch.equal(out[1].cpu(), r32["um"]) and torch.equal(r32["um"].double(), r64["um"])
    held("y", _back(y, b8_out), r64["y"], r32["y"])
    held("dx", _back(x.grad, b8_in), r64["dx"], r32["dx"])
    for name, t in _block_grads_of(blk).items():
        held(name, t.cpu(), r64[name], r32[name], r64["db_aa_terms"] if name == "db_aa" else None)
    for i, bn in ((1, blk.bn1), (2, blk.bn2)):           # stored = 0.9 * (0 | 1) + 0.1 * batch
        held(f"stored_mean{i}", bn.stored_mean.cpu(), 0.1 * r64[f"mean{i}"], 0.1 * r32[f"mean{i}"])
        held(f"stored_var{i}", bn.stored_var.cpu(), 0.9 + 0.1 * r64[f"var{i}"], 0.9 + 0.1 * r32[f"var{i}"])
    stored = tuple((bn.stored_mean.cpu(), bn.stored_var.cpu()) for bn in (blk.bn1, blk.bn2))
    blk.eval()
    with _no_sync(), torch.no_grad():
        oute = blk(x.detach(), b8_in, noise=noise)
    e64, e32 = c["run"](torch.float64, stored=stored), c["run"](torch.float32, stored=stored)
    held("y eval", _back(oute[0], b8_out), e64["y"], e32["y"])
    if not plain:
        assert torch.equal(oute[1].cpu(), e32["um"])


@pytest.mark.parametrize("b8_in", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("spec", IN_BLOCKS, ids=_id)
def test_input_block(S, spec, b8_in):
    _check_block(S, spec, b8_in, plain=False)


@pytest.mark.parametrize("spec,b8_in", [(s, b) for s in RES_BLOCKS for b in _layouts(s[1])], ids=lambda v: _id(v) if isinstance(v, tuple) else ("b8" if v else "nchw"))
def test_res_block(S, spec, b8_in):
    _check_block(S, spec, b8_in, plain=True)


# ------------------------------------------------------------------ 4. the wholes

@functools.lru_cache(maxsize=None)
def _net_case(kind):
    """A narrow decoder / encoder with N = 2 and 8 x 8 inputs: the first seed at which all 16 BNs keep their kept gates 1e-4 from zero."""
    plain = kind == "encoder"
    ch = [3] + ENC_WIDTHS + [17] if plain else [8] + DEC_WIDTHS + [3]
    kinds = [None] * 8 if plain else UPDOWN
    N, H, W = 2, 8, 8
    for seed in range(200):
        gen = torch.Generator().manual_seed(seed * 104729 + len(ch) + plain)
        r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
        x = B64.bn_inputs(N, ch[0], H, W, seed)[0]
        if not plain:
            x = x * D64.keep_pattern(N, ch[0], H, W, seed=3, zero_channel=False)
        blocks = [_block_params(gen, ch[i], ch[i + 1], kinds[i], plain) for i in range(8)]
        noise = [(r(N, 20), r(N, 20)) for _ in range(8)]
        g = r(N, ch[-1], H, W) * (1.0 + torch.arange(W) / W)

        def run(dt, ps=None, stored=None):
            a = lambda t: None if t is None else t.to(dt)                 # noqa: E731
            ps_ = [_cast(b[0] if ps is None else ps[i], a) for i, b in enumerate(blocks)]
            tabs = [_gains_biases(noise[i], blocks[i][1], a) for i in range(8)]
            gains, biases = [t[0] for t in tabs], [t[1] for t in tabs]
            st = None if stored is None else [tuple((a(m), a(v)) for m, v in s) for s in stored]
            if stored is not None or ps is not None:
                return (D64.encoder if plain else D64.decoder)(a(x), ps_, kinds, gains, biases, stored=st)
            fs, ds = (D64.encoder_grads if plain else D64.decoder_grads)(a(x), ps_, kinds, gains, biases, a(g))
            return fs, [_lin_grads(d, noise[i], a) for i, d in enumerate(ds)], gains, biases
        fs, ds, gains, biases = run(torch.float64)
        margins = []
        for i, f in enumerate(fs):
            if plain:
                margins += [B64.gate_margin(f["x"], None, gains[i][0], biases[i][0]), B64.gate_margin(f["o1"], None, gains[i][1], biases[i][1])]
            else:
                margins += [D64.gate_margin_nz(f["x"], gains[i][0], biases[i][0]) if i == 0 else B64.gate_margin(f["x"], f["mask"], gains[i][0], biases[i][0]),
                            B64.gate_margin(f["o1"], f["um1"], gains[i][1], biases[i][1])]
        if min(margins) > 1e-4:
            return dict(x=x, blocks=blocks, noise=noise, g=g, ch=ch, r64=(fs, ds), r32=run(torch.float32)[:2], run=run, margins=margins, plain=plain)
    raise AssertionError("no seed keeps the gates away from zero")


def _net(S, c):
    ch = c["ch"]
    net = (S.TrainableEncoderWithZ(cin=3, feat=16, widths=ENC_WIDTHS) if c["plain"] else S.TrainableDecoderPconv2(cin=8, cout=3, widths=DEC_WIDTHS))
    assert [b.conv_aa.weight.shape[1] for b in net.blocks] == ch[:-1] and net.blocks[-1].conv_aa.weight.shape[0] == ch[-1]
    net = net.to(DEV).train()
    for blk, (p, lin) in zip(net.blocks, c["blocks"]):
        _fill(blk, p, lin)
    return net


def _net_out(c, out):
    return torch.cat(out, 1) if c["plain"] else out            # (features, Z) of the encoder are the channels of one tensor


@pytest.mark.parametrize("kind", ["decoder", "encoder"])
def test_whole_net_trains(S, kind):
    c = _net_case(kind)
    assert len(c["margins"]) == 16 and min(c["margins"]) > 1e-4
    net = _net(S, c)
    x = c["x"].to(DEV).requires_grad_(True)
    noise = [tuple(t.to(DEV) for t in nz) for nz in c["noise"]]
    g = c["g"].to(DEV)
    with _no_sync():
        y = _net_out(c, net(x, noise=noise))
        y.backward(g)
    (f64, d64), (f32, d32) = c["r64"], c["r32"]
    held("y", y.detach().cpu(), f64[-1]["y"], f32[-1]["y"])
    held("dx", x.grad.cpu(), d64[0]["dx"], d32[0]["dx"])
    for i, blk in enumerate(net.blocks):
        for name, t in _block_grads_of(blk).items():
            behind_bn = name == "db_aa" or (name in ("db_ab", "db_b") and i < len(net.blocks) - 1)      # a batch-statistics BN follows
            terms = d64[i]["db_ab_terms" if name == "db_b" else name + "_terms"] if behind_bn else None
            held(f"block {i} {name}", t.cpu(), d64[i][name], d32[i][name], terms)
    # one SGD step by hand is seen by the next forward (the cached weight buffers follow the weights' versions)
    with _no_sync(), torch.no_grad():
        for prm in net.parameters():
            if prm.dim() == 4 or prm.dim() == 1:
                prm -= 0.05 * prm.grad
        y2 = _net_out(c, net(x.detach(), noise=noise))
    assert not torch.equal(y2, y)
    ps = [dict(w_aa=b.conv_aa.weight, b_aa=b.conv_aa.bias, w_ab=b.conv_ab.weight, b_ab=b.conv_ab.bias, w_b=None if b.conv_b is None else b.conv_b.weight,
               b_b=None if b.conv_b is None else b.conv_b.bias) for b in net.blocks]
    ps = [{k: (None if v is None else v.detach().cpu()) for k, v in p.items()} for p in ps]
    held("y after the step", y2.cpu(), c["run"](torch.float64, ps=ps)[-1]["y"], c["run"](torch.float32, ps=ps)[-1]["y"])
    # eval mode with the stored statistics the two steps left
    stored = [tuple((bn.stored_mean.cpu(), bn.stored_var.cpu()) for bn in (b.bn1, b.bn2)) for b in net.blocks]
    net.eval()
    with _no_sync(), torch.no_grad():
        ye = _net_out(c, net(x.detach(), noise=noise))
    held("y eval", ye.cpu(), c["run"](torch.float64, ps=ps, stored=stored)[-1]["y"], c["run"](torch.float32, ps=ps, stored=stored)[-1]["y"])


def _reference_state_dict(net, prefix, plain, gen):
    """A synthetic state dict with the reference's key scheme for every tensor of ``net``."""
    sd = {}
    for i, blk in enumerate(net.blocks):
        b = f"{prefix}{'gblocks' if plain else 'eblocks'}.{i}."
        names = dict(bn1="ch_a.0", bn2="ch_a.3", conv_aa="ch_a.2", conv_ab="ch_a.5", conv_b="ch_b.0") if plain else \
            dict(bn1="bn_noise1", bn2="bn_noise2", conv_aa="conv_aa", conv_ab="conv_ab", conv_b="conv_b")
        for bn in ("bn1", "bn2"):
            m = getattr(blk, bn)
            stat = f"{b}{names[bn]}.{'bn' if plain else 'pbn'}."
            sd[stat + "stored_mean"], sd[stat + "stored_var"] = torch.randn(m.stored_mean.shape, generator=gen), torch.rand(m.stored_var.shape, generator=gen)
            sd[f"{b}{names[bn]}.gain.weight"], sd[f"{b}{names[bn]}.bias.weight"] = (torch.randn(m.gain.weight.shape, generator=gen) for _ in range(2))
        for cv in ("conv_aa", "conv_ab", "conv_b"):
            m = getattr(blk, cv)
            if m is not None:
                sd[f"{b}{names[cv]}.weight"] = torch.randn(m.weight.shape, generator=gen)
                if m.bias is not None:
                    sd[f"{b}{names[cv]}.bias"] = torch.randn(m.bias.shape, generator=gen)
    return sd


def test_nets_fill_from_a_reference_state_dict(S):
    gen = torch.Generator().manual_seed(1)
    for net, prefix, plain in ((S.TrainableDecoderPconv2(), "model.module.projector.", False), (S.TrainableEncoderWithZ(), "model.module.encoder.", True)):
        base = S.nets.EncoderWithZ() if plain else S.nets.DecoderPconv2()
        assert isinstance(net, type(base)) and set(base.state_dict()) <= set(net.state_dict())
        sd = _reference_state_dict(net, prefix, plain, gen)
        before = {k: v.clone() for k, v in net.state_dict().items()}
        S.nets.load_reference_state_dict(net, sd, prefix)
        after = net.state_dict()
        assert len(sd) == len(after) and all(not torch.equal(before[k], after[k]) for k in after)       # every tensor was filled
        i = 3 if plain else 4                            # (32 -> 64 / 256 -> 128 "Up": blocks with a skip convolution)
        blk = net.blocks[i]
        b = prefix + (f"gblocks.{i}." if plain else f"eblocks.{i}.")
        assert torch.equal(blk.bn2.gain.weight, sd[b + ("ch_a.3" if plain else "bn_noise2") + ".gain.weight"]) and blk.conv_ab.weight.requires_grad
        assert torch.equal(blk.conv_b.weight, sd[b + ("ch_b.0" if plain else "conv_b") + ".weight"])


def test_full_width_decoder_is_finite_and_deterministic(S):
    """The default widths at [1,64,16,16]: forward and backward stay finite and have the same bits in two runs (no accuracy claim)."""
    torch.manual_seed(0)
    net = S.TrainableDecoderPconv2().to(DEV).train()
    gen = torch.Generator().manual_seed(2)
    x0 = (torch.randn(1, 64, 16, 16, generator=gen) * D64.keep_pattern(1, 64, 16, 16, seed=1, zero_channel=False)).to(DEV)
    noise = [(torch.randn(1, 20, generator=gen).to(DEV), torch.randn(1, 20, generator=gen).to(DEV)) for _ in range(8)]
    g = torch.randn(1, 3, 16, 16, generator=gen).to(DEV)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        with _no_sync():
            y = net(x, noise=noise)
            y.backward(g)
        runs.append([y.detach(), x.grad] + [p.grad.clone() for p in net.parameters()])
    assert tuple(runs[0][0].shape) == (1, 3, 16, 16)
    assert all(bool(torch.isfinite(t).all()) for t in runs[0]) and all(torch.equal(p, q) for p, q in zip(*runs))


# ------------------------------------------------------------------ 5. bad inputs

def test_bad_inputs_raise_before_the_device_is_touched(S):
    z = lambda *s: torch.zeros(*s, device=DEV)                             # noqa: E731
    inp, res, old = S.TrainablePconvInputBlock(8, 8).to(DEV), S.TrainableResBlock(8, 8).to(DEV), S.TrainablePconvResBlock(8, 8).to(DEV)
    with _no_sync():
        with pytest.raises(NotImplementedError):
            S.bn_relu_nonzero_train(torch.zeros(1, 8, 4, 4), None, None)
        with pytest.raises(NotImplementedError):
            S.partial_conv3x3_counts(torch.zeros(1, 8, 4, 4), z(1, 1, 4, 4), z(8, 8, 3, 3), z(8))
        with pytest.raises(NotImplementedError):
            inp(torch.zeros(1, 8, 4, 4))
        with pytest.raises(NotImplementedError):
            res(torch.zeros(1, 8, 4, 4))
        with pytest.raises(TypeError):
            S.bn_relu_nonzero_train(z(1, 8, 4, 4).double(), None, None)
        with pytest.raises(TypeError):
            S.partial_conv3x3_counts(z(1, 8, 4, 4), z(1, 1, 4, 4).half(), z(8, 8, 3, 3), z(8))
        with pytest.raises(TypeError):
            res(z(1, 8, 4, 4).half())
        with pytest.raises(ValueError, match="contiguous"):
            S.bn_relu_nonzero_train(z(1, 8, 4, 8)[..., ::2], None, None)
        with pytest.raises(ValueError, match="contiguous"):
            inp(z(1, 8, 4, 8)[..., ::2])
        with pytest.raises(ValueError, match="C % 8"):
            S.bn_relu_nonzero_train(z(1, 12, 4, 4), None, None, b8=True)
        with pytest.raises(ValueError, match="C % 8"):
            res(z(1, 12, 4, 4), True)
        with pytest.raises(ValueError, match="Cin % 8"):
            S.partial_conv3x3_counts(z(1, 12, 4, 4), z(1, 1, 4, 4), z(8, 12, 3, 3), z(8), in_b8=True)
        with pytest.raises(ValueError, match="gain / bias"):
            S.bn_relu_nonzero_train(z(1, 8, 4, 4), z(8), None)
        with pytest.raises(ValueError, match="mean and var"):
            S.bn_relu_nonzero_train(z(1, 8, 4, 4), None, None, mean=z(8))
        with pytest.raises(ValueError, match="mask"):
            S.partial_conv3x3_counts(z(1, 8, 4, 4), z(1, 8, 4, 4), z(8, 8, 3, 3), z(8))
        with pytest.raises(ValueError, match="bias"):
            S.partial_conv3x3_counts(z(1, 8, 4, 4), z(1, 1, 4, 4), z(8, 8, 3, 3), None)
        with pytest.raises(ValueError, match="residual"):
            S.conv3x3(z(1, 8, 4, 4), z(8, 8, 3, 3), residual=z(1, 8, 4, 5))
        with pytest.raises(ValueError, match="msum"):
            S.partial_conv_factors_counts(z(1, 8, 4, 4), 8)
        with pytest.raises(ValueError, match="noise"):
            S.TrainableEncoder(widths=[8] * 7)(z(1, 3, 8, 8), noise=[None])
        with pytest.raises(ValueError, match="resampling"):
            S.TrainableDecoderPconv2(widths=[8, 8])
        with pytest.raises(ValueError, match="updown"):
            S.TrainableBGDecoder(widths=[8], updown=[True, None])
        with pytest.raises(ValueError, match="multiple of 8"):
            S.TrainableEncoder(cout=8, widths=[8])
        with pytest.raises(NotImplementedError):
            S.partial_conv_factors_counts(torch.zeros(1, 1, 4, 4), 8)
        with pytest.raises(TypeError):
            S.partial_conv_factors_counts(z(1, 1, 4, 4).double(), 8)
        with pytest.raises(ValueError, match="contiguous"):
            S.partial_conv_factors_counts(z(1, 1, 4, 8)[..., ::2], 8)
        with pytest.raises(ValueError, match="mask"):
            old(z(1, 8, 4, 4), None)
