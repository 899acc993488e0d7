"""Spectral normalisation of the generator on the device (slr_sfs_amd.spectral, csrc/spectral.hip, the scaled preparation of csrc/conv.hip)
against the float64 definition of tests/spectral_f64.py.

Criterion (tests/test_gpu_block_train.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the
same written-out definition evaluated by torch in float32 on the CPU from the test's inputs, never from the kernels.  Two kinds of result
are differences of large terms and are measured against the magnitude of their terms (block_train_f64.E_terms) instead:
  * the gradient to weight_orig, (dW - <dW, W_eff> u v^T) / sigma: terms = max(max|dW|, |<dW, W_eff>| max|u v^T|) / sigma -- where the
    rank-one term is as large as dW (test_rank_one_term_is_not_lost: dW = W_eff) the result is small against both;
  * the bias gradients behind a batch-statistics batch-norm, exactly as tests/test_gpu_decoder_train.py does.
What must be bit-equal says so.  Gradients through a ReLU gate are compared on inputs whose float64 pre-activations keep 1e-4 from zero
(seed search on the CPU, asserted).  Every test prints its figures (run with -s)."""
import functools

import pytest
import torch

import block_train_f64 as B64
import conv_train_f64 as C64
import decoder_train_f64 as D64
import spectral_f64 as S64
from metrics_fixture import from_blocked, to_blocked
from test_spectral_f64 import SIGMA_SHAPES

pytestmark = pytest.mark.gpu

DEV = "cuda"
DEC_WIDTHS, ENC_WIDTHS = [16, 24, 24, 16, 16, 16, 8], [8, 8, 8, 16, 16, 16, 16]
UPDOWN = [None, "Down", "Down", None, "Up", "Up", None, None]


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


def _at(value, k=0):
    """``value`` (CPU) on the device as a contiguous tensor whose first byte lies 4 k bytes past a 16-byte boundary (k = 0 .. 3)."""
    buf = torch.zeros(value.numel() + 8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[k:k + value.numel()].view(value.shape)
    t.copy_(value)
    assert t.data_ptr() % 16 == 4 * k and t.is_contiguous()
    return t


# ------------------------------------------------------------------ 1a. the sigma list

@functools.lru_cache(maxsize=None)
def _sigma_case(n, training):
    """n (W, u, v) triples cycling through SIGMA_SHAPES (float32 values), their float64 results and the float32 evaluation."""
    out = []
    for i in range(n):
        r, c = SIGMA_SHAPES[i % len(SIGMA_SHAPES)]
        W, u, v = S64.matrix_case(r, c, 100 + i)
        ref = S64.effective(W, u, v, training)[1:]
        plain = S64.effective(W.float(), u.float(), v.float(), training)[1:]
        out.append(dict(W=W.float(), u=u.float(), v=v.float(), ref=ref, plain=plain))
    return out


def _run_sigma(S, case, training, aligned=False):
    dev = [(_at(c["W"], 0 if aligned else (i + 1) % 4), _at(c["u"], 0 if aligned else (i + 2) % 4), _at(c["v"], 0 if aligned else (i + 3) % 4))
           for i, c in enumerate(case)]
    torch.cuda.synchronize()
    with _no_sync():
        inv, su, sv, offs = S.spectral_sigma([d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev], training=training)
    return dev, inv.cpu(), su.cpu(), sv.cpu(), offs


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("n", [1, 130])
def test_sigma_list(S, n, training):
    cases = [[c] for c in _sigma_case(len(SIGMA_SHAPES), training)] if n == 1 else [_sigma_case(n, training)]
    worst = 0.0
    for case in cases:
        dev, inv, su, sv, offs = _run_sigma(S, case, training)
        for i, (c, (W, u, v), (uo, vo)) in enumerate(zip(case, dev, offs)):
            r, cc = c["W"].shape
            (u64, v64, i64), (u32, v32, i32) = c["ref"], c["plain"]
            assert torch.equal(W.cpu(), c["W"])
            assert torch.equal(su[uo:uo + r], u.cpu()) and torch.equal(sv[vo:vo + cc], v.cpu())      # the saved copies are the buffers
            if training:
                quiet = n > 1 and i >= len(SIGMA_SHAPES)
                for name, got, r64, r32 in (("u", u.cpu(), u64, u32), ("v", v.cpu(), v64, v32), ("inv_sigma", inv[i:i + 1], i64.reshape(1), i32.reshape(1))):
                    e_gpu, e_plain = C64.E(got, r64), C64.E(r32, r64)
                    worst = max(worst, e_gpu / bound(e_plain))
                    if not quiet:
                        print(f"[{r},{cc}] n={n} {name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
                    assert e_gpu <= bound(e_plain), (i, name, e_gpu, e_plain)
            else:
                assert torch.equal(u.cpu(), c["u"]) and torch.equal(v.cpu(), c["v"])               # eval leaves u and v bit-identical
                held(f"[{r},{cc}] n={n} eval inv_sigma", inv[i:i + 1], i64.reshape(1), i32.reshape(1))
    print(f"n={n} training={training}: worst E_gpu / bound {worst:.3f}")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_sigma_list_bits(S, training):
    """The same bits in two runs, and the same bits for a tensor alone (16-byte aligned) and inside the 130-tensor list (misaligned)."""
    case = _sigma_case(130, training)
    a = _run_sigma(S, case, training)
    b = _run_sigma(S, case, training)
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    for i in range(len(SIGMA_SHAPES)):
        dev, inv, su, sv, _ = _run_sigma(S, [case[i]], training, aligned=True)
        uo, vo = a[4][i]
        r, c = case[i]["W"].shape
        assert torch.equal(inv, a[1][i:i + 1]), SIGMA_SHAPES[i]
        assert torch.equal(su, a[2][uo:uo + r]) and torch.equal(sv, a[3][vo:vo + c]), SIGMA_SHAPES[i]
        assert torch.equal(dev[0][1].cpu(), a[0][i][1].cpu()) and torch.equal(dev[0][2].cpu(), a[0][i][2].cpu())


# ------------------------------------------------------------------ 1b. the scaled preparation

PREP3, PREP1 = ((3, 8), (65, 64), (128, 64)), ((16, 8), (128, 64))


def _existing(S, w):
    """The existing entry's buffer of weight ``w`` (device), zero-filled first (the plain layout of <= 4 output channels writes a prefix)."""
    from slr_sfs_amd import _lib
    conv = "conv3x3" if w.shape[2] == 3 else "conv1x1"
    buf = torch.zeros(int(getattr(_lib.lib(), f"slr_{conv}_weight_bytes")(w.shape[0], w.shape[1])), dtype=torch.uint8, device=DEV)
    _lib.call(f"slr_{conv}_f32_weights", w.device, w, buf, w.shape[0], w.shape[1])
    return buf


def _written(k, co, ci, nbytes):
    return ((ci + 7) // 8 * 8) * 36 * 4 if (k == 3 and co <= 4) else nbytes


def _prep_inputs():
    gen = torch.Generator().manual_seed(11)
    ws = [torch.randn(co, ci, 3, 3, generator=gen) for co, ci in PREP3] + [torch.randn(co, ci, 1, 1, generator=gen) for co, ci in PREP1]
    scales = 0.25 + torch.rand(len(ws) + 2, generator=gen)
    return ws, scales


def test_scaled_preparation_has_the_bits_of_the_existing_entries(S):
    from slr_sfs_amd import _lib
    ws, scales = _prep_inputs()
    wd = [_at(w, i % 4) for i, w in enumerate(ws)]
    sd = scales.to(DEV)
    slots = [i + 1 for i in range(len(ws))]
    multi = S.prepare_scaled(wd, sd, slots)
    for w, d, slot, (mf, mb) in zip(ws, wd, slots, multi):
        co, ci, k = w.shape[0], w.shape[1], w.shape[2]
        conv = "conv3x3" if k == 3 else "conv1x1"
        prod = (w.to(DEV) * sd[slot]).contiguous()                               # weight * scale computed in fp32
        for backward, ref_w, (o, i_) in ((0, prod, (co, ci)), (1, prod.flip(2, 3).transpose(0, 1).contiguous(), (ci, co))):
            ref = _existing(S, ref_w)
            got = torch.zeros_like(ref)
            _lib.call(f"slr_{conv}_f32_weights_scaled", d.device, d, sd[slot:slot + 1], got, co, ci, backward)
            assert torch.equal(got, ref), (tuple(w.shape), backward)
            n = _written(k, o, i_, ref.numel())
            m = (mb if backward else mf)
            assert m.numel() >= ref.numel() and torch.equal(m[:n], ref[:n]), (tuple(w.shape), backward, "multi")
    print(f"{len(ws)} weights x (forward, backward): single and multi form bit-equal to the existing entries on weight * scale")


# ------------------------------------------------------------------ 1c. the gradient to weight_orig

def _grad_case(r, c, seed, dW=None):
    W, u, v = S64.matrix_case(r, c, seed)
    _, u, v, inv = S64.effective(W, u, v, True)
    u, v, inv = u.float().double(), v.float().double(), inv.float().double()              # what the device holds: float32 values
    gen = torch.Generator().manual_seed(seed + 1)
    dW = (torch.randn(r, c, generator=gen).double() if dW is None else dW(W, inv)).float().double()
    ref = S64.weight_orig_grad(dW, W, u, v, inv)
    plain = S64.weight_orig_grad(dW.float(), W.float(), u.float(), v.float(), inv.float())
    terms = max(S64.rank_one_term(dW, W, u, v, inv))
    return dict(W=W, u=u, v=v, inv=inv, dW=dW, ref=ref, plain=plain, terms=terms)


def _run_grad(S, c, k=0):
    args = [_at(c[n].float(), (k + j) % 4 if k else 0) for j, n in enumerate(("dW", "W", "u", "v"))]
    inv = c["inv"].float().reshape(1).to(DEV)
    torch.cuda.synchronize()
    with _no_sync():
        out = S.spectral_weight_grad(*args, inv)
    return out.cpu()


@pytest.mark.parametrize("shape", SIGMA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_orig_gradient(S, shape):
    c = _grad_case(*shape, seed=300 + shape[0])
    got = _run_grad(S, c, k=1)
    held(f"d weight_orig {shape} (against its terms)", got, c["ref"], c["plain"], c["terms"])
    held(f"d weight_orig {shape}", got, c["ref"], c["plain"])
    assert torch.equal(got, _run_grad(S, c, k=1)) and torch.equal(got, _run_grad(S, c, k=0))      # the same bits, wherever the tensors lie


def test_rank_one_term_is_not_lost(S):
    """dW = W_eff: <dW, W_eff> u v^T is as large as dW itself.  The kernel holds the bound against the terms; dropping the term misses
    it by orders of magnitude."""
    shape = (65, 576)
    c = _grad_case(*shape, seed=77, dW=lambda W, inv: W * inv)
    got = _run_grad(S, c)
    e = held("d weight_orig with dW = W_eff", got, c["ref"], c["plain"], c["terms"])
    dropped = (c["dW"] * c["inv"]).float()
    e_drop = B64.E_terms(dropped, c["ref"], c["terms"])
    b = bound(B64.E_terms(c["plain"], c["ref"], c["terms"]))
    print(f"without the rank-one term: E {e_drop:.3e} = {e_drop / b:.0f} x the bound {b:.3e} (with it: {e:.3e})")
    assert e_drop > 1000 * b


# ------------------------------------------------------------------ operators

def _op_case(k):
    gen = torch.Generator().manual_seed(500 + k)
    r = lambda *s: torch.randn(*s, generator=gen)                              # noqa: E731
    N, cin, cout, H, W = 2, 8, 16, 12, 12
    w = r(cout, cin, k, k) / (k * cin ** 0.5)
    u, v = (t.float() for t in S64.normal_uv(cout, cin * k * k, gen))
    mask = C64.holed_mask(N, H, W, seed=3)
    return dict(x=r(N, cin, H, W) * mask, w=w, b=0.3 * r(cout), u=u, v=v, mask=mask, g=r(N, cout, H, W))


def _op_ref(c, dt, op):
    a = lambda t: t.to(dt)                                                     # noqa: E731
    We, u, v, inv = S64.effective(a(c["w"]), a(c["u"]), a(c["v"]), True)
    x, b, g = a(c["x"]), a(c["b"]), a(c["g"])
    if op == "conv3x3":
        y, dx, dW, db = C64.conv(x, We, b), C64.conv_dx(g, We), C64.conv_dw(x, g), C64.conv_db(g)
    elif op == "conv1x1":
        y, dx, dW, db = B64.conv1x1(x, We, b), B64.conv1x1_dx(g, We), B64.conv1x1_dw(x, g), C64.conv_db(g)
    else:
        y = C64.pconv(x, a(c["mask"]), We, b)[0]
        dx, dW, db = C64.pconv_grads(x, a(c["mask"]), We, g)
    return dict(y=y, dx=dx, dw=S64.weight_orig_grad(dW, a(c["w"]), u, v, inv), db=db, u=u, v=v, inv=inv,
                terms=max(S64.rank_one_term(dW, a(c["w"]), u, v, inv)))


@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("op", ["conv3x3", "partial_conv3x3", "conv1x1"])
def test_operators_with_weight_scale_and_spectral(S, op, b8):
    c = _op_case(1 if op == "conv1x1" else 3)
    r64, r32 = _op_ref(c, torch.float64, op), _op_ref(c, torch.float32, op)
    put = (lambda t: to_blocked(t.to(DEV))) if b8 else (lambda t: t.to(DEV))
    back = (lambda t: from_blocked(t).cpu()) if b8 else (lambda t: t.cpu())
    x, w, b = put(c["x"]).requires_grad_(True), c["w"].to(DEV).requires_grad_(True), c["b"].to(DEV).requires_grad_(True)
    u, v = c["u"].to(DEV), c["v"].to(DEV)
    g, mask = put(c["g"]), c["mask"].to(DEV)
    torch.cuda.synchronize()
    with _no_sync():
        inv, su, sv, _ = S.spectral_sigma([w.detach()], [u], [v], training=True)
        kw = dict(in_b8=b8, out_b8=b8, weight_scale=inv, spectral=(su, sv))
        y = S.partial_conv3x3(x, mask, w, b, **kw)[0] if op == "partial_conv3x3" else getattr(S, op)(x, w, b, **kw)
        y.backward(g)
    held(f"{op} inv_sigma", inv.cpu(), r64["inv"].reshape(1), r32["inv"].reshape(1))
    held(f"{op} y", back(y.detach()), r64["y"], r32["y"])
    held(f"{op} dx", back(x.grad), r64["dx"], r32["dx"])
    held(f"{op} d weight_orig (against its terms)", w.grad.cpu(), r64["dw"], r32["dw"], r64["terms"])
    held(f"{op} db", b.grad.cpu(), r64["db"], r32["db"])
    # both None: exactly the operator without them -- the bits of the module-free call on the effective weight's own preparation
    with torch.no_grad():
        w_eff = (w * inv).contiguous()
        kw0 = dict(in_b8=b8, out_b8=b8)
        y0 = S.partial_conv3x3(x, mask, w_eff, b, **kw0)[0] if op == "partial_conv3x3" else getattr(S, op)(x, w_eff, b, **kw0)
    assert torch.equal(y0, y.detach())


def test_weight_scale_alone_is_a_constant_factor(S):
    """weight_scale without spectral: the convolution of weight * scale, and the weight gradient is dW * scale."""
    c = _op_case(3)
    scale = torch.tensor([0.37])

    def ref(dt):
        x, w, g, s = (t.to(dt) for t in (c["x"], c["w"], c["g"], scale))
        return C64.conv(x, w * s, c["b"].to(dt)), C64.conv_dw(x, g) * s, C64.conv_dx(g, w * s)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    x, w, b = c["x"].to(DEV).requires_grad_(True), c["w"].to(DEV).requires_grad_(True), c["b"].to(DEV)
    g, sd = c["g"].to(DEV), scale.to(DEV)
    torch.cuda.synchronize()
    with _no_sync():
        y = S.conv3x3(x, w, b, weight_scale=sd)
        y.backward(g)
    for name, got, k in (("y", y.detach(), 0), ("d weight", w.grad, 1), ("dx", x.grad, 2)):
        held(f"weight_scale alone: {name}", got.cpu(), r64[k], r32[k])


# ------------------------------------------------------------------ blocks

BLOCK_SPECS = (("pconv", 8, 16, 12, 12, None), ("pconv", 8, 16, 12, 12, "Down"), ("pconv", 16, 8, 6, 6, "Up"),
               ("res", 8, 16, 12, 12, None), ("res", 8, 16, 12, 12, "Down"), ("res", 16, 8, 6, 6, "Up"),
               ("input", 8, 16, 12, 12, None), ("input", 8, 16, 12, 12, "Down"), ("input", 16, 8, 6, 6, "Up"))


def _margins(form, f, x, mask, gains, biases):
    first = D64.gate_margin_nz(x, gains[0], biases[0]) if form == "input" else B64.gate_margin(x, mask, gains[0], biases[0])
    return [first, B64.gate_margin(f["o1"], f.get("um1"), gains[1], biases[1])]


def _f32(tree):
    return S64.cast(S64.cast(tree, torch.float32), torch.float64)


@functools.lru_cache(maxsize=None)
def _block_case(spec):
    """The golden's shapes: parameters, two inputs, noise and output gradients (float32 values) -- the first seed at which no float64
    pre-activation of either BN in either forward lies within 1e-4 of zero -- and the definition in float64 and float32: two forwards,
    then the gradients of the sum."""
    form, cin, cout, H, W, kind = spec
    N = 2
    for seed in range(300):
        p, uv = _f32(S64.block_params(form, cin, cout, True, 1000 * seed + cin + 3 * cout + len(form)))
        gen = torch.Generator().manual_seed(seed * 7919 + cin)
        r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
        OH, OW = {None: (H, W), "Down": ((H - 1) // 2 + 1, (W - 1) // 2 + 1), "Up": (2 * H, 2 * W)}[kind]
        fw = []
        for k in range(2):
            mask = C64.holed_mask(N, H, W, seed=cin + H + k) if form == "pconv" else None
            x = B64.bn_inputs(N, cin, H, W, seed + 17 * k, mask)[0]
            if form == "input":
                x = x * D64.keep_pattern(N, cin, H, W, seed=3 + k, zero_channel=False)
            fw.append(dict(x=x, mask=mask, noise=(r(N, 20), r(N, 20)), g=r(N, cout, OH, OW) * (1.0 + torch.arange(OW) / OW)))

        def run(dt):
            a = lambda t: S64.cast(t, dt)                                     # noqa: E731
            pp, u_ = a(p), a(uv)
            fs, ds, uvs, total, margins = [], [], [], None, []
            for k in range(2):
                x, mask, noise, g = a(fw[k]["x"]), a(fw[k]["mask"]), a(fw[k]["noise"]), a(fw[k]["g"])
                f, u_, ctx = S64.block(form, x, mask, pp, u_, kind, noise, True)
                d = S64.block_grads(form, x, mask, pp, u_, kind, noise, g, ctx)
                margins += _margins(form, f, x, mask, ctx[2], ctx[3])
                fs.append(f), ds.append(d), uvs.append(u_)
                one = {n: d["d_" + n] for n in S64.names_of(pp)}
                one.update({b: d["d" + b] for b in ("b_aa", "b_ab", "b_b") if pp.get(b) is not None})
                tr = {n: max(S64.rank_one_term(d["dW_" + n], pp[n], *u_[n], ctx[1][n])) for n in S64.names_of(pp)}
                tr.update(b_aa=d["db_aa_terms"].max())
                total = (one, tr) if total is None else ({n: total[0][n] + one[n] for n in one}, {n: total[1][n] + tr[n] for n in tr})
            return dict(fs=fs, ds=ds, uvs=uvs, grads=total[0], terms=total[1], margins=margins)
        r64 = run(torch.float64)
        if min(r64["margins"]) > 1e-4:
            return dict(p=p, uv=uv, fw=fw, kind=kind, r64=r64, r32=run(torch.float32))
    raise AssertionError("no seed keeps the gates away from zero")


LEAVES = (("w_aa", "conv_aa"), ("w_ab", "conv_ab"), ("w_b", "conv_b"), ("gain1", "bn1.gain"), ("bias1", "bn1.bias"), ("gain2", "bn2.gain"),
          ("bias2", "bn2.bias"))


def _leaf(blk, path):
    for part in path.split("."):
        blk = getattr(blk, part)
    return blk


def _fill(blk, p, uv):
    with torch.no_grad():
        for name, path in LEAVES:
            m = _leaf(blk, path)
            assert (m is None) == (p.get(name) is None), name
            if m is not None:
                m.weight_orig.copy_(p[name]), m.weight_u.copy_(uv[name][0]), m.weight_v.copy_(uv[name][1])
        blk.conv_aa.bias.copy_(p["b_aa"]), blk.conv_ab.bias.copy_(p["b_ab"])
        if p.get("b_b") is not None:
            blk.conv_b.bias.copy_(p["b_b"])
    return blk


def _block_module(S, spec):
    form, cin, cout, H, W, kind = spec
    cls = {"pconv": S.TrainablePconvResBlock, "input": S.TrainablePconvInputBlock, "res": S.TrainableResBlock}[form]
    return cls(cin, cout, kind, spectral=True).to(DEV).train()


def _check_grads(blk, r64, r32, label=""):
    got = {name: _leaf(blk, path).weight_orig.grad for name, path in LEAVES if _leaf(blk, path) is not None}
    got.update(b_aa=blk.conv_aa.bias.grad, b_ab=blk.conv_ab.bias.grad)
    if blk.conv_b is not None and blk.conv_b.bias is not None:
        got["b_b"] = blk.conv_b.bias.grad
    for name, t in got.items():
        held(f"{label}d {name}", t.cpu(), r64["grads"][name], r32["grads"][name], r64["terms"].get(name))


@pytest.mark.parametrize("spec", BLOCK_SPECS, ids=lambda s: "-".join(map(str, s)))
def test_block_two_forwards_then_backward(S, spec):
    form = spec[0]
    c = _block_case(spec)
    r64, r32 = c["r64"], c["r32"]
    assert min(r64["margins"]) > 1e-4
    blk = _fill(_block_module(S, spec), c["p"], c["uv"])
    xs = [f["x"].float().to(DEV).requires_grad_(True) for f in c["fw"]]
    noises = [tuple(t.float().to(DEV) for t in f["noise"]) for f in c["fw"]]
    masks = [None if f["mask"] is None else f["mask"].float().to(DEV) for f in c["fw"]]
    gs = [f["g"].float().to(DEV) for f in c["fw"]]
    ys, seen = [], []
    torch.cuda.synchronize()
    with _no_sync():
        for k in range(2):
            out = blk(xs[k], masks[k], noise=noises[k]) if form == "pconv" else blk(xs[k], noise=noises[k])
            ys.append(from_blocked(out[0]) if out[-1] else out[0])       # (out[-1]: the block's output is channel-blocked)
            seen.append({name: (_leaf(blk, path).weight_u.clone(), _leaf(blk, path).weight_v.clone()) for name, path in LEAVES
                         if _leaf(blk, path) is not None})
        sum((y * g).sum() for y, g in zip(ys, gs)).backward()
    for k in range(2):
        held(f"forward {k} y", ys[k].detach().cpu(), r64["fs"][k]["y"], r32["fs"][k]["y"])
        held(f"forward {k} dx", xs[k].grad.cpu(), r64["ds"][k]["dx"], r32["ds"][k]["dx"])
        for name, (u, v) in seen[k].items():
            held(f"forward {k} u {name}", u.cpu(), r64["uvs"][k][name][0], r32["uvs"][k][name][0])
            held(f"forward {k} v {name}", v.cpu(), r64["uvs"][k][name][1], r32["uvs"][k][name][1])
    _check_grads(blk, r64, r32)


# ------------------------------------------------------------------ whole networks

@functools.lru_cache(maxsize=None)
def _net_case(kind):
    """A narrow decoder / encoder (8 blocks, N = 2, 8 x 8 inputs) under spectral normalisation, one step: the first seed at which all 16
    BNs keep their gates 1e-4 from zero."""
    plain = kind == "encoder"
    ch = [3] + ENC_WIDTHS + [17] if plain else [8] + DEC_WIDTHS + [3]
    kinds = [None] * 8 if plain else UPDOWN
    forms = ["res"] * 8 if plain else ["input"] + ["pconv"] * 7
    N, H, W = 2, 8, 8
    for seed in range(300):
        gen = torch.Generator().manual_seed(seed * 104729 + plain)
        r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
        x = B64.bn_inputs(N, ch[0], H, W, seed)[0]
        if not plain:
            x = x * D64.keep_pattern(N, ch[0], H, W, seed=3, zero_channel=False)
        blocks = [_f32(S64.block_params(forms[i], ch[i], ch[i + 1], bool(kinds[i]) or ch[i] != ch[i + 1], 31 * seed + i)) for i in range(8)]
        noise = [(r(N, 20), r(N, 20)) for _ in range(8)]
        g = r(N, ch[-1], H, W) * (1.0 + torch.arange(W) / W)

        def run(dt, ps=None, uvs=None, training=True, stored=None, grads=True):
            a = lambda t: S64.cast(t, dt)                                     # noqa: E731
            ps_ = a([b[0] for b in blocks] if ps is None else ps)
            uvs_ = a([b[1] for b in blocks] if uvs is None else uvs)
            fs, uns, ctxs = S64.network(forms, a(x), ps_, uvs_, kinds, a(noise), training, a(stored))
            ds = S64.network_grads(forms, fs, ps_, uns, kinds, a(noise), a(g), ctxs) if grads else None
            return fs, uns, ctxs, ds
        fs, uns, ctxs, ds = run(torch.float64)
        margins = []
        for i, f in enumerate(fs):
            margins += _margins(forms[i], f, f["x"], f["mask"], ctxs[i][2], ctxs[i][3])
        if min(margins) > 1e-4:
            return dict(x=x, blocks=blocks, noise=noise, g=g, ch=ch, kinds=kinds, forms=forms, plain=plain, run=run, margins=margins,
                        r64=(fs, uns, ctxs, ds), r32=run(torch.float32))
    raise AssertionError("no seed keeps the gates away from zero")


def _net(S, c, spectral=True):
    net = (S.TrainableEncoderWithZ(cin=3, feat=16, widths=ENC_WIDTHS, spectral=spectral) if c["plain"]
           else S.TrainableDecoderPconv2(cin=8, cout=3, widths=DEC_WIDTHS, spectral=spectral))
    net = net.to(DEV).train()
    if spectral:
        for blk, (p, uv) in zip(net.blocks, c["blocks"]):
            _fill(blk, p, uv)
    return net


def _out(c, out):
    return torch.cat(out, 1) if c["plain"] else out


def _net_terms(c, r, i):
    fs, uns, ctxs, ds = r
    p = c["blocks"][i][0]
    t = {n: max(S64.rank_one_term(ds[i]["dW_" + n], S64.cast(p[n], ds[i]["dx"].dtype), *uns[i][n], ctxs[i][1][n])) for n in S64.names_of(p)}
    t["b_aa"] = ds[i]["db_aa_terms"].max()
    if i < 7:                                            # a batch-statistics BN follows: db_ab and db_b cancel, too
        if "db_ab_terms" in ds[i]:
            t["b_ab"] = t["b_b"] = ds[i]["db_ab_terms"].max()
    return t


@pytest.mark.parametrize("kind", ["decoder", "encoder"])
def test_whole_net_one_step(S, kind):
    c = _net_case(kind)
    assert len(c["margins"]) == 16 and min(c["margins"]) > 1e-4
    net = _net(S, c)
    x = c["x"].to(DEV).requires_grad_(True)
    noise = [tuple(t.to(DEV) for t in nz) for nz in c["noise"]]
    g = c["g"].to(DEV)
    torch.cuda.synchronize()
    with _no_sync():
        y = _out(c, net(x, noise=noise))
        y.backward(g)
    (f64, u64, c64, d64), (f32, u32, c32, d32) = c["r64"], c["r32"]
    held("y", y.detach().cpu(), f64[-1]["y"], f32[-1]["y"])
    held("dx", x.grad.cpu(), d64[0]["dx"], d32[0]["dx"])
    for i, blk in enumerate(net.blocks):
        if not c["plain"] and i > 0:                     # (the definition's pconv blocks lack these terms: as test_gpu_decoder_train)
            gs = B64.resample_adjoint(d64[i + 1]["dx"] if i < 7 else c["g"].double(), c["kinds"][i], f64[i]["x"].shape[2], f64[i]["x"].shape[3])
            d64[i]["db_ab_terms"] = C64.conv_db((gs * C64.partial_factors(f64[i]["um1"], f64[i]["a2"].shape[1])[1]).abs())
        terms = _net_terms(c, c["r64"], i)
        r64 = dict(grads={n: d64[i]["d_" + n] for n in S64.names_of(c["blocks"][i][0])}, terms=terms)
        r32 = dict(grads={n: d32[i]["d_" + n] for n in S64.names_of(c["blocks"][i][0])})
        for b in ("b_aa", "b_ab", "b_b"):
            if c["blocks"][i][0].get(b) is not None:
                r64["grads"][b], r32["grads"][b] = d64[i]["d" + b], d32[i]["d" + b]
        _check_grads(blk, r64, r32, f"block {i} ")
        for name, path in LEAVES:
            m = _leaf(blk, path)
            if m is not None:
                held(f"block {i} u {name}", m.weight_u.cpu(), u64[i][name][0], u32[i][name][0])
                held(f"block {i} v {name}", m.weight_v.cpu(), u64[i][name][1], u32[i][name][1])


def test_eval_mode_agrees_with_the_folded_network(S):
    """A spectral=True network filled from a synthetic reference state dict against the spectral=False network that
    nets.load_reference_state_dict fills from the same dict (it folds), both in eval mode, and both against float64."""
    for kind, prefix in (("decoder", "model.module.projector."), ("encoder", "model.module.encoder.")):
        c = _net_case(kind)
        src = S64.settle(_net(S, c))
        with torch.no_grad():
            for m in src.modules():
                if hasattr(m, "stored_var"):
                    m.stored_mean.copy_(0.1 * torch.randn_like(m.stored_mean)), m.stored_var.copy_(0.5 + torch.rand_like(m.stored_var))
        sd = {k: v.cpu() for k, v in S.reference_state_dict(src, prefix).items()}
        a = S.load_spectral_state_dict(_net(S, c), sd, prefix).eval()
        b = S.nets.load_reference_state_dict(_net(S, c, spectral=False), sd, prefix).eval()
        x = c["x"].to(DEV)
        torch.cuda.synchronize()
        with _no_sync(), torch.no_grad():
            ya, yb = _out(c, a(x)), _out(c, b(x))
            ya2 = _out(c, a(x))                          # the kept state of the eval group: nothing is made again
        assert torch.equal(ya, ya2)
        ps = [{**p, **{n: m.weight_orig.detach().cpu() for n, path in LEAVES for m in [_leaf(blk, path)] if m is not None}}
              for blk, (p, _) in zip(a.blocks, c["blocks"])]
        uvs = [{n: (m.weight_u.cpu(), m.weight_v.cpu()) for n, path in LEAVES for m in [_leaf(blk, path)] if m is not None} for blk in a.blocks]
        stored = [((blk.bn1.stored_mean.cpu(), blk.bn1.stored_var.cpu()), (blk.bn2.stored_mean.cpu(), blk.bn2.stored_var.cpu())) for blk in a.blocks]
        zero = [(torch.zeros(2, 20), torch.zeros(2, 20))] * 8

        def ref(dt):
            cast = lambda t: S64.cast(t, dt)                                  # noqa: E731
            fs, _, _ = S64.network(c["forms"], cast(c["x"]), cast(ps), cast(uvs), c["kinds"], cast(zero), False, cast(stored))
            return fs[-1]["y"]
        r64, r32 = ref(torch.float64), ref(torch.float32)
        held(f"{kind} eval, spectral=True", ya.cpu(), r64, r32)
        held(f"{kind} eval, folded", yb.cpu(), r64, r32)
        e, e_plain = C64.E(ya.cpu(), yb.cpu().double()), C64.E(r32, r64)
        print(f"{kind} eval, spectral=True against folded: E {e:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
        assert e <= bound(e_plain)
        for m in a.modules():
            if getattr(m, "spectral_leaf", False):       # eval moves nothing
                assert torch.equal(m.weight_u.cpu(), sd[prefix + _ref_key(a, m) + ".weight_u"])
                assert torch.equal(m.weight_v.cpu(), sd[prefix + _ref_key(a, m) + ".weight_v"])


@pytest.mark.parametrize("case", ["encoder_with_z", "decoder_holes"])
def test_eval_mode_from_the_references_own_key_lists(S, case):
    """Full-size networks filled from state dicts with the reference's recorded keys and shapes (tests/golden/nets_vs_reference.npz,
    tensors of tests/nets_fixture.py): the spectral=True network, the folded spectral=False network and the inference class evaluated by
    torch on the CPU in float64 / float32 (nets.cpu_reference: an implementation that shares no code with the loaders under test)."""
    import nets_fixture as NF
    from test_spectral_f64 import RECORDED, recorded_state_dict
    sd, prefix = recorded_state_dict(case)
    _, cls, args, _, _, _ = NF.VS_REFERENCE[case]
    x = NF.vs_reference_input(case)
    out = lambda y: torch.cat(y, 1) if isinstance(y, tuple) else y             # noqa: E731
    refs = {}
    for dt in (torch.float64, torch.float32):
        m = S.nets.load_reference_state_dict(getattr(S.nets, cls)(*args).to(dt), {k: v.to(dt) for k, v in sd.items()}, prefix).eval()
        with torch.no_grad(), S.nets.cpu_reference():
            refs[dt] = out(m(x.to(dt)))
    a = S.load_spectral_state_dict(RECORDED[case](S.trainable, True), sd, prefix).to(DEV).eval()
    b = S.nets.load_reference_state_dict(RECORDED[case](S.trainable, False), sd, prefix).to(DEV).eval()
    xd = x.to(DEV)
    torch.cuda.synchronize()
    with _no_sync(), torch.no_grad():
        ya, yb = out(a(xd)), out(b(xd))
    held(f"{case} eval, spectral=True", ya.cpu(), refs[torch.float64], refs[torch.float32])
    held(f"{case} eval, folded", yb.cpu(), refs[torch.float64], refs[torch.float32])
    e, e_plain = C64.E(ya.cpu(), yb.cpu().double()), C64.E(refs[torch.float32], refs[torch.float64])
    print(f"{case} eval, spectral=True against folded: E {e:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    assert e <= bound(e_plain)
    back = S.reference_state_dict(a, prefix)
    assert set(back) == set(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)        # eval moved nothing; every key comes back


def _ref_key(net, leaf):
    from slr_sfs_amd import spectral
    return [key for _, m, key in spectral._pairs(net) if m is leaf][0]


# ------------------------------------------------------------------ after an optimiser step

def test_adam_step_is_seen_and_nothing_synchronises(S):
    """forward + backward + Adam.step() under a sync guard; then the next forward in train() and in eval() mode uses the new
    weight_orig (and the u, v the first forward left), against float64."""
    c = _net_case("encoder")
    net = _net(S, c)
    names = {id(p): n for n, p in net.named_parameters()}
    opt = S.Adam(list(net.parameters()), lr=1e-2, betas=(0.0, 0.9))
    assert sum(1 for n in names.values() if n.endswith("weight_orig")) == len(S.SpectralGroup([net]).leaves)
    x = c["x"].to(DEV)
    noise = [tuple(t.to(DEV) for t in nz) for nz in c["noise"]]
    g = c["g"].to(DEV)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    torch.cuda.synchronize()
    with _no_sync():
        _out(c, net(x, noise=noise)).backward(g)
        opt.step()
        y_train = _out(c, net(x, noise=noise)).detach()
        net.eval()
        with torch.no_grad():
            y_eval = _out(c, net(x, noise=noise))
    assert all(p.grad is not None for p in net.parameters())
    still = [n for n, p in net.named_parameters() if n.endswith("weight_orig") and torch.equal(p, before[n])]
    assert not still, f"weight_orig tensors the step did not move: {still}"
    ps = [{**p, **{n: _leaf(blk, path).weight_orig.detach().cpu() for n, path in LEAVES if _leaf(blk, path) is not None},
           "b_aa": blk.conv_aa.bias.detach().cpu(), "b_ab": blk.conv_ab.bias.detach().cpu(),
           "b_b": None if blk.conv_b is None else blk.conv_b.bias.detach().cpu()} for blk, (p, _) in zip(net.blocks, c["blocks"])]
    for dt_name in ("train", "eval"):
        def ref(dt, dt_name=dt_name):
            u1 = c["run"](dt, grads=False)[1]                                  # u, v after the first forward
            fs2, u2, _, _ = c["run"](dt, ps=ps, uvs=u1, grads=False)
            if dt_name == "train":
                return fs2[-1]["y"]
            # the BNs' stored statistics after two training forwards: 0.9 (0.9 s0 + 0.1 b1) + 0.1 b2
            fs1 = c["run"](dt, grads=False)[0]
            stored = [tuple((0.1 * 0.9 * f1[f"mean{k}"] + 0.1 * f2[f"mean{k}"], 0.81 + 0.09 * f1[f"var{k}"] + 0.1 * f2[f"var{k}"]) for k in (1, 2))
                      for f1, f2 in zip(fs1, fs2)]
            return c["run"](dt, ps=ps, uvs=u2, training=False, stored=stored, grads=False)[0][-1]["y"]
        held(f"y after the step, {dt_name}()", (y_train if dt_name == "train" else y_eval).cpu(), ref(torch.float64), ref(torch.float32))
