"""The Winograd fp32 convolution (csrc/conv_wino.hpp: conv3x3_wino_kernel, convs="fp32-winograd") against float64 on every path it has.
The cases are the table of tests/wino_model.py (16 small shapes: every block / slice / chunk / group count at which the kernel takes another
path); references are the written-out convolutions of tests/conv_train_f64.py on the CPU, never a kernel.

  a. exact probes: integer inputs on which every fp32 operation of the algorithm is exact (tests/test_wino_model.py proves it) -- bit for bit
     against the float64 convolution, plain / bias + residual / BN + ReLU prologue; one-hot pixels at corners, block seams and ragged edges,
     with dense weights and with a single tap.
  b. accuracy: E_gpu <= 10 E_plain32 + 1e-6 (E = max|got - ref64| / max|ref64|, no floor; the criterion of test_gpu_conv_train.py) on dense
     randn, randn + 100 and relu(randn) inputs; E_gpu, E_plain32, E_wino32 (the fp32 CPU model) and E_direct (the rung's direct kernel on
     the same layer) per case are printed (-s): profiles/conv_wino_range.txt is that output.
  c. layouts are addressing only: IN_B8 / OUT_B8 / RES_B8 variants and outputs / residuals 4 bytes off an 8-byte boundary are BIT-identical to
     the NCHW run; outputs start as NaN, guard bands around them stay untouched.
  d. the partial convolution against its definition (conv_train_f64.pconv, nets.pconv_epilogue's torch composition in float64): explicit mask
     (NCHW and channel-blocked), derived mask; update mask bit for bit, exact zeros where it is 0.
  e. conv(2^k x) == 2^k conv(x) bit for bit, k = -40, -20, 20, 40: no clamp, flush or reduced-precision detour.
  f. the edge of the contract through the C ABI: Cin = 272 (17 chunks) runs without a prologue and is refused with one; SLR_CONV_WINO without
     SLR_CONV_F32, with Cout <= 4 and on the skip entry points is refused.

Cases with Cin <= 256 go through nets.Conv / nets.PartialConv inside nets.fp32_kernels(winograd=True) (their outputs come from torch.empty, made
NaN-filled by torch's deterministic mode) and assert that the Winograd weight form ``_wwino`` is what ran; Cin = 272, guard bands and offset
pointers need slr_conv3x3_forward itself (with the module's own ``_wwino`` buffer where there is a module)."""
import functools
import math

import pytest
import torch

import conv_train_f64 as cf
import wino_model as wm
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
IDX = list(range(len(wm.CASES)))
GUARD, SENTINEL = 64, 12345.0                        # floats of guard band on either side of a raw output (256 bytes: keeps 16-byte alignment)


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


TABLE = []                                           # (tag, E_gpu, E_plain32, E_wino32, E_direct or None) of sections b and d


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    if TABLE:
        by_wino, by_plain = max(TABLE, key=lambda r: ratio(r[1], r[3])), max(TABLE, key=lambda r: ratio(r[1], r[2]))
        print(f"\nwino worst E_gpu / E_wino32 {ratio(by_wino[1], by_wino[3]):.2f} ({by_wino[0]}); worst E_gpu / E_plain32 {ratio(by_plain[1], by_plain[2]):.2f} "
              f"({by_plain[0]}); largest E_gpu {max(r[1] for r in TABLE):.2e}, E_wino32 {max(r[3] for r in TABLE):.2e}, "
              f"E_plain32 {max(r[2] for r in TABLE):.2e} over {len(TABLE)} rows")
        with_direct = [r for r in TABLE if r[4] is not None]
        if with_direct:
            q = sorted(ratio(r[1], r[4]) for r in with_direct)
            print(f"wino against the direct fp32 kernel on the same layers: E_gpu / E_direct {q[0]:.2f} .. {q[-1]:.2f}, median {q[len(q) // 2]:.2f}; largest "
                  f"E_direct {max(r[4] for r in with_direct):.2e}, largest E_gpu there {max(r[1] for r in with_direct):.2e} over {len(q)} rows")


def bound(e_plain):
    return 10.0 * e_plain + 1e-6


def ratio(a, b):
    return a / b if b else math.inf


def judge(tag, got, ref, p32, w32, direct=None):
    """One row of the table; ``direct``: the same layer on the direct fp32 kernel (a figure, not a criterion: tests/test_gpu_conv_f32.py holds it)."""
    e_gpu, e_plain, e_wino = wm.E(got, ref), wm.E(p32, ref), wm.E(w32, ref)
    e_direct = None if direct is None else wm.E(direct, ref)
    TABLE.append((tag, e_gpu, e_plain, e_wino, e_direct))
    print(f"wino {tag}: E_gpu {e_gpu:.2e} E_plain32 {e_plain:.2e} E_wino32 {e_wino:.2e} bound {bound(e_plain):.2e} "
          f"E_gpu/E_plain32 {ratio(e_gpu, e_plain):.2f} E_gpu/E_wino32 {ratio(e_gpu, e_wino):.2f}"
          + ("" if direct is None else f" E_direct {e_direct:.2e} E_gpu/E_direct {ratio(e_gpu, e_direct):.2f}"))
    return e_gpu <= bound(e_plain), (tag, e_gpu, bound(e_plain))


# ------------------------------------------------------------------------------------------------------------------ running the kernel

class nan_empty:
    """Inside, torch.empty returns NaN-filled memory (torch.utils.deterministic.fill_uninitialized_memory): an output element the kernel
    does not write stays NaN."""

    def __enter__(self):
        self._prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
        assert torch.utils.deterministic.fill_uninitialized_memory
        torch.use_deterministic_algorithms(True, warn_only=True)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self._prev[0], warn_only=self._prev[1])
        return False


def ran_winograd(mod):
    return mod.__dict__.get("_wwino") is not None and mod.__dict__.get("_wf32") is None and mod.__dict__.get("_wsplit") is None


def layer(nets, wt, bias=None, partial=False):
    cout, cin = wt.shape[:2]
    mod = (nets.PartialConv if partial else nets.Conv)(cin, cout, 3, **({} if partial else {"bias": bias is not None})).cuda()
    with torch.no_grad():
        mod.weight.copy_(wt)
        if bias is not None:
            mod.bias.copy_(bias)
    return mod


def wino_buffer(S, wt):
    """The Winograd-domain weight buffer of ``wt``: the module's own ``_wwino`` where nets.Conv takes the Winograd kernel (Cin <= 256), else
    slr_conv3x3_wino_weights itself."""
    nets, _lib = S.nets, S._lib
    cout, cin = wt.shape[:2]
    if cin <= wm.WN_MAXCIN:
        mod = layer(nets, wt)
        with nets.fp32_kernels(winograd=True):
            buf, wscale, xscale, arith = mod._split_weights()
        assert ran_winograd(mod) and (wscale, xscale, arith) == (1.0, 1.0, nets.CONV_F32 | nets.CONV_WINO)
        return buf
    buf = torch.empty(_lib.lib().slr_conv3x3_wino_weight_bytes(cout, cin), dtype=torch.uint8, device=DEV)
    _lib.call("slr_conv3x3_wino_weights", buf.device, wt.cuda().contiguous(), buf, cout, cin)
    return buf


def offset_view(t, shift, fill=None):
    """(buffer, a contiguous view of the shape of ``t`` that starts GUARD + ``shift`` floats into it): a copy of ``t``, or all ``fill``;
    SENTINEL around it."""
    n = t.numel()
    big = torch.full((GUARD + shift + n + GUARD,), SENTINEL, device=DEV)
    view = big[GUARD + shift:GUARD + shift + n].view(t.shape)
    view.copy_(t) if fill is None else view.fill_(fill)
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + 4 * (GUARD + shift) and big.data_ptr() % 16 == 0
    return big, view


def raw_conv(S, buf, x, bias, res, pre, layout, dims, shift_out=0, shift_res=0):
    """slr_conv3x3_forward with SLR_CONV_F32 | SLR_CONV_WINO on device tensors, the output a NaN-filled view between guard bands (``shift_*``:
    floats past the 16-byte boundary).  Nothing outside the output is written, no NaN is left inside."""
    nets, _lib = S.nets, S._lib
    n, cin, cout, h, w = dims
    big, out = offset_view(torch.empty(n, cout, h, w), shift_out, fill=float("nan"))
    if res is not None and shift_res:
        _, res = offset_view(res, shift_res)
        assert res.data_ptr() % 8 == 4
    assert out.data_ptr() % 8 == (4 if shift_out else 0)
    psc, psh = pre if pre is not None else (None, None)
    _lib.call("slr_conv3x3_forward", out.device, x, buf, bias, res, out, n, cin, cout, h, w, 1.0, 1.0, psc, psh,
              layout | nets.CONV_F32 | nets.CONV_WINO)
    torch.cuda.synchronize()
    lo = GUARD + shift_out
    assert bool((big[:lo] == SENTINEL).all()) and bool((big[lo + out.numel():] == SENTINEL).all()), "written outside the output"
    assert not bool(torch.isnan(out).any()), "output elements left unwritten"
    return out


def conv_gpu(S, d, mode, layout=0, raw=False, shift_out=0, shift_res=0):
    """The convolution of the inputs ``d`` (wino_model.exact_inputs / dense_inputs) in ``mode`` on the Winograd kernel -> host tensor, NCHW.
    ``layout``: IN_B8 / OUT_B8 / RES_B8 -- the operands are handed over channel-blocked and the result is un-blocked here."""
    nets = S.nets
    n, cin, h, w = d["x"].shape
    cout = d["w"].shape[0]
    x = d["x"].cuda()
    bias, res = (None, None) if mode == "plain" else (d["bias"].cuda(), d["res"].cuda())
    pre = (d["sc"].cuda(), d["sh"].cuda()) if mode == "prologue" else None
    if layout & nets.IN_B8:
        x = to_blocked(x)
    if layout & nets.RES_B8:
        res = to_blocked(res)
    if raw or cin > wm.WN_MAXCIN:
        y = raw_conv(S, wino_buffer(S, d["w"]), x, bias, res, pre, layout, (n, cin, cout, h, w), shift_out, shift_res)
    else:
        mod = layer(nets, d["w"], bias)
        with torch.no_grad(), nets.fp32_kernels(winograd=True), nan_empty():
            y = mod(x, pre, res, layout)
        assert ran_winograd(mod)
        assert not bool(torch.isnan(y).any()), "output elements left unwritten"
    return (from_blocked(y) if layout & nets.OUT_B8 else y).cpu()


def direct_gpu(S, d, mode):
    """The same layer on the rung's direct kernel (nets.fp32_kernels(winograd=False)) -> host tensor."""
    nets = S.nets
    mod = layer(nets, d["w"], None if mode == "plain" else d["bias"])
    with torch.no_grad(), nets.fp32_kernels(winograd=False):
        y = mod(d["x"].cuda(), (d["sc"].cuda(), d["sh"].cuda()) if mode == "prologue" else None, None if mode == "plain" else d["res"].cuda())
    assert mod.__dict__.get("_wf32") is not None and mod.__dict__.get("_wwino") is None
    return y.cpu()


def first_difference(got, want):
    bad = (got.double() != want.double()).nonzero()
    if not len(bad):
        return None
    n, o, y, x = bad[0].tolist()
    return f"{len(bad)} outputs differ, first [image {n}, channel {o}, y {y}, x {x}]: got {float(got[n, o, y, x])!r} want {float(want[n, o, y, x])!r}"


@functools.lru_cache(maxsize=None)
def dense_refs(i, variant, mode):
    """(ref64, plain32, wino32) of case ``i``: computed once, shared, never modified."""
    d = wm.dense_inputs(wm.CASES[i], variant)
    return (wm.reference(d, mode, F64, cf.conv), wm.reference(d, mode, F32, cf.conv), wm.reference(d, mode, F32, wm.conv))


# ------------------------------------------------------------------------------------------------------------------ a. exact probes

@pytest.mark.parametrize("i", IDX, ids=wm.CASE_IDS)
def test_a_integer_probes_equal_float64_bit_for_bit(S, i):
    """Integer inputs (wino_model.exact_inputs): the output IS the float64 convolution -- plain, + bias + residual, behind the prologue.
    (Cin = 272 is section f's: through the C ABI, no prologue.)"""
    d = wm.exact_inputs(wm.CASES[i])
    for mode in wm.modes(wm.CASES[i]):
        diff = first_difference(conv_gpu(S, d, mode), wm.reference(d, mode, F64, cf.conv))
        assert diff is None, (mode, diff)


@pytest.mark.parametrize("cin,cout,h,w", wm.ONE_HOT_SHAPES)
def test_a_one_hot_probes(S, cin, cout, h, w):
    """One non-zero pixel per image (corners, x = 15 | 16, y = 7 | 8, last ragged column / row: wino_model.one_hot_pixels) under dense integer
    weights and under each single tap: bit for bit, a failure names the probe and the output pixel."""
    for tap in [None] + cf.TAPS:
        x, wt, names = wm.one_hot_inputs(cin, cout, h, w, tap)
        got, want = conv_gpu(S, {"x": x, "w": wt}, "plain"), cf.conv(x.double(), wt.double())
        bad = (got.double() != want).nonzero()
        if len(bad):
            p, o, y, xx = bad[0].tolist()
            pytest.fail(f"probe '{names[p]}' at {wm.one_hot_pixels(h, w)[names[p]]}, tap {tap}: {len(bad)} outputs differ, first channel {o} at "
                        f"({y}, {xx}): got {float(got[p, o, y, xx])!r} want {float(want[p, o, y, xx])!r}")


# ------------------------------------------------------------------------------------------------------------------ b. accuracy

@pytest.mark.parametrize("i", IDX, ids=wm.CASE_IDS)
def test_b_accuracy_against_float64(S, i):
    """E_gpu <= 10 E_plain32 + 1e-6 on randn, randn + 100 and relu(randn), plain / bias + residual / prologue (N = 3: cases 1, 3, 7, 9)."""
    failures = []
    for variant in wm.VARIANTS:
        d = wm.dense_inputs(wm.CASES[i], variant)
        for mode in wm.modes(wm.CASES[i]):
            ok, what = judge(f"{wm.CASE_IDS[i]} {variant} {mode}", conv_gpu(S, d, mode), *dense_refs(i, variant, mode), direct_gpu(S, d, mode))
            if not ok:
                failures.append(what)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------ c. layouts are addressing

BLOCKABLE = [i for i in IDX if wm.CASES[i][0] % 8 == 0 or wm.CASES[i][1] % 8 == 0]


@pytest.mark.parametrize("i", BLOCKABLE, ids=[wm.CASE_IDS[i] for i in BLOCKABLE])
def test_c_blocked_layouts_are_bit_identical_to_nchw(S, i):
    """IN_B8, OUT_B8, IN_B8 | OUT_B8, OUT_B8 | RES_B8, OUT_B8 with an NCHW residual, and the form a residual block's second convolution takes
    on this rung (nets._block_route: prologue, IN_B8 | OUT_B8 | RES_B8): load_item and the store branch change addresses, no arithmetic."""
    nets = S.nets
    cin, cout = wm.CASES[i][:2]
    I, O, R = (nets.IN_B8 if cin % 8 == 0 else None), (nets.OUT_B8 if cout % 8 == 0 else None), nets.RES_B8
    d = wm.dense_inputs(wm.CASES[i])
    base = {mode: conv_gpu(S, d, mode) for mode in wm.modes(wm.CASES[i])}
    variants = [("plain", I), ("bias+residual", I), ("plain", O), ("bias+residual", O)]
    if O:
        variants += [("bias+residual", O | R)] + ([("plain", I | O), ("bias+residual", I | O | R)] if I else [])
        if "prologue" in base:
            variants += [("prologue", O | R)] + ([("prologue", I | O | R)] if I else [])
    ran = 0
    for mode, layout in variants:
        if layout is None:
            continue
        diff = first_difference(conv_gpu(S, d, mode, layout, raw=True), base[mode])
        assert diff is None, (mode, layout, diff)
        ran += 1
    assert ran >= 2


PAIR_CASES = [i for i in IDX if wm.CASES[i][2:4] == (24, 48)]


@pytest.mark.parametrize("i", PAIR_CASES, ids=[wm.CASE_IDS[i] for i in PAIR_CASES])
def test_c_output_and_residual_off_the_8_byte_boundary(S, i):
    """Even W: rows go out as 8-byte pairs -- unless the output or the residual is only 4-byte aligned (legal for NCHW), which the kernel finds
    out at run time (pair_ok).  Output, residual and both one float past a 16-byte boundary: bit-identical to the aligned run."""
    d = wm.dense_inputs(wm.CASES[i])
    aligned = conv_gpu(S, d, "bias+residual", raw=True)
    assert first_difference(aligned, conv_gpu(S, d, "bias+residual")) is None
    for so, sr in ((1, 0), (0, 1), (1, 1)):
        diff = first_difference(conv_gpu(S, d, "bias+residual", raw=True, shift_out=so, shift_res=sr), aligned)
        assert diff is None, (so, sr, diff)


# ------------------------------------------------------------------------------------------------------------------ d. partial convolution

PCONV = [i for i in IDX if wm.CASES[i][2] >= 8 and wm.CASES[i][0] <= wm.WN_MAXCIN]       # (a 1x1 image under holed_mask has no valid pixel)
PCONV_MODES = ("mask", "mask+prologue", "mask b8", "mask+prologue b8", "derived")
EPILOGUES = ("plain", "residual", "next_bn")


def box3(mask):
    return sum(cf.shifted(mask, ky - 1, kx - 1) for ky, kx in cf.TAPS)


def pconv_definition(nets, xm, mask, w, b, res, nbn, dtype, conv_fn):
    """(out, um) of the partial convolution of the already masked input ``xm`` in ``dtype``: conv_train_f64.pconv; with a residual or the next
    layer's BN nets.pconv_epilogue's torch composition on the raw convolution ``conv_fn`` (cf.conv, or the Winograd model)."""
    cin = xm.shape[1]
    xm, mask, w, b = xm.to(dtype), mask.to(dtype), w.to(dtype), b.to(dtype)
    if res is None and nbn is None and conv_fn is cf.conv:
        return cf.pconv(xm, mask, w, b)
    with nets.cpu_reference():
        return nets.pconv_epilogue(conv_fn(xm, w), b, box3(mask), float(cin), float(cin * 9), None if res is None else res.to(dtype),
                                   None if nbn is None else (nbn[0].to(dtype), nbn[1].to(dtype)))


@pytest.mark.parametrize("i", PCONV, ids=[wm.CASE_IDS[i] for i in PCONV])
def test_d_partial_convolution_against_its_definition(S, i):
    """nets.PartialConv on the Winograd kernel: explicit mask (x already masked, or raw behind the prologue; NCHW and channel-blocked, the
    blocked runs with blocked output and residual where Cout allows: the residual blocks' layouts) and derived mask (x != 0, prologue), each
    plain, with a residual and with the next layer's BN.  Update mask bit for bit, out by the criterion of section b, exact zeros (the
    residual itself) where the update mask is 0."""
    nets = S.nets
    case = wm.CASES[i]
    cin, cout, h, w, n = case
    d = wm.dense_inputs(case)
    mask = cf.holed_mask(n, h, w, seed=i)
    g = torch.Generator().manual_seed(500 + i)
    nbn = (torch.rand(cout, generator=g) + 0.5, 0.3 * torch.randn(cout, generator=g))
    masked = d["x"] * mask                                           # randn is never 0: (masked != 0) == mask in every channel
    assert bool(((masked != 0) == (mask != 0)).all())
    mod = layer(nets, d["w"], d["bias"], partial=True)
    failures = []
    for pmode in PCONV_MODES:
        b8 = pmode.endswith("b8")
        if b8 and cin % 8:
            continue
        pre = (d["sc"], d["sh"]) if pmode != "mask" and pmode != "mask b8" else None
        xk = masked if pmode in ("mask", "mask b8", "derived") else d["x"]
        xm = {T: (xk.to(T) if pre is None else wm.prologue(xk.to(T), *pre) * mask.to(T)) for T in (F64, F32)}
        for epi in EPILOGUES:
            res, nb = (d["res"] if epi == "residual" else None), (nbn if epi == "next_bn" else None)
            ref, um_ref = pconv_definition(nets, xm[F64], mask, d["w"], d["bias"], res, nb, F64, cf.conv)
            p32, _ = pconv_definition(nets, xm[F32], mask, d["w"], d["bias"], res, nb, F32, cf.conv)
            w32, _ = pconv_definition(nets, xm[F32], mask, d["w"], d["bias"], res, nb, F32, wm.conv)
            if epi == "plain":                                       # the two statements of the definition agree
                alt, um_alt = pconv_definition(nets, xm[F64], mask, d["w"], d["bias"], res, nb, F64, wm.conv)
                assert torch.equal(um_alt, um_ref) and wm.E(alt, ref) <= 1e-12
            ob8 = b8 and cout % 8 == 0
            layout = (nets.IN_B8 if b8 else 0) | (nets.OUT_B8 if ob8 else 0) | (nets.RES_B8 if ob8 and res is not None else 0)
            xg, rg = xk.cuda(), None if res is None else res.cuda()
            with torch.no_grad(), nets.fp32_kernels(winograd=True), nan_empty():
                out, um = mod(to_blocked(xg) if b8 else xg, None if pmode == "derived" else mask.cuda(),
                              residual=to_blocked(rg) if layout & nets.RES_B8 else rg, next_bn=None if nb is None else (nb[0].cuda(), nb[1].cuda()),
                              pre_bn=None if pre is None else (pre[0].cuda(), pre[1].cuda()), layout=layout)
            assert ran_winograd(mod)
            out, um = (from_blocked(out) if ob8 else out).cpu(), um.cpu()
            tag = f"{wm.CASE_IDS[i]} pconv {pmode} {epi}"
            assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(um).any()), tag
            assert torch.equal(um.double(), um_ref), tag
            assert bool((um_ref == 0).any()) and bool((um_ref == 1).any())
            hole = (um_ref == 0).expand_as(out)
            assert torch.equal(out[hole], (res[hole] if res is not None else torch.zeros_like(out)[hole])), tag
            ok, what = judge(tag, out, ref, p32, w32)
            if not ok:
                failures.append(what)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------ e. power-of-two equivariance

EQUIVARIANT = [3, 8, 10]
EXPONENTS = (-40, -20, 20, 40)


@pytest.mark.parametrize("i", EQUIVARIANT, ids=[wm.CASE_IDS[i] for i in EQUIVARIANT])
def test_e_power_of_two_equivariance(S, i):
    """x, bias, residual and the prologue / next-BN shifts times 2^k: the result is 2^k times the unscaled one, bit for bit (nothing under- or
    overflows at k = -40 .. 40: |x| spans 1e-17 .. 5e12, fp32 32 orders of magnitude more).  Plain and partial convolution; nothing saturates."""
    nets = S.nets
    case = wm.CASES[i]
    cin, cout, h, w, n = case
    d = wm.dense_inputs(case)
    mask = cf.holed_mask(n, h, w, seed=i)
    g = torch.Generator().manual_seed(600 + i)
    nsc, nsh = torch.rand(cout, generator=g) + 0.5, 0.3 * torch.randn(cout, generator=g)
    pmod = layer(nets, d["w"], d["bias"], partial=True)

    def scaled(k):
        s = 2.0 ** k
        return dict(d, x=d["x"] * s, bias=d["bias"] * s, res=d["res"] * s, sh=d["sh"] * s)

    def partial(dk, k, derived):
        """derived mask + prologue + residual, or explicit mask + prologue + next BN"""
        xk = (dk["x"] * mask).cuda()
        with torch.no_grad(), nets.fp32_kernels(winograd=True), nan_empty():
            pmod.bias.copy_(dk["bias"])
            pre = (dk["sc"].cuda(), dk["sh"].cuda())
            if derived:
                out, um = pmod(xk, None, residual=dk["res"].cuda(), pre_bn=pre)
            else:
                out, um = pmod(xk, mask.cuda(), next_bn=(nsc.cuda(), (nsh * 2.0 ** k).cuda()), pre_bn=pre)
        assert ran_winograd(pmod)
        return out.cpu(), um.cpu()

    nets.saturation_count(DEV)
    one = {mode: conv_gpu(S, d, mode) for mode in wm.modes(case)}
    pone = {derived: partial(d, 0, derived) for derived in (True, False)}
    for k in EXPONENTS:
        dk = scaled(k)
        for mode in wm.modes(case):
            diff = first_difference(conv_gpu(S, dk, mode), one[mode] * 2.0 ** k)
            assert diff is None, (k, mode, diff)
        for derived in (True, False):
            out, um = partial(dk, k, derived)
            assert torch.equal(um, pone[derived][1])
            diff = first_difference(out, pone[derived][0] * 2.0 ** k)
            assert diff is None, (k, "pconv derived" if derived else "pconv mask", diff)
    for t in list(one.values()) + [p[0] for p in pone.values()]:
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    assert nets.saturation_count(DEV) == 0


# ------------------------------------------------------------------------------------------------------------------ f. the edge of the contract

WIDE = [i for i in IDX if wm.CASES[i][0] > wm.WN_MAXCIN]


def test_f_wide_cases_are_in_sections_a_and_b():
    """Cin = 272 without a prologue runs (17 chunks; nets.Conv never routes it) and meets sections a and b: those tests take it through the C ABI."""
    assert [wm.CASES[i][0] for i in WIDE] == [272, 272] and all("prologue" not in wm.modes(wm.CASES[i]) for i in WIDE)
    assert {wm.CASES[i][2:4] for i in WIDE} == {(17, 35), (24, 48)}


def test_f_refusals(S):
    """Every request outside the kernel's contract returns SLR_E_BADARG (-1) and launches nothing: Cin > 256 with a prologue, SLR_CONV_WINO
    without SLR_CONV_F32 or with Cout <= 4, and on the four skip entry points.  (Every buffer is a valid one for the shape.)"""
    nets, _lib = S.nets, S._lib
    L, ptr = _lib.lib(), _lib.ptr
    WINO = nets.CONV_F32 | nets.CONV_WINO

    def refused(rc, text):
        return rc == -1 and text in L.slr_last_error()

    # Cin = 272 with a prologue
    d = wm.dense_inputs(wm.CASES[WIDE[0]])
    n, cin, h, w = d["x"].shape
    cout = d["w"].shape[0]
    x, buf, out = d["x"].cuda(), wino_buffer(S, d["w"]), torch.zeros(n, cout, h, w, device=DEV)
    sc, sh = d["sc"].cuda(), d["sh"].cuda()
    st = _lib.stream_of(x)
    rc = L.slr_conv3x3_forward(ptr(x), ptr(buf), None, None, ptr(out), n, cin, cout, h, w, 1.0, 1.0, ptr(sc), ptr(sh), WINO, st)
    assert refused(rc, b"Cin <= 256"), (rc, L.slr_last_error())
    with pytest.raises(RuntimeError, match="Cin <= 256"):
        _lib.call("slr_conv3x3_forward", x.device, x, buf, None, None, out, n, cin, cout, h, w, 1.0, 1.0, sc, sh, WINO)
    # the same through the partial entry point (explicit mask behind the prologue)
    mask, bias, um = torch.ones(n, 1, h, w, device=DEV), torch.zeros(cout, device=DEV), torch.zeros(n, 1, h, w, device=DEV)
    rc = L.slr_pconv3x3_forward(ptr(x), ptr(sc), ptr(sh), ptr(mask), ptr(buf), 1.0, 1.0, ptr(bias), None, None, None, ptr(out), ptr(um),
                                n, cin, cout, h, w, WINO, st)
    assert refused(rc, b"Cin <= 256"), (rc, L.slr_last_error())
    assert not bool(out.any()) and not bool(um.any())

    # SLR_CONV_WINO without SLR_CONV_F32; with Cout <= 4
    cin, cout, h, w = 64, 64, 8, 16
    g = torch.Generator().manual_seed(9)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / 24.0
    xb, buf, out = to_blocked(torch.randn(1, cin, h, w, generator=g)).cuda(), wino_buffer(S, wt), torch.zeros(1, cout, h, w, device=DEV)
    rc = L.slr_conv3x3_forward(ptr(xb), ptr(buf), None, None, ptr(out), 1, cin, cout, h, w, 1.0, 1.0, None, None, nets.CONV_WINO, st)
    assert refused(rc, b"SLR_CONV_WINO goes with SLR_CONV_F32"), (rc, L.slr_last_error())
    for few in (1, 4):
        fbuf = torch.zeros(L.slr_conv3x3_wino_weight_bytes(few, cin), dtype=torch.uint8, device=DEV)
        rc = L.slr_conv3x3_forward(ptr(xb), ptr(fbuf), None, None, ptr(out), 1, cin, few, h, w, 1.0, 1.0, None, None, WINO, st)
        assert refused(rc, b"more than 4 output channels"), (few, rc, L.slr_last_error())

    # the skip entry points: the fused skip branch (channel-blocked operands, as the residual blocks call it) ...
    lay = WINO | nets.IN_B8 | nets.OUT_B8 | nets.SKIP_B8
    sbuf = torch.zeros(L.slr_conv1x1_weight_bytes(cout, cin), dtype=torch.uint8, device=DEV)
    bias, mask, um = torch.zeros(cout, device=DEV), torch.ones(1, 1, h, w, device=DEV), torch.zeros(1, 1, h, w, device=DEV)
    rc = L.slr_conv3x3_forward_skip(ptr(xb), ptr(buf), ptr(bias), ptr(out), 1, cin, cout, h, w, 1.0, 1.0, None, None,
                                    ptr(xb), ptr(sbuf), None, cin, 1.0, None, 0, lay, st)
    assert refused(rc, b"no fused skip branch in the Winograd kernel"), (rc, L.slr_last_error())
    rc = L.slr_pconv3x3_forward_skip(ptr(xb), None, None, ptr(mask), ptr(buf), 1.0, 1.0, ptr(bias), ptr(out), ptr(um), 1, cin, cout, h, w,
                                     ptr(xb), ptr(sbuf), cin, 1.0, None, 0, lay, st)
    assert refused(rc, b"no fused skip branch in the Winograd kernel"), (rc, L.slr_last_error())
    # ... and the skip output of the <= 4-channel kernel
    few = 3
    fbuf = torch.zeros(max(L.slr_conv3x3_wino_weight_bytes(few, cin), L.slr_conv3x3_weight_bytes(few, cin)), dtype=torch.uint8, device=DEV)
    w4, fout, skip = torch.zeros(cin, 4, device=DEV), torch.zeros(1, few, h, w, device=DEV), torch.zeros(1, few, h, w, device=DEV)
    rc = L.slr_conv3x3_forward_skipout(ptr(xb), ptr(fbuf), ptr(bias), None, ptr(fout), 1, cin, few, h, w, 1.0, 1.0, None, None,
                                       ptr(w4), None, ptr(skip), WINO | nets.IN_B8, st)
    assert refused(rc, b"SLR_CONV_WINO"), (rc, L.slr_last_error())
    rc = L.slr_pconv3x3_forward_skipout(ptr(xb), None, None, ptr(mask), ptr(fbuf), 1.0, 1.0, ptr(bias), None, None, None, ptr(fout), ptr(um),
                                        1, cin, few, h, w, ptr(w4), ptr(skip), WINO | nets.IN_B8, st)
    assert refused(rc, b"SLR_CONV_WINO"), (rc, L.slr_last_error())
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(fout.any()) and not bool(skip.any()) and not bool(um.any())


def test_module_and_library_agree_on_the_weight_buffer(S):
    """nets.Conv's ``_wwino`` buffer is slr_conv3x3_wino_weights' output for its weights (the C-ABI runs above use either)."""
    nets, _lib = S.nets, S._lib
    d = wm.dense_inputs(wm.CASES[4])
    cout, cin = d["w"].shape[:2]
    own = wino_buffer(S, d["w"])
    buf = torch.zeros(_lib.lib().slr_conv3x3_wino_weight_bytes(cout, cin), dtype=torch.uint8, device=DEV)
    _lib.call("slr_conv3x3_wino_weights", buf.device, d["w"].cuda(), buf, cout, cin)
    assert own.numel() == buf.numel() == 192 * 32 * 16 * 4 and torch.equal(own, buf)
    u = wm.weights(d["w"], F32)                                      # and it holds U = G g G^T, rounded once: sorted values agree
    assert torch.equal(buf.view(torch.float32).cpu().sort().values, torch.cat([u.flatten(), torch.zeros(192 * 32 * 16 - u.numel())]).sort().values)
