"""Host-side checks of the generator's spectral normalisation (no GPU): the float64 definition of tests/spectral_f64.py against torch's
own spectral_norm and against the reference's blocks (tests/golden/spectral_train_vs_reference.npz), the plan fillers of
include/slr_splat.h decoded from the documented layouts, the refusals of the operators, the unfolded loader and its inverse, and
E_plain32 of the sigma list's inputs -- the figure the device bounds of tests/test_gpu_spectral.py are made of."""
import os
import re

import numpy as np
import pytest
import torch

import block_train_f64 as B64
import conv_train_f64 as C64
import nets_fixture as NF
import spectral_f64 as S64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spectral_train_vs_reference.npz")
P = 0x7F0000100000
ENTRIES = ("slr_spectral_plan_bytes", "slr_spectral_plan_fill", "slr_spectral_sigma", "slr_conv3x3_f32_weights_scaled",
           "slr_conv1x1_f32_weights_scaled", "slr_conv_prep_plan_bytes", "slr_conv_prep_plan_fill", "slr_conv_prep_scaled_multi",
           "slr_spectral_grad_ws_bytes", "slr_spectral_weight_grad")


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def _refused(L, rc, *words):
    msg = L.slr_last_error()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def test_entry_points_are_declared_and_abi_is_20(L):
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.ABI_VERSION >= 20 and L.slr_abi_version() == _lib.ABI_VERSION


# ------------------------------------------------------------------ the definition against torch

def _torch_spectral_grads(module, W, u, v, run):
    """d loss / d weight_orig by torch.autograd through torch.nn.utils.spectral_norm for two consecutive training forwards, the loss
    the sum of run(module) over both; returns (grad, [(u, v) after each forward])."""
    with torch.no_grad():
        module.weight.copy_(W)
    m = torch.nn.utils.spectral_norm(module)
    with torch.no_grad():
        m.weight_u.copy_(u)
        m.weight_v.copy_(v)
    m.train()
    loss, uvs = 0.0, []
    for k in range(2):
        loss = loss + run(m, k)
        uvs.append((m.weight_u.clone(), m.weight_v.clone()))
    loss.backward()
    return m.weight_orig.grad, uvs


def test_definition_gradient_is_autograd_through_torch_spectral_norm_conv():
    gen = torch.Generator().manual_seed(3)
    W = torch.randn(6, 5, 3, 3, generator=gen, dtype=torch.float64)
    u, v = S64.normal_uv(6, 45, gen)
    xs = [torch.randn(2, 5, 7, 6, generator=gen, dtype=torch.float64) for _ in range(2)]
    gs = [torch.randn(2, 6, 7, 6, generator=gen, dtype=torch.float64) for _ in range(2)]
    conv = torch.nn.Conv2d(5, 6, 3, padding=1, bias=False).double()
    ref, uvs = _torch_spectral_grads(conv, W, u, v, lambda m, k: (m(xs[k]) * gs[k]).sum())
    got = torch.zeros_like(W)
    for k in range(2):
        We, u, v, inv = S64.effective(W, u, v, training=True)
        assert C64.E(u, uvs[k][0]) < 1e-13 and C64.E(v, uvs[k][1]) < 1e-13
        got += S64.weight_orig_grad(C64.conv_dw(xs[k], gs[k]), W, u, v, inv)
    e = C64.E(got, ref)
    print(f"conv: definition vs autograd through spectral_norm: {e:.2e}")
    assert e < 1e-12


def test_definition_gradient_is_autograd_through_torch_spectral_norm_linear():
    gen = torch.Generator().manual_seed(4)
    W = torch.randn(9, 20, generator=gen, dtype=torch.float64)
    u, v = S64.normal_uv(9, 20, gen)
    xs = [torch.randn(3, 20, generator=gen, dtype=torch.float64) for _ in range(2)]
    gs = [torch.randn(3, 9, generator=gen, dtype=torch.float64) for _ in range(2)]
    lin = torch.nn.Linear(20, 9, bias=False).double()
    ref, _ = _torch_spectral_grads(lin, W, u, v, lambda m, k: (m(xs[k]) * gs[k]).sum())
    got = torch.zeros_like(W)
    for k in range(2):
        _, u, v, inv = S64.effective(W, u, v, training=True)
        got += S64.weight_orig_grad(gs[k].t() @ xs[k], W, u, v, inv)
    e = C64.E(got, ref)
    print(f"linear: definition vs autograd through spectral_norm: {e:.2e}")
    assert e < 1e-12


def test_eval_mode_of_the_definition_is_the_fold_of_the_loader():
    from slr_sfs_amd import nets
    W, u, v = S64.matrix_case(7, 18, 5)
    W4 = W.reshape(7, 2, 3, 3)
    We, u2, v2, _ = S64.effective(W4, u, v, training=False)
    assert torch.equal(u2, u) and torch.equal(v2, v)
    folded = nets._fold_sn({"c.weight_orig": W4, "c.weight_u": u, "c.weight_v": v}, "c")
    assert C64.E(We, folded) < 1e-14


def load_golden(path=GOLDEN):
    """{case: {key: float64 tensor or str}} of tests/golden/spectral_train_vs_reference.npz (float64 results in the packed form of
    decoder_train_f64.packed; inputs and parameters float32 values)."""
    g = np.load(path)
    flat = {}
    for k in g.files:
        if k.endswith("#hi"):
            flat[k[:-3]] = torch.from_numpy(g[k].astype(np.float64) + g[k[:-3] + "#lo"].astype(np.float64) * float(g[k[:-3] + "#scale"]))
        elif "#" not in k:
            flat[k] = str(g[k]) if g[k].dtype.kind == "U" else torch.from_numpy(g[k]).double()
    out = {}
    for k, v in flat.items():
        case, key = k.split("/", 1)
        out.setdefault(case, {})[key] = v
    return out


def golden_block(c):
    """(form, kind, p, uv) of a golden case."""
    p = {k[2:]: v for k, v in c.items() if k.startswith("p/")}
    p.setdefault("w_b", None)
    uv = {k: (c["u0/" + k], c["v0/" + k]) for k in S64.names_of(p)}
    return c["form"], c["kind"] or None, p, uv


def test_definition_reproduces_the_reference_blocks():
    """tests/golden/spectral_train_vs_reference.npz (tools/make_golden_spectral_train.py): the reference's own ResNet_Block_Pconv2 and
    ResNet_Block under norm_G = sync:spectral_batch in train() mode, float64, two forwards and the backward of the sum of both."""
    assert os.path.exists(GOLDEN), "tests/golden/spectral_train_vs_reference.npz is missing (tools/make_golden_spectral_train.py writes it)"
    cases = load_golden()
    assert sorted(cases) == ["pconv_down", "pconv_none", "pconv_up", "res_down", "res_none", "res_up"]
    worst = 0.0
    for case, c in sorted(cases.items()):
        form, kind, p, uv = golden_block(c)
        grads, w = None, 0.0
        for k in range(2):
            x, noise, gy = c[f"{k}/x"], (c[f"{k}/noise1"], c[f"{k}/noise2"]), c[f"{k}/gy"]
            mask = c[f"{k}/mask"] if form == "pconv" else None
            f, uv, ctx = S64.block(form, x, mask, p, uv, kind, noise, training=True)
            w = max(w, C64.E(f["y"], c[f"{k}/y"]))
            for name in uv:
                w = max(w, C64.E(uv[name][0], c[f"{k}/u/{name}"]), C64.E(uv[name][1], c[f"{k}/v/{name}"]))
            d = S64.block_grads(form, x, mask, p, uv, kind, noise, gy, ctx)
            w = max(w, C64.E(d["dx"], c[f"{k}/dx"]))
            one = {name: d["d_" + name] for name in S64.names_of(p)}
            one.update({b: d["d" + b] for b in ("b_aa", "b_ab", "b_b") if p.get(b) is not None})
            grads = one if grads is None else {n: grads[n] + one[n] for n in one}
            aa_terms = d["db_aa_terms"] if k == 0 else aa_terms + d["db_aa_terms"]
        refs = {k[2:]: v for k, v in c.items() if k.startswith("d/")}
        assert sorted(refs) == sorted(grads)
        for name, ref in refs.items():               # db_aa: a batch-statistics BN follows, it cancels to rounding (block_train_f64.E_terms)
            w = max(w, B64.E_terms(grads[name], ref, aa_terms) if name == "b_aa" else C64.E(grads[name], ref))
        print(f"{case}: definition vs the reference: worst E {w:.2e}")
        worst = max(worst, w)
    assert worst <= 1e-10


# ------------------------------------------------------------------ E_plain32 of the sigma list (the device bounds' input)

SIGMA_SHAPES = ((3, 20), (64, 20), (3, 27), (65, 576), (16, 8), (128, 1152), (256, 2304))


def sigma_reference(training):
    """Per shape: (u64, v64, inv64) and E_plain32 of each, the definition evaluated by torch in float32 on the same inputs."""
    out = []
    for i, (r, c) in enumerate(SIGMA_SHAPES):
        W, u, v = S64.matrix_case(r, c, 100 + i)
        _, u64, v64, i64 = S64.effective(W, u, v, training)
        _, u32, v32, i32 = S64.effective(W.float(), u.float(), v.float(), training)
        out.append(dict(ref=(u64, v64, i64), plain=(C64.E(u32, u64), C64.E(v32, v64), abs(float(i32) - float(i64)) / abs(float(i64)))))
    return out


@pytest.mark.parametrize("training", (True, False))
def test_plain_float32_error_of_the_sigma_list_inputs(training):
    for (r, c), e in zip(SIGMA_SHAPES, sigma_reference(training)):
        print(f"[{r},{c}] training={training}: E_plain32 u {e['plain'][0]:.2e} v {e['plain'][1]:.2e} inv_sigma {e['plain'][2]:.2e}")
        assert all(np.isfinite(x) and x < 1e-5 for x in e["plain"])
        if not training:
            assert e["plain"][0] == 0.0 and e["plain"][1] == 0.0


# ------------------------------------------------------------------ the plans, decoded from the documented layouts

def test_spectral_plan_layout_is_the_documented_one(L):
    rows = np.array([3, 64, 256, 16, 128, 31], dtype=np.int32)
    cols = np.array([20, 20, 2304, 8, 1152, 3000], dtype=np.int32)
    n = len(rows)
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    band, split = (int(re.search(rf"{k}\s+(\d+)", hdr).group(1)) for k in ("SLR_SPECTRAL_BAND_ROWS", "SLR_SPECTRAL_SPLIT_ELEMENTS"))
    bands = [(-(-r // band) if r * c >= split and r >= 2 * band else 0) for r, c in zip(rows, cols)]
    assert bands == [0, 0, 16, 0, 8, 0]                                       # ([31, 3000] is large but has fewer than two bands)
    al = lambda v, a: (v + a - 1) // a * a                                    # noqa: E731
    n_work = sum(bands)
    work_off = al(64 + 64 * n, 16)
    scratch_off = al(work_off + 8 * n_work, 256)
    sizes = [al(8 * (b * int(c) + int(r)), 256) if b else 0 for b, r, c in zip(bands, rows, cols)]
    addr = np.empty((3, n), dtype=np.uint64)
    for k in range(3):
        addr[k] = P + (k << 36) + 4 * np.arange(n, dtype=np.uint64) * 4099
    need = L.slr_spectral_plan_bytes(n, rows.ctypes.data, cols.ctypes.data)
    assert need == al(scratch_off + sum(sizes), 256)
    assert L.slr_spectral_plan_bytes(0, rows.ctypes.data, cols.ctypes.data) == 0 and L.slr_spectral_plan_bytes(n, None, cols.ctypes.data) == 0
    buf = np.full(need + 64, 0xAB, dtype=np.uint8)
    fill = lambda **kw: L.slr_spectral_plan_fill(kw.get("buf", buf.ctypes.data), kw.get("bytes", need), kw.get("n", n),      # noqa: E731
                                                 *(kw.get("a%d" % k, addr[k].ctypes.data) for k in range(3)),
                                                 kw.get("rows", rows.ctypes.data), kw.get("cols", cols.ctypes.data))
    assert fill() == 0, L.slr_last_error()
    assert (buf[need:] == 0xAB).all(), "written behind the plan"
    magic, maxdim, nn_, nw = buf[:16].view(np.uint32)
    assert int(magic) == int(re.search(r"SLR_SPECTRAL_PLAN_MAGIC\s+0x([0-9a-f]+)u", hdr).group(1), 16) == 0x43455053
    assert int(maxdim) == int(re.search(r"SLR_SPECTRAL_MAX_DIM\s+(\d+)", hdr).group(1)) and int(nn_) == n and int(nw) == n_work
    toff, nbytes, tu, tv, woff, soff = (int(x) for x in buf[16:64].view(np.uint64))
    assert (toff, nbytes, tu, tv, woff, soff) == (64, need, rows.sum(), cols.sum(), work_off, scratch_off)
    rec = buf[64:64 + 64 * n]
    r64, r32 = rec.view(np.uint64).reshape(n, 8), rec.view(np.int32).reshape(n, 16)
    at = scratch_off
    for t in range(n):
        assert [int(x) for x in r64[t, :3]] == [int(addr[k, t]) for k in range(3)]
        assert list(r32[t, 6:10]) == [rows[t], cols[t], t, bands[t]]
        assert int(r64[t, 5]) == rows[:t].sum() and int(r64[t, 6]) == cols[:t].sum()
        assert int(r64[t, 7]) == (at if bands[t] else 0)
        at += sizes[t]
    assert not buf[64 + 64 * n:work_off].any()
    work = buf[work_off:work_off + 8 * n_work].view(np.int32).reshape(n_work, 2)
    assert [tuple(int(x) for x in w) for w in work] == [(t, b) for t in range(n) for b in range(bands[t])]
    assert not buf[work_off + 8 * n_work:scratch_off].any()
    _refused(L, fill(bytes=need - 1), b"slr_spectral_plan_fill", b"bytes")
    _refused(L, fill(n=0), b"slr_spectral_plan_fill", b"n ")
    for k in ("buf", "a0", "a1", "a2", "rows", "cols"):
        _refused(L, fill(**{k: None}), b"slr_spectral_plan_fill", b"null")
    big = rows.copy()
    big[2] = 3073
    _refused(L, fill(rows=big.ctypes.data), b"slr_spectral_plan_fill", b"rows")
    assert L.slr_spectral_plan_bytes(n, big.ctypes.data, cols.ctypes.data) == 0
    odd = addr[1].copy()
    odd[2] += 2
    _refused(L, fill(a1=odd.ctypes.data), b"slr_spectral_plan_fill", b"aligned")


def test_prep_plan_covers_every_buffer_element_once(L):
    cout = np.array([3, 3, 65, 65, 16, 16, 128], dtype=np.int32)
    cin = np.array([8, 8, 64, 64, 8, 8, 64], dtype=np.int32)
    taps = np.array([9, 9, 9, 9, 1, 1, 9], dtype=np.int32)
    bwd = np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.int32)
    slot = np.array([0, 0, 1, 1, 2, 2, 5], dtype=np.int32)
    n = len(cout)
    w = (P + 4096 * np.arange(n)).astype(np.uint64)
    wf = (P + (1 << 30) + (1 << 22) * np.arange(n)).astype(np.uint64)
    shape = [a.ctypes.data for a in (cout, cin, taps, bwd)]
    need = L.slr_conv_prep_plan_bytes(n, *shape)
    buf = np.full(need + 64, 0xAB, dtype=np.uint8)
    assert L.slr_conv_prep_plan_fill(buf.ctypes.data, need, n, w.ctypes.data, wf.ctypes.data, slot.ctypes.data, *shape) == 0, L.slr_last_error()
    assert (buf[need:] == 0xAB).all()
    magic, chunk, nn_, n_work = (int(x) for x in buf[:16].view(np.uint32))
    toff, woff, nbytes = (int(x) for x in buf[16:40].view(np.uint64))
    assert magic == 0x50455250 and chunk == 4096 and nn_ == n and toff == 64 and woff == (64 + 48 * n + 15) // 16 * 16
    assert nbytes == need == (woff + 8 * n_work + 255) // 256 * 256 and not buf[40:64].any()
    rec = buf[64:64 + 48 * n]
    r64, r32 = rec.view(np.uint64).reshape(n, 6), rec.view(np.int32).reshape(n, 12)
    work = buf[woff:woff + 8 * n_work].view(np.int32).reshape(n_work, 2)
    for t in range(n):
        co, ci = (cin[t], cout[t]) if bwd[t] else (cout[t], cin[t])
        few = int(taps[t] == 9 and co <= 4)
        nbytes_buf = (L.slr_conv3x3_weight_bytes if taps[t] == 9 else L.slr_conv1x1_weight_bytes)(int(co), int(ci))
        slot_, co_, ci_, cip, taps_, bwd_, few_, total = (int(x) for x in r32[t, 4:12])
        assert (int(r64[t, 0]), int(r64[t, 1])) == (int(w[t]), int(wf[t]))
        assert (slot_, co_, ci_, cip, taps_, bwd_, few_) == (slot[t], co, ci, (ci + 15) // 16 * 16, taps[t], bwd[t], few)
        assert 0 < total * 4 <= nbytes_buf, "the elements of a plan's tensor lie inside its buffer"
        if not few:
            assert total * 4 == nbytes_buf
        starts = sorted(int(s) for tt, s in work if tt == t)
        assert starts == list(range(0, total, chunk))
    _refused(L, L.slr_conv_prep_plan_fill(buf.ctypes.data, need - 1, n, w.ctypes.data, wf.ctypes.data, slot.ctypes.data, *shape),
             b"slr_conv_prep_plan_fill", b"bytes")
    bad = taps.copy()
    bad[0] = 4
    assert L.slr_conv_prep_plan_bytes(n, cout.ctypes.data, cin.ctypes.data, bad.ctypes.data, bwd.ctypes.data) == 0


def test_entry_points_refuse_bad_arguments_before_anything_is_launched(L):
    _refused(L, L.slr_spectral_sigma(None, 1, 0, P, P, P, 1, None), b"slr_spectral_sigma", b"null")
    _refused(L, L.slr_spectral_sigma(P, 0, 0, P, P, P, 1, None), b"slr_spectral_sigma", b"n_tensors")
    _refused(L, L.slr_spectral_sigma(P, 1, -1, P, P, P, 1, None), b"slr_spectral_sigma", b"n_work")
    _refused(L, L.slr_spectral_sigma(P + 8, 1, 0, P, P, P, 1, None), b"slr_spectral_sigma", b"aligned")
    _refused(L, L.slr_conv3x3_f32_weights_scaled(P, None, P, 8, 8, 0, None), b"scale")
    _refused(L, L.slr_conv1x1_f32_weights_scaled(P, P, P, 0, 8, 0, None), b"sizes")
    _refused(L, L.slr_conv_prep_scaled_multi(P, 1, 0, P, None), b"slr_conv_prep_scaled_multi", b"n_work")
    assert L.slr_spectral_grad_ws_bytes(256, 2304) == (8 * 144 + 255) // 256 * 256 and L.slr_spectral_grad_ws_bytes(0, 5) == 0
    _refused(L, L.slr_spectral_weight_grad(P, P, P, P, None, P, 4, 4, P, 256, None), b"slr_spectral_weight_grad", b"null")
    _refused(L, L.slr_spectral_weight_grad(P, P, P, P, P, P, 0, 4, P, 256, None), b"slr_spectral_weight_grad", b"rows")
    assert L.slr_spectral_weight_grad(P, P, P, P, P, P, 4, 4, P, 8, None) == -2


# ------------------------------------------------------------------ the Python layer without a device

def test_operators_refuse_bad_spectral_arguments_without_a_device():
    """CPU tensors, wrong dtypes, non-contiguous tensors and u / v of the wrong length raise before anything touches the device: the
    checks run on CPU tensors here, in the order type / device / dtype / shape / layout of the operators' other arguments."""
    import slr_sfs_amd as S
    w = torch.zeros(6, 4, 3, 3)
    scale, u, v = torch.ones(1), torch.zeros(6), torch.zeros(36)
    with pytest.raises(NotImplementedError):
        S.spectral.check_spectral("conv3x3", w, scale, (u, v))
    with pytest.raises(NotImplementedError):
        S.conv3x3(torch.zeros(1, 4, 5, 5), w, weight_scale=scale, spectral=(u, v))
    with pytest.raises(NotImplementedError):
        S.spectral_weight_grad(w, w, u, v, scale)
    with pytest.raises(ValueError):
        S.spectral.check_spectral("conv3x3", w, None, (u, v))
    with pytest.raises(TypeError):
        S.spectral.check_spectral("conv3x3", w, 1.0, None)
    # beyond the device check: the same function on tensors that claim to be on a device

    class _Dev(torch.Tensor):
        is_cuda = True
    on = lambda t: t.as_subclass(_Dev)                                                    # noqa: E731
    ok = (on(w), on(scale), (on(u), on(v)))
    S.spectral.check_spectral("conv3x3", *ok)
    with pytest.raises(TypeError):
        S.spectral.check_spectral("conv3x3", on(w), on(scale.double()), None)
    with pytest.raises(ValueError):
        S.spectral.check_spectral("conv3x3", on(w), on(torch.ones(2)), None)
    with pytest.raises(ValueError):
        S.spectral.check_spectral("conv3x3", on(w), on(scale), (on(torch.zeros(5)), on(v)))
    with pytest.raises(ValueError):
        S.spectral.check_spectral("conv3x3", on(w), on(scale), (on(u), on(torch.zeros(37))))
    with pytest.raises(TypeError):
        S.spectral.check_spectral("conv3x3", on(w), on(scale), (on(u.double()), on(v)))
    with pytest.raises(ValueError):
        S.spectral.check_spectral("conv3x3", on(w), on(scale), (on(u), on(torch.zeros(72)[::2])))
    with pytest.raises(TypeError):
        S.spectral.check_spectral("conv3x3", on(w), on(scale), (on(u),))
    # the list forms and the group run the same refusals before they build a plan
    for bad in (dict(ws=[on(w.double())]), dict(us=[on(torch.zeros(5))]), dict(vs=[on(torch.zeros(37))]), dict(us=[on(u.double())]),
                dict(ws=[on(torch.zeros(6, 8, 3, 3)[:, ::2])]), dict(vs=[on(torch.zeros(72)[::2])]), dict(ws=[on(torch.zeros(6))]), dict(us=[])):
        kw = dict(ws=[on(w)], us=[on(u)], vs=[on(v)])
        kw.update(bad)
        with pytest.raises((TypeError, ValueError)):
            S.spectral_sigma(kw["ws"], kw["us"], kw["vs"])
    with pytest.raises(NotImplementedError):
        S.spectral_sigma([w], [u], [v])
    for ws, sc, slots in (([on(w.double())], on(torch.ones(2)), None), ([on(torch.zeros(6, 4, 2, 2))], on(torch.ones(2)), None),
                          ([on(w)], on(torch.ones(2).double()), None), ([on(w)], on(torch.ones(2)), [2]), ([on(w)], on(torch.ones(2)), [0, 1]),
                          ([on(torch.zeros(6, 8, 3, 3)[:, ::2])], on(torch.ones(2)), None), ([], on(torch.ones(2)), None)):
        with pytest.raises((TypeError, ValueError)):
            S.prepare_scaled(ws, sc, slots)
    with pytest.raises(NotImplementedError):
        S.prepare_scaled([w], scale)
    conv = S.TrainableConv3x3(4, 6, spectral=True)
    with pytest.raises(NotImplementedError):
        S.SpectralGroup([conv]).run()
    for name, value in (("weight_u", torch.zeros(5)), ("weight_v", torch.zeros(36).double()), ("weight_v", torch.zeros(72)[::2])):
        conv = S.TrainableConv3x3(4, 6, spectral=True)
        conv._parameters["weight_orig"] = on(conv.weight_orig.detach())
        conv._buffers["weight_u"], conv._buffers["weight_v"] = on(conv.weight_u), on(conv.weight_v)
        conv._buffers[name] = on(value)
        with pytest.raises((TypeError, ValueError)):
            S.SpectralGroup([conv]).run()
    with pytest.raises(ValueError):
        S.SpectralGroup([torch.nn.Conv2d(3, 3, 3)]).run()


def test_spectral_modules_have_torchs_parametrisation():
    import slr_sfs_amd as S
    T = S.trainable
    for m, shape in ((T.TrainableConv3x3(4, 6, spectral=True), (6, 36)), (T.TrainablePartialConv3x3(4, 6, spectral=True), (6, 36)),
                     (T.TrainableConv1x1(4, 6, spectral=True), (6, 4)), (S.SpectralLinear(20, 6), (6, 20))):
        names = dict(m.named_parameters())
        assert "weight_orig" in names and "weight" not in names and names["weight_orig"].requires_grad
        bufs = dict(m.named_buffers())
        assert tuple(bufs["weight_u"].shape) == (shape[0],) and tuple(bufs["weight_v"].shape) == (shape[1],)
        assert abs(float(bufs["weight_u"].norm()) - 1) < 1e-5 and abs(float(bufs["weight_v"].norm()) - 1) < 1e-5
        assert not hasattr(m, "weight")
    bn = T.TrainableNoiseBN(6, spectral=True)
    assert {"gain.weight_orig", "gain.weight_u", "gain.weight_v", "bias.weight_orig", "stored_mean"} <= set(bn.state_dict())
    plain = T.TrainablePconvResBlock(4, 6)
    assert set(plain.state_dict()) == {"bn1.stored_mean", "bn1.stored_var", "bn1.gain.weight", "bn1.bias.weight", "bn2.stored_mean",
                                       "bn2.stored_var", "bn2.gain.weight", "bn2.bias.weight", "conv_aa.weight", "conv_aa.bias",
                                       "conv_ab.weight", "conv_ab.bias", "conv_b.weight"}
    g = S.SpectralGroup([T.TrainablePconvResBlock(4, 6, spectral=True)])
    assert len(g.leaves) == 7 and len(g.convs) == 3 and g.total_u == 4 + 4 + 6 + 6 + 6 + 6 + 6


def _nets(S, spectral):
    T = S.trainable
    ud = [None, "Down", "Up", None]
    return {"model.module.projector.": T.TrainableDecoderPconv2(8, 3, widths=[16, 8, 8], updown=ud, spectral=spectral),
            "model.module.encoder.": T.TrainableEncoderWithZ(3, 8, widths=[8, 16, 8], updown=[None] * 4, spectral=spectral),
            "model.module.net_bg.": T.TrainableBGDecoder(3, 3, widths=[8, 16, 8], updown=ud, spectral=spectral)}


def test_loader_is_strict_and_reference_state_dict_is_its_inverse():
    import slr_sfs_amd as S
    torch.manual_seed(0)
    src, dst = _nets(S, True), _nets(S, True)
    for prefix, net in src.items():
        for b in net.buffers():                                                          # (fresh statistics are 0 / 1: make them tell)
            if b.dim() == 1 and b.shape[0] > 0 and "stored" in "".join(n for n, t in net.named_buffers() if t is b):
                b.add_(torch.rand_like(b))
        sd = S.reference_state_dict(net, prefix)
        assert all(k.startswith(prefix) for k in sd)
        blocks = "eblocks" if not prefix.endswith("encoder.") else "gblocks"
        first = "conv_aa" if prefix.endswith("projector.") else "ch_a.2"
        for suffix in ("weight_orig", "weight_u", "weight_v", "bias"):
            assert f"{prefix}{blocks}.0.{first}.{suffix}" in sd
        noise = "bn_noise1" if prefix.endswith("projector.") else "ch_a.0"
        stats = "pbn" if prefix.endswith("projector.") else "bn"
        assert {f"{prefix}{blocks}.1.{noise}.gain.weight_orig", f"{prefix}{blocks}.1.{noise}.bias.weight_v",
                f"{prefix}{blocks}.1.{noise}.{stats}.stored_var"} <= set(sd)
        assert not any(k.endswith(".weight") for k in sd)
        other = {"model.module.other.x": torch.zeros(1)}
        S.load_spectral_state_dict(dst[prefix], {**sd, **other}, prefix)
        back = S.reference_state_dict(dst[prefix], prefix)
        assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
        assert len(sd) == sum(1 for _ in net.parameters()) + sum(1 for _ in net.buffers())
        # strict in both directions, and nothing is written when it refuses
        before = {k: t.clone() for k, t in back.items()}
        k0 = sorted(sd)[0]
        with pytest.raises(KeyError):
            S.load_spectral_state_dict(dst[prefix], {k: v + 1 for k, v in sd.items() if k != k0}, prefix)
        with pytest.raises(KeyError):
            S.load_spectral_state_dict(dst[prefix], {**{k: v + 1 for k, v in sd.items()}, prefix + "eblocks.0.extra": torch.zeros(1)}, prefix)
        with pytest.raises(ValueError):
            S.load_spectral_state_dict(dst[prefix], {k: (v + 1 if k != k0 else torch.zeros(v.numel() + 1)) for k, v in sd.items()}, prefix)
        after = S.reference_state_dict(dst[prefix], prefix)
        assert all(torch.equal(after[k], before[k]) for k in before)
    with pytest.raises(ValueError):
        S.reference_state_dict(_nets(S, False)["model.module.encoder."], "")


RECORDED = {"encoder_with_z": lambda T, sn: T.TrainableEncoderWithZ(spectral=sn), "decoder_holes": lambda T, sn: T.TrainableDecoderPconv2(64, 3, spectral=sn),
            "net_bg": lambda T, sn: T.TrainableBGDecoder(spectral=sn), "alpha_encoder": lambda T, sn: T.TrainableEncoder(3, 2, spectral=sn),
            "alpha_decoder": lambda T, sn: T.TrainableDecoderPconv2(65, 1, spectral=sn)}


def recorded_state_dict(case):
    """A state dict with the reference's OWN key and shape list for ``case`` (recorded from its modules under sync:spectral_batch in
    tests/golden/nets_vs_reference.npz; tensors regenerated by tests/nets_fixture.py) and the case's prefix."""
    ref = np.load(os.path.join(ROOT, "tests", "golden", "nets_vs_reference.npz"))
    prefix = NF.VS_REFERENCE[case][3]
    keys = [str(k) for k in ref[f"{case}_keys"]]
    return {prefix + k: v for k, v in NF.state_dict("vs_reference/" + case, keys, ref[f"{case}_shapes"]).items()}, prefix


@pytest.mark.parametrize("case", sorted(RECORDED))
def test_loader_takes_the_references_own_key_lists_and_the_inverse_returns_them(case):
    """Independent of reference_state_dict: the key lists were recorded from the reference's modules.  Every key is consumed (the BN
    layers' accumulation_counter and the conv_b that ResNet_Block_Pconv2 builds but does not call included), the inverse returns exactly
    that key set with the same tensors, and the folded loader's weights are the eval-mode effective weights of what was loaded."""
    import slr_sfs_amd as S
    sd, prefix = recorded_state_dict(case)
    assert any(k.endswith("accumulation_counter") for k in sd)
    net = S.load_spectral_state_dict(RECORDED[case](S.trainable, True), sd, prefix)
    back = S.reference_state_dict(net, prefix)
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert back[k].shape == v.shape and torch.equal(back[k], v), k
    assert len(back) == sum(1 for _ in net.parameters()) + sum(1 for _ in net.buffers())
    if "decoder" in case:
        unused = [k for k in sd if ".conv_b." in k and k.rsplit(".conv_b.", 1)[0] + ".conv_b.weight_orig" in sd]
        assert sum(1 for b in net.blocks if b.conv_b is None) == sum(1 for b in net.blocks if getattr(b, "conv_b_unused", None) is not None) > 0
        assert len(unused) == 3 * len(net.blocks)
    folded = S.nets.load_reference_state_dict(RECORDED[case](S.trainable, False), sd, prefix)
    for bs, bf in zip(net.blocks, folded.blocks):
        for name in ("conv_aa", "conv_ab", "conv_b"):
            cs, cf = getattr(bs, name), getattr(bf, name)
            assert (cs is None) == (cf is None)
            if cs is not None:
                We = S64.effective(cs.weight_orig.detach().double(), cs.weight_u.double(), cs.weight_v.double(), training=False)[0]
                assert C64.E(cf.weight, We) < 1e-6
    with pytest.raises(KeyError):                        # a counter that is missing is missing
        S.load_spectral_state_dict(net, {k: v for k, v in sd.items() if not k.endswith("0.bn.accumulation_counter") and not k.endswith("noise1.pbn.accumulation_counter")}, prefix)


def test_folding_loader_is_unchanged_and_agrees_with_the_unfolded_one_in_eval():
    """nets.load_reference_state_dict folds the same synthetic reference state dict into a spectral=False network: its weights are the
    definition's eval-mode effective weights of the spectral=True network's tensors."""
    import slr_sfs_amd as S
    torch.manual_seed(1)
    for prefix, net in _nets(S, True).items():
        sd = S.reference_state_dict(S64.settle(net), prefix)
        folded = S.nets.load_reference_state_dict(_nets(S, False)[prefix], sd, prefix)
        for bs, bf in zip(net.blocks, folded.blocks):
            for name in ("conv_aa", "conv_ab", "conv_b"):
                cs, cf = getattr(bs, name), getattr(bf, name)
                if cs is None:
                    continue
                We, _, _, _ = S64.effective(cs.weight_orig.detach().double(), cs.weight_u.double(), cs.weight_v.double(), training=False)
                assert C64.E(cf.weight, We) < 1e-6
            for bn_s, bn_f in ((bs.bn1, bf.bn1), (bs.bn2, bf.bn2)):
                We, _, _, _ = S64.effective(bn_s.gain.weight_orig.detach().double(), bn_s.gain.weight_u.double(), bn_s.gain.weight_v.double(), False)
                assert C64.E(bn_f.gain.weight, We) < 1e-6
