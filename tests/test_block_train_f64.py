"""CPU checks of the trainable decoder block's yardstick (tests/block_train_f64.py): its written-out backward formulas against torch's
float64 autograd of its written-out forward, its resamplers against F.avg_pool2d / F.interpolate / F.max_pool2d, and the block against
the reference's own ResNet_Block_Pconv2 in train() mode (tests/golden/block_train_vs_reference.npz, made by
tools/make_golden_block_train.py); then what the new entry points decide on the host (no device is touched: the pointers are dummy
integers)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_train_f64 as B64
import conv_train_f64 as C64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "block_train_vs_reference.npz")


def _close(name, got, ref, tol, terms=None):
    e = C64.E(got, ref) if terms is None else B64.E_terms(got, ref, terms)
    print(f"{name}: {e:.2e}")
    assert e <= tol, (name, e)


def _bn_case(masked, seed=3):
    N, C, H, W = 2, 6, 9, 7
    mask = C64.holed_mask(N, H, W, seed) if masked else None
    x, gain, bias, ga = (t.double() for t in B64.bn_inputs(N, C, H, W, seed, mask))
    mask = mask.double() if masked else None
    return x, mask, gain, bias, ga


@pytest.mark.parametrize("stored", [False, True], ids=["batch", "stored"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "partial"])
def test_bn_backward_formulas_are_float64_autograd(masked, stored):
    x, mask, gain, bias, ga = _bn_case(masked)
    st = (torch.linspace(-1, 1, 6, dtype=torch.float64), torch.linspace(0.5, 2, 6, dtype=torch.float64)) if stored else None
    addend = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    xa, ga_, ba = (t.clone().requires_grad_(True) for t in (x, gain, bias))
    a = B64.bn_train(xa, mask, ga_, ba, stored=st)[0]
    dx, dgain, dbias = torch.autograd.grad(a, (xa, ga_, ba), ga)
    got = B64.bn_train_grads(x, mask, gain, bias, ga, stored=st, addend=addend)
    _close("dx", got[0], dx + addend, 1e-12)
    _close("dgain", got[1], dgain, 1e-12)
    _close("dbias", got[2], dbias, 1e-12)


def test_bn_definition_is_the_reference_formula():
    """partial_manual_bn / manual_bn + partial_fused_bn (normalization.py:236-253, 319-354) as torch ops."""
    for masked in (False, True):
        x, mask, gain, bias, _ = _bn_case(masked)
        if masked:
            cnt = torch.sum(mask.expand_as(x), [0, 2, 3], keepdim=True) + 1e-5
            m, m2 = torch.sum(x, [0, 2, 3], keepdim=True) / cnt, torch.sum(x ** 2, [0, 2, 3], keepdim=True) / cnt
        else:
            m, m2 = torch.mean(x, [0, 2, 3], keepdim=True), torch.mean(x ** 2, [0, 2, 3], keepdim=True)
        var = m2 - m ** 2
        scale = torch.rsqrt(var + 1e-5) * gain[:, :, None, None]
        ref = torch.relu(x * scale - (m * scale - bias[:, :, None, None]))
        a, mean, v = B64.bn_train(x, mask, gain, bias)
        _close("a", a, ref if mask is None else ref * mask, 1e-13)
        _close("mean", mean, m.flatten(), 1e-13)
        _close("var", v, var.flatten(), 1e-12)


@pytest.mark.parametrize("hw", [(5, 7), (33, 20), (16, 24), (1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_resamplers_are_torch(hw):
    H, W = hw
    gen = torch.Generator().manual_seed(H * W)
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=gen)
    m = C64.holed_mask(2, H, W, seed=H).double()
    for kind, ref, mref in (("Down", lambda t: F.avg_pool2d(t, 3, stride=2, padding=1), lambda t: F.max_pool2d(t, 3, stride=2, padding=1)),
                            ("Up", lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False),
                             lambda t: F.interpolate(t, scale_factor=2, mode="nearest"))):
        xa = x.clone().requires_grad_(True)
        out = ref(xa)
        g = torch.randn(out.shape, dtype=torch.float64, generator=gen)
        _close(f"{kind} forward", B64.resample(x, kind), out, 1e-13)
        _close(f"{kind} adjoint", B64.resample_adjoint(g, kind, H, W), torch.autograd.grad(out, xa, g)[0], 1e-13)
        assert torch.equal(B64.resample_mask(m, kind), mref(m))


def test_conv1x1_formulas_are_float64_autograd():
    gen = torch.Generator().manual_seed(5)
    x, w, b = (torch.randn(*s, dtype=torch.float64, generator=gen) for s in ((2, 5, 6, 7), (4, 5, 1, 1), (4,)))
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = F.conv2d(xa, wa, b)
    g = torch.randn(out.shape, dtype=torch.float64, generator=gen)
    dx, dw = torch.autograd.grad(out, (xa, wa), g)
    _close("out", B64.conv1x1(x, w, b), out, 1e-13)
    _close("dx", B64.conv1x1_dx(g, w), dx, 1e-13)
    _close("dw", B64.conv1x1_dw(x, g), dw, 1e-13)


def _golden(name):
    z = np.load(GOLDEN)
    c = {k.split("/", 1)[1]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith(name + "/")}
    p = dict(w_aa=c["p_conv_aa.weight"], b_aa=c["p_conv_aa.bias"], w_ab=c["p_conv_ab.weight"], b_ab=c["p_conv_ab.bias"],
             w_b=c.get("p_conv_b.weight"))
    return c, p


@pytest.mark.parametrize("name,kind", [("none", None), ("down", "Down"), ("up", "Up")])
def test_block_definition_is_the_reference_block(name, kind):
    """Forward, stored statistics after one step and every gradient of the reference's block in train() mode, float64, to 1e-10."""
    c, p = _golden(name)
    gains, biases = (c["gain1"], c["gain2"]), (c["bias1"], c["bias2"])
    f = B64.block(c["x"], c["mask"], p, kind, gains, biases)
    _close("y", f["y"], c["y"], 1e-10)
    assert torch.equal(f["um"], c["um"])
    for i in (1, 2):                                     # stored = 0.9 * (0 | 1) + 0.1 * batch (normalization.py:294-300)
        _close(f"stored_mean{i}", 0.1 * f[f"mean{i}"], c[f"stored_mean{i}"], 1e-10)
        _close(f"stored_var{i}", 0.9 + 0.1 * f[f"var{i}"], c[f"stored_var{i}"], 1e-10)
    d = B64.block_grads(c["x"], c["mask"], p, kind, gains, biases, c["g"])
    _close("dx", d["dx"], c["dx"], 1e-10)
    for k in ("aa", "ab"):
        _close(f"dw_{k}", d[f"dw_{k}"], c[f"d_conv_{k}.weight"], 1e-10)
        _close(f"db_{k}", d[f"db_{k}"], c[f"d_conv_{k}.bias"], 1e-10, d["db_aa_terms"] if k == "aa" else None)      # (B64.E_terms)
    _close("dw_b", d["dw_b"], c["d_conv_b.weight"], 1e-10)
    for i in (1, 2):                                     # gain = 1 + noise W_g^T, bias = noise W_b^T: dW = d(table)^T noise
        _close(f"gain{i}", 1.0 + c[f"noise{i}"] @ c[f"p_bn_noise{i}.gain.weight"].t(), c[f"gain{i}"], 1e-12)
        _close(f"d gain{i}.weight", d[f"dgain{i}"].t() @ c[f"noise{i}"], c[f"d_bn_noise{i}.gain.weight"], 1e-10)
        _close(f"d bias{i}.weight", d[f"dbias{i}"].t() @ c[f"noise{i}"], c[f"d_bn_noise{i}.bias.weight"], 1e-10)


@pytest.mark.parametrize("kind", [None, "Down", "Up"])
@pytest.mark.parametrize("stored", [False, True], ids=["train", "eval"])
def test_block_backward_formulas_are_float64_autograd(kind, stored):
    """Also the identity skip (16 -> 16 without resampling), which the reference fixture does not hold."""
    N, cin, cout, H, W = 2, 16, (16 if kind is None else 12), 9, 8
    gen = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)       # noqa: E731
    mask = C64.holed_mask(N, H, W, seed=4)
    x = B64.bn_inputs(N, cin, H, W, 7, mask)[0].double()
    mask = mask.double()
    p = dict(w_aa=r(cout, cin, 3, 3) / 12, b_aa=r(cout) / 3, w_ab=r(cout, cout, 3, 3) / 12, b_ab=r(cout) / 3,
             w_b=None if kind is None else r(cout, cin, 1, 1) / 4)
    gains, biases = [1 + 0.3 * r(N, cin), 1 + 0.3 * r(N, cout)], [0.5 * r(N, cin), 0.5 * r(N, cout)]
    st = ((r(cin), 0.5 + r(cin).abs()), (r(cout) / 3, 0.5 + r(cout).abs())) if stored else None
    leaves = [x] + [p[k] for k in ("w_aa", "b_aa", "w_ab", "b_ab")] + gains + biases + ([] if p["w_b"] is None else [p["w_b"]])
    la = [t.clone().requires_grad_(True) for t in leaves]
    pa = dict(w_aa=la[1], b_aa=la[2], w_ab=la[3], b_ab=la[4], w_b=la[9] if p["w_b"] is not None else None)
    y = B64.block(la[0], mask, pa, kind, la[5:7], la[7:9], stored=st)["y"]
    g = r(*y.shape)
    ref = torch.autograd.grad(y, la, g)
    d = B64.block_grads(x, mask, p, kind, gains, biases, g, stored=st)
    names = ["dx", "dw_aa", "db_aa", "dw_ab", "db_ab", "dgain1", "dgain2", "dbias1", "dbias2"] + ([] if p["w_b"] is None else ["dw_b"])
    for nme, rf in zip(names, ref):
        _close(nme, d[nme], rf, 1e-12, d["db_aa_terms"] if nme == "db_aa" and not stored else None)                 # (B64.E_terms)


# ------------------------------------------------------------------ the host side of the entry points

@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def test_workspace_sizes(L):
    al = lambda v: (v + 255) & ~255                                          # noqa: E731
    assert L.slr_bn_train_ws_bytes(2, 64, 37, 51) == al(2 * 64 * 8 * 2 * 8) + al(2 * 8 * 8) + al(2 * 64 * 4)
    assert L.slr_bn_train_ws_bytes(0, 64, 4, 4) == 0 and L.slr_bn_train_ws_bytes(1024, 64, 4, 4) == 0
    # 64 -> 128 on 2 x 256 x 256: one channel tile, 4096 chunks; 256 slots, 8 MiB / 32 KiB = 256 slabs
    assert L.slr_conv1x1_grad_ws_bytes(2, 64, 128, 256, 256, 0) == 256 * 128 * 64 * 4
    # 256 -> 256 on 2 x 64 x 64: 4 x 2 tiles -> 32 slabs
    assert L.slr_conv1x1_grad_ws_bytes(2, 256, 256, 64, 64, 0) == 32 * 256 * 256 * 4
    assert L.slr_conv1x1_grad_ws_bytes(1, 8, 3, 5, 7, 0) == al(2 * 3 * 8 * 4)        # 35 pixels: two chunks
    assert L.slr_conv1x1_grad_ws_bytes(1, 8, 3, 5, 7, 9) == al(2 * 3 * 8 * 4)        # (at most one slab per chunk)
    assert L.slr_conv1x1_grad_ws_bytes(1, 8, 3, 5, 7, -1) == 0 and L.slr_conv1x1_grad_ws_bytes(1, 0, 3, 5, 7, 0) == 0


def test_entry_points_refuse_bad_arguments_before_launching(L):
    P, BIG = 0x10000, 1 << 24
    bad = lambda rc, word: rc == -1 and word in L.slr_last_error()           # noqa: E731
    assert bad(L.slr_bn_batch_stats(P, None, 1e-5, P, P, P, 1, 12, 4, 4, 1, P, BIG, None), b"C % 8")
    assert bad(L.slr_bn_batch_stats(None, None, 1e-5, P, P, P, 1, 8, 4, 4, 0, P, BIG, None), b"null")
    assert bad(L.slr_bn_batch_stats(P, None, 1e-5, P, P, P, 1, 8, 0, 4, 0, P, BIG, None), b"sizes")
    assert bad(L.slr_bn_batch_stats(P, None, 1e-5, P, P, P, 1, 8, 4, 4, 2, P, BIG, None), b"b8")
    assert bad(L.slr_bn_batch_stats(P + 4, None, 1e-5, P, P, P, 1, 8, 4, 4, 1, P, BIG, None), b"16-byte")
    assert L.slr_bn_batch_stats(P, None, 1e-5, P, P, P, 1, 8, 4, 4, 0, P, 16, None) == -2
    assert L.slr_bn_batch_stats(P, None, 1e-5, P, P, P, 1, 8, 4, 4, 0, P + 16, BIG, None) == -2
    assert bad(L.slr_bn_train_tables(P, P, None, None, 1e-5, P, None, 1, 8, None), b"null")
    assert bad(L.slr_bn_train_tables(P, P, None, None, 1e-5, P, P, 0, 8, None), b"sizes")
    assert bad(L.slr_bn_relu_mask_train(P, P, P, None, P, 1, 12, 4, 4, 1, None), b"C % 8")
    assert bad(L.slr_bn_relu_mask_train(P, P, P, None, None, 1, 8, 4, 4, 0, None), b"null")
    bw = lambda **k: L.slr_bn_relu_mask_backward(*[k.get(n, d) for n, d in (                                 # noqa: E731
        ("x", P), ("ga", P), ("mask", None), ("scale", P), ("shift", P), ("mean", P), ("var", P), ("gain", None), ("count", P), ("eps", 1e-5),
        ("addend", None), ("dx", P), ("dgain", None), ("dbias", None), ("stored", 0), ("N", 1), ("C", 8), ("H", 4), ("W", 4), ("b8", 0),
        ("ws", P), ("ws_bytes", BIG), ("stream", None))])
    assert bad(bw(dx=None), b"nothing to compute")
    assert bad(bw(count=None), b"count")
    assert bad(bw(stored=2), b"stored")
    assert bad(bw(dx=None, dgain=P, addend=P), b"addend")
    assert bad(bw(C=12, b8=1), b"C % 8")
    assert bw(ws=None) == -2 and bw(ws_bytes=16) == -2
    assert bad(L.slr_conv1x1_weight_grad(P, P, P, 1, 12, 8, 4, 4, 0, 1, P, BIG, None), b"Cin % 8")
    assert bad(L.slr_conv1x1_weight_grad(P, P, P, 1, 8, 12, 4, 4, 0, 2, P, BIG, None), b"Cout % 8")
    assert bad(L.slr_conv1x1_weight_grad(P, P, P, 1, 8, 8, 4, 4, -1, 0, P, BIG, None), b"splits")
    assert bad(L.slr_conv1x1_weight_grad(P, P, P, 1, 8, 8, 4, 4, 0, 4, P, BIG, None), b"layout")
    assert L.slr_conv1x1_weight_grad(P, P, P, 1, 8, 8, 4, 4, 0, 0, P, 16, None) == -2
    for fn in (L.slr_avgpool3x3s2_backward, L.slr_upsample_bilinear2x_backward):
        assert bad(fn(P, P, 1, 12, 4, 4, 1, None), b"C % 8")
        assert bad(fn(P, None, 1, 8, 4, 4, 0, None), b"null")
        assert bad(fn(P, P, 1, 8, 0, 4, 0, None), b"sizes")
