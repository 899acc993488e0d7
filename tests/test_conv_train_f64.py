"""CPU checks of the trainable 3x3 convolutions: the written-out float64 yardstick (tests/conv_train_f64.py) against torch's float64
autograd through F.conv2d and the PartialConv2d arithmetic as torch ops, and what the new entry points decide on the host -- the
workspace size and every argument check (no device is touched: the pointers are dummy integers)."""
import os

import pytest
import torch
import torch.nn.functional as F

import conv_train_f64 as C64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 8, 3, 5, 7), (2, 3, 32, 16, 16), (2, 40, 72, 33, 20))          # N, Cin, Cout, H, W


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def _inputs(N, cin, cout, H, W):
    g = torch.Generator().manual_seed(N * 1000 + cin * 100 + cout + H + W)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    return r(N, cin, H, W), r(cout, cin, 3, 3), r(cout), r(N, cout, H, W)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plain_yardstick_is_float64_autograd(shape):
    x, w, b, g = _inputs(*shape)
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    out = F.conv2d(xa, wa, ba, padding=1)
    dx, dw, db = torch.autograd.grad(out, (xa, wa, ba), g)
    for name, got, ref in (("out", C64.conv(x, w, b), out), ("dx", C64.conv_dx(g, w), dx), ("dW", C64.conv_dw(x, g), dw),
                           ("db", C64.conv_db(g), db)):
        e = C64.E(got, ref)
        print(f"{name}: {e:.2e}")
        assert e <= 1e-12, (name, e)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_partial_yardstick_is_float64_autograd(shape):
    """PartialConv2d.forward (multi_channel, return_mask) written as torch ops, partialconv2d.py:61-74, with a full-channel mask."""
    N, cin, cout, H, W = shape
    x, w, b, g = _inputs(*shape)
    mask = C64.holed_mask(N, H, W, seed=cin).double()
    xm = x * mask
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (xm, w, b))
    mfull = mask.expand(N, cin, H, W)
    um_raw = F.conv2d(mfull, torch.ones(cout, cin, 3, 3, dtype=torch.float64), padding=1)
    ratio = (cin * 9) / (um_raw + 1e-8)
    um = torch.clamp(um_raw, 0, 1)
    ratio = ratio * um
    raw = F.conv2d(xa, wa, ba, padding=1)                # (xm is masked already: the reference's `input * mask` changes nothing)
    bv = ba.view(1, cout, 1, 1)
    out = ((raw - bv) * ratio + bv) * um
    dx, dw, db = torch.autograd.grad(out, (xa, wa, ba), g)
    got_out, got_um = C64.pconv(xm, mask, w, b)
    gdx, gdw, gdb = C64.pconv_grads(xm, mask, w, g)
    assert (got_um == 0).any() and (got_um == 1).any()
    assert torch.equal(got_um.expand_as(um), um)
    for name, got, ref in (("out", got_out, out), ("dxm", gdx, dx), ("dW", gdw, dw), ("db", gdb, db)):
        e = C64.E(got, ref)
        print(f"{name}: {e:.2e}")
        assert e <= 1e-12, (name, e)


def al256(v):
    return (v + 255) & ~255


def test_workspace_size_is_the_documented_formula(L):
    ws = L.slr_conv3x3_grad_ws_bytes

    def want(N, cin, cout, H, W, S):
        return al256(N * cout * ((H * W + 255) // 256) * 8) + (al256(S * 9 * cout * cin * 4) if cin else 0)

    def auto(N, cin, cout, H, W):
        chunks = N * ((H + 1) // 2) * ((W + 31) // 32)
        tiles = ((cin + 63) // 64) * ((cout + 63) // 64)
        return max(1, min((512 + tiles - 1) // tiles, chunks, (32 << 20) // (36 * cout * cin)))

    for shape in ((2, 64, 64, 256, 256), (2, 64, 128, 256, 256), (2, 128, 256, 128, 128), (2, 256, 256, 64, 64), (2, 128, 3, 256, 256),
                  (2, 64, 64, 37, 51), (1, 8, 3, 5, 7), (1, 1, 1, 1, 1)):
        assert ws(*shape, 0) == want(*shape, auto(*shape)), shape
        assert ws(*shape, 0) <= (32 << 20) + al256(shape[0] * shape[2] * ((shape[3] * shape[4] + 255) // 256) * 8) + 256
    assert auto(2, 64, 64, 256, 256) == 227 and auto(2, 256, 256, 64, 64) == 14 and auto(2, 64, 64, 37, 51) == 76
    assert ws(2, 64, 64, 37, 51, 3) == want(2, 64, 64, 37, 51, 3)
    assert ws(2, 64, 64, 37, 51, 1000) == want(2, 64, 64, 37, 51, 76)          # at most one slab per chunk
    assert ws(2, 0, 64, 37, 51, 0) == al256(2 * 64 * 8 * 8)                    # the bias part alone: what the scale / bias pass needs
    for bad in ((0, 64, 64, 8, 8, 0), (1, 64, 0, 8, 8, 0), (1, 64, 64, 0, 8, 0), (1, 64, 64, 8, -1, 0), (1, 64, 64, 8, 8, -1),
                (1, 64, 64, 65536, 65536, 0), (1024, 8, 64, 8, 8, 0)):
        assert ws(*bad) == 0, bad


def test_entry_points_refuse_bad_arguments_on_the_host(L):
    P, N, cin, cout, H, W = 0x10000, 2, 64, 64, 37, 51       # a 256-byte aligned non-null "pointer"
    need = L.slr_conv3x3_grad_ws_bytes(N, cin, cout, H, W, 0)

    def refused(rc, code, *words):
        msg = L.slr_last_error()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    def wgrad(x=P, g=P, dw=P, db=P, N=N, cin=cin, cout=cout, H=H, W=W, splits=0, layout=0, ws=P, ws_bytes=need):
        return L.slr_conv3x3_weight_grad(x, g, dw, db, N, cin, cout, H, W, splits, layout, ws, ws_bytes, None)

    for name in ("x", "g", "dw"):
        refused(wgrad(**{name: None}), -1, b"slr_conv3x3_weight_grad", b"null")
    for kw in ({"N": 0}, {"cin": 0}, {"cout": -1}, {"H": 0}, {"W": 0}, {"H": 65536, "W": 65536}, {"N": 2048}):
        refused(wgrad(**kw), -1, b"slr_conv3x3_weight_grad", b"sizes")
    refused(wgrad(splits=-1), -1, b"splits")
    refused(wgrad(layout=4), -1, b"layout")
    refused(wgrad(cin=12, layout=1), -1, b"Cin % 8")
    refused(wgrad(cout=12, layout=2), -1, b"Cout % 8")
    refused(wgrad(x=P + 4, layout=1), -1, b"16-byte")
    refused(wgrad(g=P + 8, layout=2), -1, b"16-byte")
    refused(wgrad(x=P + 2), -1, b"4-byte")
    refused(wgrad(ws=None), -2, b"ws")
    refused(wgrad(ws=P + 64), -2, b"ws", b"aligned")
    refused(wgrad(ws_bytes=need - 1), -2, b"ws")
    refused(wgrad(splits=76, ws_bytes=L.slr_conv3x3_grad_ws_bytes(N, cin, cout, H, W, 3)), -2, b"ws")

    bneed = L.slr_conv3x3_grad_ws_bytes(N, 0, cout, H, W, 0)

    def sb(g=P, r=P, um=P, gr=P, db=P, N=N, C=cout, H=H, W=W, layout=0, ws=P, ws_bytes=bneed):
        return L.slr_conv_grad_scale_bias(g, r, um, gr, db, N, C, H, W, layout, ws, ws_bytes, None)

    refused(sb(g=None), -1, b"slr_conv_grad_scale_bias", b"null")
    refused(sb(gr=None, db=None), -1, b"null")
    refused(sb(r=None), -1, b"null", b"gr needs r")
    for kw in ({"N": 0}, {"C": 0}, {"H": 0}, {"W": -3}, {"H": 65536, "W": 65536}):
        refused(sb(**kw), -1, b"sizes")
    refused(sb(layout=1), -1, b"layout")
    refused(sb(C=12, layout=2), -1, b"C % 8")
    refused(sb(g=P + 8, layout=2), -1, b"16-byte")
    refused(sb(gr=P + 4, layout=2), -1, b"16-byte")
    refused(sb(ws=None), -2, b"ws")
    refused(sb(ws_bytes=bneed - 1), -2, b"ws")
    refused(sb(ws=P + 8), -2, b"ws", b"aligned")


def test_operators_refuse_cpu_tensors():
    import slr_sfs_amd as S
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        S.conv3x3(z(1, 8, 4, 4), z(8, 8, 3, 3), z(8))
    with pytest.raises(NotImplementedError):
        S.partial_conv3x3(z(1, 8, 4, 4), z(1, 1, 4, 4), z(8, 8, 3, 3), z(8))
    with pytest.raises(NotImplementedError):
        S.TrainableConv3x3(8, 8)(z(1, 8, 4, 4))
    with pytest.raises(NotImplementedError):
        S.TrainablePartialConv3x3(8, 8)(z(1, 8, 4, 4), z(1, 1, 4, 4))
    m, c = S.TrainablePartialConv3x3(8, 16), S.nets.Conv(8, 16, 3)
    assert list(m.state_dict()) == list(c.state_dict()) == ["weight", "bias"]
    assert all(p.requires_grad for p in m.parameters()) and not any(p.requires_grad for p in c.parameters())
