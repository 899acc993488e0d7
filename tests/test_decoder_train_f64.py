"""CPU checks of the trainable networks' yardstick (tests/decoder_train_f64.py): its written-out formulas against torch's float64 autograd
of the reference's own operations written with torch operators -- partial_manual_bn with the [N,C,H,W] mask (x != 0).float()
(models/layers/normalization.py:319-354), PartialConv2d's mask arithmetic with F.conv2d(mask, ones) (models/layers/partialconv2d.py:61-74),
F.conv2d, F.avg_pool2d / F.interpolate -- to 1e-12; against the reference's own blocks and networks in train() mode and float64
(tests/golden/decoder_train_vs_reference.npz, made by tools/make_golden_decoder_train.py) to 1e-10; then what the ABI 17 entry points decide on the host (no device is touched: the
pointers are dummy integers).

One kind of tensor is measured against the magnitude of its terms (block_train_f64.E_terms): the gradient to a convolution's bias where, and
only where, a batch-norm with batch statistics follows it (db_aa in batch mode; db_ab and db_b of every chain block but the last).  That batch-norm removes a per-channel constant, so the gradient cancels to rounding (exactly to zero
behind manual_bn); against max|ref| two float64 evaluations in different orders do not agree."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import block_train_f64 as B64
import conv_train_f64 as C64
import decoder_train_f64 as D64

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_train_vs_reference.npz")


def _close(name, got, ref, tol=1e-12, terms=None):
    e = C64.E(got, ref) if terms is None else B64.E_terms(got, ref, terms)
    print(f"{name}: {e:.2e}")
    assert e <= tol, (name, e)


# ------------------------------------------------------------------ the reference's operations, with torch operators and autograd

def ag_bn(x, mask, gain, bias, stored=None, eps=1e-5):
    """partial_manual_bn (mask [N,C,H,W] or [N,1,H,W]) / manual_bn (mask None) + partial_fused_bn"""
    if stored is not None:
        m, var = stored[0].view(1, -1, 1, 1), stored[1].view(1, -1, 1, 1)
    else:
        cnt = float(x.shape[0] * x.shape[2] * x.shape[3]) if mask is None else torch.sum(mask.expand_as(x), [0, 2, 3], keepdim=True) + eps
        m, m2 = torch.sum(x, [0, 2, 3], keepdim=True) / cnt, torch.sum(x ** 2, [0, 2, 3], keepdim=True) / cnt
        var = m2 - m ** 2
    scale = torch.rsqrt(var + eps) * gain[:, :, None, None]
    return x * scale - (m * scale - bias[:, :, None, None])


def ag_pconv(x, mask, w, b):
    """PartialConv2d(multi_channel=True, return_mask=True).forward with mask [N,Cin,H,W]; the update mask as one plane"""
    cin = x.shape[1]
    um = F.conv2d(mask, torch.ones(1, cin, 3, 3, dtype=x.dtype), padding=1)
    ratio = (cin * 9.0) / (um + 1e-8)
    um = torch.clamp(um, 0, 1)
    ratio = ratio * um
    raw = F.conv2d(x * mask, w, b, padding=1)
    return ((raw - b.view(1, -1, 1, 1)) * ratio + b.view(1, -1, 1, 1)) * um, um


def ag_resample(x, kind):
    if kind == "Up":
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return F.avg_pool2d(x, 3, stride=2, padding=1) if kind else x


def ag_pconv_block(x, mask, p, kind, gains, biases, stored=(None, None)):
    """ResNet_Block_Pconv2.forward (blocks.py:218-248); mask [N,Cin,H,W] or [N,1,H,W]"""
    mask = mask.expand_as(x)
    a = torch.relu(ag_bn(x, mask, gains[0], biases[0], stored[0]))
    a, m = ag_pconv(a, mask, p["w_aa"], p["b_aa"])
    a = torch.relu(ag_bn(a, m, gains[1], biases[1], stored[1]))
    a, m = ag_pconv(a, m.expand_as(a), p["w_ab"], p["b_ab"])
    skip = F.conv2d(x, p["w_b"]) if p.get("w_b") is not None else x
    return ag_resample(a, kind) + ag_resample(skip, kind), B64.resample_mask(m, kind)


def ag_res_block(x, p, kind, gains, biases, stored=(None, None)):
    """ResNet_Block.forward (blocks.py:47-87)"""
    a = F.conv2d(torch.relu(ag_bn(x, None, gains[0], biases[0], stored[0])), p["w_aa"], p["b_aa"], padding=1)
    a = F.conv2d(torch.relu(ag_bn(a, None, gains[1], biases[1], stored[1])), p["w_ab"], p["b_ab"], padding=1)
    skip = F.conv2d(x, p["w_b"], p["b_b"]) if p.get("w_b") is not None else x
    return ag_resample(a, kind) + ag_resample(skip, kind)


# ------------------------------------------------------------------ cases

def _params(gen, cin, cout, kind, plain):
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)                  # noqa: E731
    p = dict(w_aa=r(cout, cin, 3, 3) / (3.0 * cin ** 0.5), b_aa=0.3 * r(cout), w_ab=r(cout, cout, 3, 3) / (3.0 * cout ** 0.5), b_ab=0.3 * r(cout),
             w_b=r(cout, cin, 1, 1) / cin ** 0.5 if (kind or cin != cout) else None)
    if plain:
        p["b_b"] = 0.3 * r(cout) if p["w_b"] is not None else None
    return p, [1.0 + 0.3 * r(2, cin), 1.0 + 0.3 * r(2, cout)], [0.5 * r(2, cin), 0.5 * r(2, cout)]


def _x(N, C, H, W, seed, zero_channel=True):
    return (B64.bn_inputs(N, C, H, W, seed)[0] * D64.keep_pattern(N, C, H, W, seed, zero_channel)).double()


def _leaves(x, p, gains, biases):
    xa = x.clone().requires_grad_(True)
    pa = {k: (None if v is None else v.clone().requires_grad_(True)) for k, v in p.items()}
    return xa, pa, [t.clone().requires_grad_(True) for t in gains], [t.clone().requires_grad_(True) for t in biases]


def _check_block_grads(tag, d, y, g, xa, pa, ga, ba, stored=False):
    names = [k for k in ("w_aa", "b_aa", "w_ab", "b_ab", "w_b", "b_b") if pa.get(k) is not None]
    grads = torch.autograd.grad(y, [xa] + [pa[k] for k in names] + ga + ba, g)
    _close(f"{tag} dx", d["dx"], grads[0])
    for k, t in zip(names, grads[1:]):
        _close(f"{tag} d{k}", d["d" + k], t, terms=d["db_aa_terms"] if k == "b_aa" and not stored else None)
    for i in (0, 1):
        _close(f"{tag} dgain{i + 1}", d[f"dgain{i + 1}"], grads[1 + len(names) + i])
        _close(f"{tag} dbias{i + 1}", d[f"dbias{i + 1}"], grads[3 + len(names) + i])


@pytest.mark.parametrize("stored", [False, True], ids=["batch", "stored"])
def test_per_element_bn_is_float64_autograd_of_the_reference_formula(stored):
    N, C, H, W = 2, 6, 9, 7
    x = _x(N, C, H, W, 3)
    _, gain, bias, ga = (t.double() for t in B64.bn_inputs(N, C, H, W, 3))
    st = (torch.linspace(-1, 1, C, dtype=F64), torch.linspace(0.5, 2, C, dtype=F64)) if stored else None
    addend = torch.randn(x.shape, dtype=F64, generator=torch.Generator().manual_seed(1))
    xa, g_, b_ = (t.clone().requires_grad_(True) for t in (x, gain, bias))
    mask = (xa != 0).double()
    a_ref = torch.relu(ag_bn(xa, mask, g_, b_, st)) * mask
    a, mean, var, msum = D64.bn_nz_train(x, gain, bias, stored=st)
    _close("a", a, a_ref, 1e-13)
    assert torch.equal(msum, mask.sum(1, keepdim=True).detach())
    if not stored:                                       # channel 0 is zero everywhere: cnt = eps, m = v = 0
        assert float(mean[0]) == 0.0 == float(var[0])
    dx, dgain, dbias = torch.autograd.grad(a_ref, (xa, g_, b_), ga)
    got = D64.bn_nz_train_grads(x, gain, bias, ga, stored=st, addend=addend)
    _close("dx", got[0], dx + addend)
    _close("dgain", got[1], dgain)
    _close("dbias", got[2], dbias)
    if not stored:                                       # the statistics' gradient reaches the zero elements
        assert float(dx[x == 0].abs().max()) > 0


def test_count_plane_factors_are_partialconv2d():
    N, cin, cout, H, W = 2, 5, 4, 9, 7
    gen = torch.Generator().manual_seed(5)
    x = _x(N, cin, H, W, 5)
    w, b, g = (torch.randn(*s, generator=gen, dtype=F64) for s in ((cout, cin, 3, 3), (cout,), (N, cout, H, W)))
    mask = (x != 0).double()
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    out_ref, um_ref = ag_pconv(xa, mask, wa, ba)
    out, um = D64.pconv_counts(x, mask.sum(1, keepdim=True), w, b)
    assert torch.equal(um, um_ref) and 0.0 < float(um.mean()) < 1.0
    _close("out", out, out_ref, 1e-13)
    dx, dw, db = D64.pconv_counts_grads(x, mask.sum(1, keepdim=True), w, g)
    # (PartialConv2d multiplies its input by the mask once more: autograd's gradient at x is the gradient at xm times the mask)
    for name, got, ref in zip(("dx", "dw", "db"), (dx * mask, dw, db), torch.autograd.grad(out_ref, (xa, wa, ba), g)):
        _close(name, got, ref)


@pytest.mark.parametrize("stored", [False, True], ids=["batch", "stored"])
@pytest.mark.parametrize("spec", [(8, 16, None), (16, 16, None), (8, 12, "Down"), (12, 8, "Up")], ids=str)
def test_input_block_is_float64_autograd(spec, stored):
    cin, cout, kind = spec
    N, H, W = 2, 10, 8
    gen = torch.Generator().manual_seed(cin + cout)
    p, gains, biases = _params(gen, cin, cout, kind, plain=False)
    x = _x(N, cin, H, W, cin, zero_channel=not stored)
    st = tuple((torch.linspace(-1, 1, c, dtype=F64), torch.linspace(0.5, 2, c, dtype=F64)) for c in (cin, cout)) if stored else None
    xa, pa, ga, ba = _leaves(x, p, gains, biases)
    y_ref, um_ref = ag_pconv_block(xa, (xa != 0).double(), pa, kind, ga, ba, st or (None, None))
    f = D64.input_block(x, p, kind, gains, biases, stored=st)
    _close("y", f["y"], y_ref, 1e-13)
    assert torch.equal(f["um"], um_ref)
    g = torch.randn(y_ref.shape, generator=gen, dtype=F64)
    _check_block_grads("input block", D64.input_block_grads(x, p, kind, gains, biases, g, stored=st), y_ref, g, xa, pa, ga, ba, stored)


@pytest.mark.parametrize("stored", [False, True], ids=["batch", "stored"])
@pytest.mark.parametrize("spec", [(3, 16, None), (16, 16, None), (8, 12, "Down"), (12, 8, "Up")], ids=str)
def test_res_block_is_float64_autograd(spec, stored):
    cin, cout, kind = spec
    N, H, W = 2, 10, 8
    gen = torch.Generator().manual_seed(cin + cout)
    p, gains, biases = _params(gen, cin, cout, kind, plain=True)
    x = B64.bn_inputs(N, cin, H, W, cin)[0].double()
    st = tuple((torch.linspace(-1, 1, c, dtype=F64), torch.linspace(0.5, 2, c, dtype=F64)) for c in (cin, cout)) if stored else None
    xa, pa, ga, ba = _leaves(x, p, gains, biases)
    y_ref = ag_res_block(xa, pa, kind, ga, ba, st or (None, None))
    _close("y", D64.res_block(x, p, kind, gains, biases, stored=st)["y"], y_ref, 1e-13)
    g = torch.randn(y_ref.shape, generator=gen, dtype=F64)
    _check_block_grads("res block", D64.res_block_grads(x, p, kind, gains, biases, g, stored=st), y_ref, g, xa, pa, ga, ba, stored)


def _check_chain_grads(tag, ds, y, g, xa, leaves):
    """Every gradient of every block of a chain against autograd through the whole chain, to 1e-12"""
    _close(f"{tag} dx", ds[0]["dx"], torch.autograd.grad(y, xa, g, retain_graph=True)[0])
    for i, (pa, ga, ba) in enumerate(leaves):
        names = [k for k in ("w_aa", "b_aa", "w_ab", "b_ab", "w_b", "b_b") if pa.get(k) is not None]
        grads = torch.autograd.grad(y, [pa[k] for k in names] + ga + ba, g, retain_graph=True)
        for k, t in zip(names, grads):
            behind_bn = k == "b_aa" or (k in ("b_ab", "b_b") and i < len(leaves) - 1)          # a batch-statistics BN follows
            _close(f"{tag} block {i} d{k}", ds[i]["d" + k], t, terms=ds[i]["db_ab_terms" if k == "b_b" else f"d{k}_terms"] if behind_bn else None)
        for j in (0, 1):
            _close(f"{tag} block {i} dgain{j + 1}", ds[i][f"dgain{j + 1}"], grads[len(names) + j])
            _close(f"{tag} block {i} dbias{j + 1}", ds[i][f"dbias{j + 1}"], grads[len(names) + 2 + j])


def test_chains_are_float64_autograd():
    """A narrow decoder (the real resampling pattern) and a narrow encoder: the chained definitions against autograd through the chain."""
    N, H, W = 2, 8, 8
    gen = torch.Generator().manual_seed(11)
    kinds = [None, "Down", "Down", None, "Up", "Up", None, None]
    ch = [8, 16, 24, 24, 16, 16, 16, 8, 3]
    cases = [_params(gen, ch[i], ch[i + 1], kinds[i], plain=False) for i in range(8)]
    ps, gains, biases = ([c[j] for c in cases] for j in range(3))
    x = _x(N, 8, H, W, 2, zero_channel=False)
    xa = x.clone().requires_grad_(True)
    leaves = [_leaves(x, ps[i], gains[i], biases[i])[1:] for i in range(8)]
    y, mask = xa, (xa != 0).double()
    for i in range(8):
        y, mask = ag_pconv_block(y, mask, leaves[i][0], kinds[i], leaves[i][1], leaves[i][2])
    g = torch.randn(y.shape, generator=gen, dtype=F64)
    fs, ds = D64.decoder_grads(x, ps, kinds, gains, biases, g)
    _close("decoder y", fs[-1]["y"], y)
    _check_chain_grads("decoder", ds, y, g, xa, leaves)

    ch = [3, 8, 8, 8, 16, 16, 16, 16, 17]
    cases = [_params(gen, ch[i], ch[i + 1], None, plain=True) for i in range(8)]
    ps, gains, biases = ([c[j] for c in cases] for j in range(3))
    x = torch.randn(N, 3, H, W, generator=gen, dtype=F64)
    xa = x.clone().requires_grad_(True)
    leaves = [_leaves(x, ps[i], gains[i], biases[i])[1:] for i in range(8)]
    y = xa
    for i in range(8):
        y = ag_res_block(y, leaves[i][0], None, leaves[i][1], leaves[i][2])
    g = torch.randn(y.shape, generator=gen, dtype=F64)
    fs, ds = D64.encoder_grads(x, ps, [None] * 8, gains, biases, g)
    _close("encoder y", fs[-1]["y"], y)
    _check_chain_grads("encoder", ds, y, g, xa, leaves)


def test_keep_pattern_and_nudging_keep_their_promises():
    """The GPU tests' input recipe: zeros stay exact zeros, kept gates clear 1e-4, the count plane spans 0 .. C - 1 (C - 2 in image 0), variances are >= 0."""
    for N, C, H, W in ((1, 8, 5, 7), (2, 24, 33, 20)):
        x, gain, bias, _ = B64.bn_inputs(N, C, H, W, seed=C * 10 + H)
        x = x * D64.keep_pattern(N, C, H, W, seed=C + W)
        xn = D64.nudged_nz(x, gain, bias)
        assert torch.equal(xn == 0, x == 0) and D64.gate_margin_nz(xn, gain, bias) > 1e-4
        m, v, cnt = D64.bn_nz_stats(xn.double())
        assert float(v.min()) >= 0.0 and float(cnt[0]) == 1e-5 and float(m[0]) == 0.0
        msum = D64.kept(xn).sum(1)
        assert float(msum.min()) == 0.0 and float(msum.max()) == (C - 1 if N > 1 else C - 2)      # (image 0 lacks channel 1 as well)


# ------------------------------------------------------------------ the reference's own networks (tools/make_golden_decoder_train.py)

@pytest.fixture(scope="module")
def G():
    return D64.load_packed(GOLDEN)


def _case(G, name):
    return {k[len(name) + 1:]: v.double() for k, v in G.items() if k.startswith(name + "/")}


_PCONV = dict(bn1="bn_noise1", bn2="bn_noise2", aa="conv_aa", ab="conv_ab", b="conv_b", stat="pbn")
_PLAIN = dict(bn1="ch_a.0", bn2="ch_a.3", aa="ch_a.2", ab="ch_a.5", b="ch_b.0", stat="bn")


def _ref_block(c, b, names):
    """(p, gains, biases, noise) of the block with key prefix b, in the yardstick's terms"""
    p = dict(w_aa=c[f"p/{b}{names['aa']}.weight"], b_aa=c[f"p/{b}{names['aa']}.bias"], w_ab=c[f"p/{b}{names['ab']}.weight"],
             b_ab=c[f"p/{b}{names['ab']}.bias"], w_b=c.get(f"p/{b}{names['b']}.weight"), b_b=c.get(f"p/{b}{names['b']}.bias"))
    bns = (b + names["bn1"], b + names["bn2"])
    return p, [c["gain/" + k] for k in bns], [c["bias/" + k] for k in bns], [c["noise/" + k] for k in bns]


def _against_reference(tag, c, b, names, f, d, noise, bn_follows=False):
    """One block's gradients and stored statistics against the recorded ones.  bn_follows: the block is not the last of a chain, so a
    batch-norm with batch statistics follows its conv_ab and conv_b as well."""
    want = {"dw_aa": f"{names['aa']}.weight", "db_aa": f"{names['aa']}.bias", "dw_ab": f"{names['ab']}.weight", "db_ab": f"{names['ab']}.bias",
            "dw_b": f"{names['b']}.weight", "db_b": f"{names['b']}.bias"}
    for k, key in want.items():
        if f"d/{b}{key}" in c:
            terms = d["db_ab_terms" if k == "db_b" else k + "_terms"] if (k == "db_aa" or (bn_follows and k in ("db_ab", "db_b"))) else None
            _close(f"{tag} {k}", d[k], c[f"d/{b}{key}"], 1e-10, terms)
    for i in (1, 2):
        bn = b + names[f"bn{i}"]
        _close(f"{tag} gain{i}.weight", d[f"dgain{i}"].t() @ noise[i - 1], c[f"d/{bn}.gain.weight"], 1e-10)
        _close(f"{tag} bias{i}.weight", d[f"dbias{i}"].t() @ noise[i - 1], c[f"d/{bn}.bias.weight"], 1e-10)
        _close(f"{tag} stored_mean{i}", 0.1 * f[f"mean{i}"], c[f"s/{bn}.{names['stat']}.stored_mean"], 1e-10)
        _close(f"{tag} stored_var{i}", 0.9 + 0.1 * f[f"var{i}"], c[f"s/{bn}.{names['stat']}.stored_var"], 1e-10)


@pytest.mark.parametrize("name", ["pblock_8_16", "pblock_16_16"])
def test_input_block_is_the_reference_block_with_its_per_element_mask(G, name):
    c = _case(G, name)
    p, gains, biases, noise = _ref_block(c, "", _PCONV)
    assert (c["x"] == 0).any() and (p["w_b"] is None) == (name == "pblock_16_16")
    f = D64.input_block(c["x"], p, None, gains, biases)
    _close("y", f["y"], c["y"], 1e-10)
    assert torch.equal(f["um"], c["um"])
    d = D64.input_block_grads(c["x"], p, None, gains, biases, c["g"])
    _close("dx", d["dx"], c["dx"], 1e-10)
    _against_reference(name, c, "", _PCONV, f, d, noise)


@pytest.mark.parametrize("name,kind", [("block_None_8_8", None), ("block_Down_8_16", "Down"), ("block_Up_16_8", "Up")])
def test_res_block_is_the_reference_block(G, name, kind):
    c = _case(G, name)
    p, gains, biases, noise = _ref_block(c, "", _PLAIN)
    assert (p["w_b"] is None) == (kind is None)
    f = D64.res_block(c["x"], p, kind, gains, biases)
    _close("y", f["y"], c["y"], 1e-10)
    d = D64.res_block_grads(c["x"], p, kind, gains, biases, c["g"])
    _close("dx", d["dx"], c["dx"], 1e-10)
    _against_reference(name, c, "", _PLAIN, f, d, noise)


@pytest.mark.parametrize("name", ["decoder", "encoder"])
def test_chains_are_the_reference_networks(G, name):
    """ResNetDecoderPconv2.forward on a narrow architecture with the real resampling pattern, and a narrow ResNetEncoder_with_Z"""
    c = _case(G, name)
    plain = name == "encoder"
    names, prefix = (_PLAIN, "gblocks") if plain else (_PCONV, "eblocks")
    kinds = [None] * 8 if plain else [None, "Down", "Down", None, "Up", "Up", None, None]
    blocks = [_ref_block(c, f"{prefix}.{i}.", names) for i in range(8)]
    ps, gains, biases = ([b[j] for b in blocks] for j in range(3))
    fs, ds = (D64.encoder_grads if plain else D64.decoder_grads)(c["x"], ps, kinds, gains, biases, c["g"])
    _close(f"{name} y", fs[-1]["y"], c["y"], 1e-10)
    _close(f"{name} dx", ds[0]["dx"], c["dx"], 1e-10)
    for i in range(8):
        _against_reference(f"{name} block {i}", c, f"{prefix}.{i}.", names, fs[i], ds[i], blocks[i][3], bn_follows=i < 7)


# ------------------------------------------------------------------ the entry points' host side

@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    return slr_sfs_amd._lib.lib()


def test_abi17_entry_points_refuse_bad_sizes_and_workspaces(L):
    P = ctypes.c_void_p
    ok = P(4096)                                         # a dummy, 256-byte aligned pointer: nothing launches on an argument error
    N, C, H, W = 2, 16, 9, 7
    need = L.slr_bn_nonzero_ws_bytes(N, C, H, W)
    assert need > 0 and need % 256 == 0
    assert L.slr_bn_nonzero_ws_bytes(1, 65536, 2, 2) == 0 and L.slr_bn_nonzero_ws_bytes(1, 8, 1 << 14, 1 << 14) == 0
    assert L.slr_bn_nonzero_ws_bytes(0, 8, 4, 4) == 0
    stats = lambda n, c, h, w, b8, ws, nb: L.slr_bn_nonzero_stats(ok, 1e-5, ok, ok, ok, n, c, h, w, b8, ws, nb, None)   # noqa: E731
    assert stats(1, 65536, 2, 2, 0, ok, 1 << 30) == -1                      # N * C > 65535
    assert stats(1, 8, 1 << 14, 1 << 14, 0, ok, 1 << 30) == -1              # N * C * H * W >= 2^31 - 1024
    assert stats(N, 12, H, W, 1, ok, 1 << 30) == -1                         # blocked needs C % 8 == 0
    assert stats(N, C, H, W, 2, ok, 1 << 30) == -1
    assert stats(N, C, H, W, 0, ok, need - 1) == -2 and stats(N, C, H, W, 0, P(4096 + 16), need) == -2 and stats(N, C, H, W, 0, None, need) == -2
    assert b"slr_bn_nonzero_ws_bytes" in L.slr_last_error()
    assert L.slr_bn_nonzero_stats(None, 1e-5, ok, ok, ok, N, C, H, W, 0, ok, need, None) == -1
    assert L.slr_nonzero_count_plane(ok, ok, 1, 65536, 2, 2, 0, None) == -1 and L.slr_nonzero_count_plane(ok, None, N, C, H, W, 0, None) == -1
    assert L.slr_nonzero_count_plane(P(4096 + 4), ok, N, C, H, W, 1, None) == -1           # blocked x: 16-byte aligned
    assert L.slr_bn_relu_nonzero_train(ok, ok, ok, ok, 1, 65536, 2, 2, 0, None) == -1
    assert L.slr_bn_relu_nonzero_train(ok, ok, None, ok, N, C, H, W, 0, None) == -1
    back = lambda dx, dg, db, stored, count, addend, ws, nb, n=N, c=C: L.slr_bn_relu_nonzero_backward(   # noqa: E731
        ok, ok, ok, ok, ok, ok, ok, count, 1e-5, addend, dx, dg, db, stored, n, c, H, W, 0, ws, nb, None)
    assert back(None, None, None, 0, ok, None, ok, need) == -1               # nothing to compute
    assert back(ok, None, None, 0, None, None, ok, need) == -1               # batch statistics need their counts
    assert back(None, ok, None, 1, None, ok, ok, need) == -1                 # addend goes with dx
    assert back(ok, None, None, 2, ok, None, ok, need) == -1
    assert back(ok, ok, ok, 0, ok, None, ok, need, n=1, c=65536) == -1
    assert back(ok, None, None, 0, ok, None, ok, need - 1) == -2 and back(None, ok, None, 1, None, None, None, 0) == -2
    assert back(ok, None, None, 0, ok, None, P(4096 + 128), need) == -2
    assert L.slr_pconv_train_epilogue(ok, ok, ok, ok, None, ok, 1, 65536, 2, 2, 0, None) == -1
    assert L.slr_pconv_train_epilogue(ok, ok, ok, None, None, ok, N, C, H, W, 0, None) == -1
    assert L.slr_pconv_train_epilogue(ok, ok, ok, ok, None, ok, N, 12, H, W, 1, None) == -1
