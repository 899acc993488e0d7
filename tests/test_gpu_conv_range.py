"""The split-f16 convolutions (csrc/conv.hip) over the whole range of their inputs, against their own written-out arithmetic
(tests/split_model.py) and float64 -- WITHOUT a floor in any tolerance: a layer whose outputs are 1e-4 is judged on the scale of 1e-4.

  a. exact probes: does a subnormal f16 half survive the conversion and the matrix instruction?  Bit for bit against the model.
  b. magnitude sweep, input std 2^7 (2^13 at activation scale 1) .. 2^-20:  E_gpu <= 2 E_model + 10 E_plain32, E = max|a - ref64| / max|ref64|.
     The model's products are exact in fp32, so a kernel may differ from it by its fp32 accumulation only: ten times the error of a plain
     float32 convolution of the same inputs, next to twice the model's own (tests/test_split_model.py keeps a float32-accumulated model inside).
  c. mixed ranges: input channels, output channels (judged per channel) and image halves of different magnitude in one call.
  d. the scale plumbing, exact: wscale per layer, the skip's own wscale, the accumulator rescale between the 3x3 and the fused 1x1 phase.

Kernel families: 3x3 NCHW, 3x3 channel-blocked in and out, 3x3 with the BN + ReLU prologue (scale 1, shift 0), the fused partial convolution
with derived and with explicit mask, 1x1 NCHW and channel-blocked; at nets.activation_scale(64) and (1).  Biases are zero, so outputs scale
with inputs; every case asserts that nothing was clamped.  Controls: the fp32 rung and the <= 4-channel kernel (fp32 arithmetic).
Every test prints its figures (-s); profiles/conv_range.txt is that output."""
import pytest
import torch

import conv_train_f64 as cf
import split_model as sm
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

SCALES = (64.0, 1.0)
DEV = "cuda:0"
FAMILIES_3X3 = ("nchw", "b8", "prologue", "pconv_derived", "pconv_mask")
FAMILIES_1X1 = ("nchw", "b8")
CASES = [(f, s, 3) for f in FAMILIES_3X3 for s in sm.SHAPES_3X3] + [(f, s, 1) for f in FAMILIES_1X1 for s in sm.SHAPES_1X1]
CASE_IDS = [f"{f}-{s[0]}to{s[1]}at{s[2]}x{s[3]}-k{k}" for f, s, k in CASES]
PLAIN_CASES = [c for c in CASES if c[0] == "nchw"]
PLAIN_IDS = [i for c, i in zip(CASES, CASE_IDS) if c[0] == "nchw"]


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


# ------------------------------------------------------------------------------------------------------------------ one layer, every family

def hole_mask(h, w):
    """[BATCH,1,h,w] of ones with one block of zeros wide enough that whole 3x3 windows are empty (the update mask has zeros)."""
    m = torch.ones(sm.BATCH, 1, h, w)
    m[:, :, 2:6, 5:12] = 0.0
    return m


def layer(nets, family, wt):
    cout, cin, k, _ = wt.shape
    mod = (nets.PartialConv if family.startswith("pconv") else nets.Conv)(cin, cout, k).cuda()
    with torch.no_grad():
        mod.weight.copy_(wt)
        mod.bias.zero_()
    return mod


def family_input(family, base, s, positive=False):
    """(x handed to the kernel, the tensor the convolution itself sees, mask [N,1,H,W] or None) for ``base`` at magnitude ``s``."""
    n, c, h, w = base.shape
    m = hole_mask(h, w) if family.startswith("pconv") else None
    if family == "prologue":
        x = (base if positive else torch.relu(base)) * s
        return x, x, None
    if family == "pconv_derived":                     # relu(x * 1 - 0) * (x != 0): the zero block is the derived mask, the same in every channel
        x = base * m * s
        assert bool(((x != 0) == (m != 0)).all())
        return x, torch.relu(x), m
    if family == "pconv_mask":                        # no prologue: x is the already masked input
        x = base * m * s
        return x, x, m
    return base * s, base * s, None


def run(nets, family, mod, x, mask):
    """The family's kernel on the host tensor ``x`` -> host tensors (out, update mask or None)."""
    x = x.cuda()
    cin, cout = mod.weight.shape[1], mod.weight.shape[0]
    ones, zeros = torch.ones(cin, device="cuda"), torch.zeros(cin, device="cuda")
    with torch.no_grad():
        if family == "nchw":
            out, um = mod(x), None
        elif family == "b8":
            lay = (nets.IN_B8 if cin % 8 == 0 else 0) | nets.OUT_B8
            out, um = from_blocked(mod(to_blocked(x) if cin % 8 == 0 else x, layout=lay)), None
        elif family == "prologue":
            out, um = mod(x, (ones, zeros)), None
        elif family == "pconv_derived":
            out, um = mod(x, None, pre_bn=(ones, zeros))
        else:
            out, um = mod(x, mask.cuda())
    return out.cpu(), None if um is None else um.cpu()


def partial_epilogue(raw, mask, cin):
    """(raw * ratio + 0) * um of the partial convolution in the dtype of ``raw`` (tests/conv_train_f64.py), or raw itself without a mask."""
    if mask is None:
        return raw, None
    ratio, um, _ = cf.partial_factors(mask.to(raw.dtype), cin)
    return raw * ratio * um, um


def references(xe, wt, mask, xscale, k):
    """(model, ref64, plain32) of the family's output for the convolution input ``xe``."""
    cin = wt.shape[1]
    model, um = partial_epilogue(sm.conv(xe, wt, xscale, k), mask, cin)
    ref, _ = partial_epilogue(sm.plain(xe.double(), wt.double(), k), mask, cin)
    p32, _ = partial_epilogue(sm.plain(xe, wt, k), mask, cin)
    return model, ref, p32, um


def check_um(um_gpu, um_ref):
    if um_ref is not None:
        assert torch.equal(um_gpu.double(), um_ref.double())
        assert bool((um_ref == 0).any()) and bool((um_ref == 1).any())


def in_domain(x, xscale):
    return float(x.abs().max()) * xscale < sm.F16_MAX_SPLIT


# ------------------------------------------------------------------------------------------------------------------ a. exact probes

def fp32_partial_mirror(raw, mask, cin):
    """The partial epilogue as the kernel computes it, in float32 and in its order (csrc/conv.hip): u = box * mscale, um = clamp(u, 0, 1),
    ratio = (1 / (u + 1e-8)) * winsize * um, out = (raw * ratio + 0) * um.  -> (out, um, ratio * um)."""
    box = sum(cf.shifted(mask.float(), ky - 1, kx - 1) for ky, kx in cf.TAPS)
    u = box * float(cin)
    um = u.clamp(0.0, 1.0)
    ratio = (1.0 / (u + 1e-8)) * float(cin * 9) * um
    return (raw.float() * ratio) * um, um, ratio * um


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("family,shape,k", CASES, ids=CASE_IDS)
def test_probe_subnormal_halves_of_activations_survive(S, family, shape, k, xscale):
    """Centre-tap identity weights (wscale 4096: the split weight is exactly 4096 + 0, every other product an exact zero) on a tensor tiled with
    the probes of split_model.probe_values and their negatives (positives only behind a ReLU): the kernel returns the model's result with f16
    subnormals KEPT, bit for bit -- x itself for A (lo half normal), B (lo half subnormal), C (hi half subnormal), E (large), 0 for D (rounds to 0).
    Every value sits in the first and the last channel of a 16-channel chunk and in the first and last column of a 32-column block.  A B or C
    probe that comes back flushed is a finding about the hardware or the build (ISSUE: locate it by reading, do not re-run)."""
    from slr_sfs_amd import nets
    cin, cout, h, w = shape
    signed = family not in ("prologue", "pconv_derived")
    x, idx, classes = sm.probe_tensor(cin, h, w, xscale, signed)
    if cin >= 16:
        for sel in (idx[0], idx[15], idx[:, :, 0], idx[:, :, 31]):
            assert set(sel.flatten().tolist()) == set(range(len(classes)))
    wt = sm.centre_identity(cin, cout, k)
    xk, xe, mask = family_input(family, x, 1.0, positive=True)
    mod = layer(nets, family, wt)
    nets.saturation_count(DEV)
    with nets.activation_scale(xscale):
        out, um = run(nets, family, mod, xk, mask)
        assert mod._split_weights()[1] == 4096.0
    assert nets.saturation_count(DEV) == 0
    model = sm.conv(xe, wt, xscale, k).float()                       # one exact product per output: the float64 model is an fp32 number
    kept = torch.tensor([c != "D" for c in classes])[idx]
    assert torch.equal(model[:, :cin], xe * kept) and not model[:, cin:].any()
    flushed = sm.conv(xe, wt, xscale, k, flush=True).float()
    gain = None
    if mask is not None:
        model, um_ref, gain = fp32_partial_mirror(model, mask, cin)
        flushed = fp32_partial_mirror(flushed, mask, cin)[0]
        assert torch.equal(um, um_ref)
    same, as_flushed = torch.equal(out, model), torch.equal(out, flushed)
    bad = out != model
    by_class = {c: int((bad[:, :cin] & torch.tensor([cc == c for cc in classes])[idx]).sum()) for c in sorted(set(classes))}
    print(f"probe {family} {cin}->{cout} {h}x{w} k{k} xscale {xscale:g}: equals model with subnormals kept: {same}; equals the flushed model: "
          f"{as_flushed}; differing outputs by class {by_class}, outside the diagonal channels {int(bad[:, cin:].sum())}")
    assert same, (by_class, as_flushed)
    if gain is not None:                                             # where the partial ratio is exactly 1 the probe itself comes back
        one = (gain == 1.0).expand(-1, cin, -1, -1)
        assert bool(one.any())
        assert torch.equal(out[:, :cin][one], (xe * kept)[one])


WEIGHT_PROBES = {"w=2^-16 (normal half after wscale)": 2.0 ** -16, "hi half subnormal: w*4096=2^-16": 2.0 ** -28,
                 "hi half subnormal: w*4096=3*2^-20": 3.0 * 2.0 ** -32, "lo half subnormal: w*4096=1+2^-18": 2.0 ** -12 + 2.0 ** -30,
                 "rounds to 0: w*4096=2^-26": 2.0 ** -38}


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("k", (3, 1))
@pytest.mark.parametrize("name", list(WEIGHT_PROBES))
def test_probe_subnormal_halves_of_weights_survive(S, name, k, xscale):
    """The subnormal half on the WEIGHT side (it goes through conv_split_weights_kernel, the activations through the staging of the forward
    kernels): w[c, c] = value next to one weight of 1 in another channel (max|w| = 1, wscale 4096), activations x * xscale in {1, -1, 1.5}.
    The first value is the one the issue names: at wscale 4096 it is the normal half 2^-4, so it checks the plumbing only; the others are
    subnormal after the scale (hi half, lo half) or vanish.  Bit for bit against the model with subnormals kept."""
    from slr_sfs_amd import nets
    cin, cout, h, w = (16, 32, 8, 32) if k == 3 else (64, 128, 9, 33)
    value = WEIGHT_PROBES[name]
    wt = sm.centre_identity(cin, cout, k, value)
    wt[cout - 1, 0, k // 2, k // 2] = 1.0
    assert float(torch.tensor(value, dtype=torch.float32)) == value and sm.wscale(wt) == 4096.0
    vals = torch.tensor([1.0, -1.0, 1.5]) / xscale
    c, y, xx = torch.meshgrid(torch.arange(cin), torch.arange(h), torch.arange(w), indexing="ij")
    x = vals[(c + y + xx) % 3].unsqueeze(0).repeat(sm.BATCH, 1, 1, 1).contiguous()
    mod = layer(nets, "nchw", wt)
    nets.saturation_count(DEV)
    with nets.activation_scale(xscale):
        out, _ = run(nets, "nchw", mod, x, None)
    assert nets.saturation_count(DEV) == 0
    model = sm.conv(x, wt, xscale, k)
    assert torch.equal(model.float().double(), model)                # exact products: an fp32 number
    expect = x.double() * (0.0 if "rounds to 0" in name else value)
    assert torch.equal(model[:, :cin], expect[:, :cin]) and torch.equal(model[:, cout - 1], x[:, 0].double())
    flushed = sm.conv(x, wt, xscale, k, flush=True).float()
    same, as_flushed = torch.equal(out, model.float()), torch.equal(out, flushed)
    print(f"weight probe '{name}' k{k} xscale {xscale:g}: equals model with subnormals kept: {same}; equals the flushed model: {as_flushed}")
    assert same, as_flushed


# ------------------------------------------------------------------------------------------------------------------ b. magnitude sweep

def judge(tag, out, model, ref, p32):
    e_gpu, e_model, e_plain = sm.E(out, ref), sm.E(model, ref), sm.E(p32, ref)
    bound = 2 * e_model + 10 * e_plain
    print(f"{tag}: E_gpu {e_gpu:.2e} E_model {e_model:.2e} E_plain32 {e_plain:.2e} bound {bound:.2e}")
    return e_gpu, bound


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("family,shape,k", CASES, ids=CASE_IDS)
def test_magnitude_sweep(S, family, shape, k, xscale):
    """x = base * s for s = 2^7 (2^13 at activation scale 1), 1, 2^-4 .. 2^-20; base ~ N(0, 1) (relu of it behind the prologue, a zero block for
    the partial convolutions), weights ~ N(0, 1 / (Cin k k)), zero bias.  Per tensor: E_gpu <= 2 E_model + 10 E_plain32."""
    from slr_sfs_amd import nets
    cin, cout, h, w = shape
    base, wt = sm.seeded(cin, cout, h, w, k)
    mod = layer(nets, family, wt)
    failures = []
    for s in sm.magnitudes(xscale):
        xk, xe, mask = family_input(family, base, s)
        assert in_domain(xk, xscale)
        model, ref, p32, um_ref = references(xe, wt, mask, xscale, k)
        nets.saturation_count(DEV)
        with nets.activation_scale(xscale):
            out, um = run(nets, family, mod, xk, mask)
        assert nets.saturation_count(DEV) == 0
        check_um(um, um_ref)
        e_gpu, bound = judge(f"sweep {family} {cin}->{cout} {h}x{w} k{k} xscale {xscale:g} std {s:.2e}", out, model, ref, p32)
        if not e_gpu <= bound:
            failures.append((s, e_gpu, bound))
    assert not failures, failures


FP32_CASES = [(s, 3) for s in sm.SHAPES_3X3] + [(s, 1) for s in sm.SHAPES_1X1] + [(sm.SHAPE_FEW, 3)]


@pytest.mark.parametrize("shape,k", FP32_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_fp32_controls_are_scale_free(S, shape, k):
    """The controls: the fp32 rung (nets.fp32_kernels(winograd=False)) on the sweep's shapes and the <= 4-channel kernel (fp32 FMAs on either rung).
    E_gpu <= 10 E_plain32 at every magnitude of both sweeps, and conv(x 2^k) == conv(x) 2^k bit for bit for k = -20, -8, 7: fp32 arithmetic
    has no preferred magnitude."""
    from slr_sfs_amd import nets
    cin, cout, h, w = shape
    base, wt = sm.seeded(cin, cout, h, w, k)
    mod = layer(nets, "nchw", wt)
    few = cout <= 4
    ctx = (lambda: nets.activation_scale(64.0)) if few else (lambda: nets.fp32_kernels(winograd=False))
    failures = []
    nets.saturation_count(DEV)
    for s in [sm.TOP[1.0], sm.TOP[64.0]] + sm.MAGNITUDES:
        x = base * s
        ref, p32 = sm.plain(x.double(), wt.double(), k), sm.plain(x, wt, k)
        with ctx():
            out, _ = run(nets, "nchw", mod, x, None)
        e_gpu, e_plain = sm.E(out, ref), sm.E(p32, ref)
        print(f"control {'few' if few else 'fp32 rung'} {cin}->{cout} {h}x{w} k{k} std {s:.2e}: E_gpu {e_gpu:.2e} E_plain32 {e_plain:.2e} "
              f"bound {10 * e_plain:.2e}")
        if not e_gpu <= 10 * e_plain:
            failures.append((s, e_gpu, 10 * e_plain))
    with ctx():
        one, _ = run(nets, "nchw", mod, base, None)
        for p in (-20, -8, 7):
            scaled, _ = run(nets, "nchw", mod, base * 2.0 ** p, None)
            assert torch.equal(scaled, one * 2.0 ** p), p
    assert nets.saturation_count(DEV) == 0
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------ c. mixed ranges

@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("family,shape,k", CASES, ids=CASE_IDS)
def test_mixed_input_channels(S, family, shape, k, xscale):
    """Input channel c scaled by 2^(-2 (c mod 13)): magnitudes 1 .. 2^-24 inside one 16-channel chunk.  Criterion of the sweep, per tensor."""
    from slr_sfs_amd import nets
    cin, cout, h, w = shape
    base, wt = sm.seeded(cin, cout, h, w, k, seed=1)
    base = base * (2.0 ** (-2.0 * (torch.arange(cin) % 13))).view(1, -1, 1, 1)
    xk, xe, mask = family_input(family, base, 1.0)
    model, ref, p32, um_ref = references(xe, wt, mask, xscale, k)
    mod = layer(nets, family, wt)
    nets.saturation_count(DEV)
    with nets.activation_scale(xscale):
        out, um = run(nets, family, mod, xk, mask)
    assert nets.saturation_count(DEV) == 0
    check_um(um, um_ref)
    e_gpu, bound = judge(f"mixed input channels {family} {cin}->{cout} {h}x{w} k{k} xscale {xscale:g}", out, model, ref, p32)
    assert e_gpu <= bound


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("family,shape,k", CASES, ids=CASE_IDS)
def test_mixed_output_channels_judged_per_channel(S, family, shape, k, xscale):
    """Output channel o of the weights scaled by 2^(-2 (o mod 9)): ONE wscale per layer serves all of them, so a small channel's weights live
    on subnormal lo halves.  Judged per output channel on that channel's own scale: E_o <= 2 E_model,o + 10 E_plain32,o."""
    from slr_sfs_amd import nets
    cin, cout, h, w = shape
    base, wt = sm.seeded(cin, cout, h, w, k, seed=2)
    wt = wt * (2.0 ** (-2.0 * (torch.arange(cout) % 9))).view(-1, 1, 1, 1)
    xk, xe, mask = family_input(family, base, 1.0)
    model, ref, p32, um_ref = references(xe, wt, mask, xscale, k)
    mod = layer(nets, family, wt)
    nets.saturation_count(DEV)
    with nets.activation_scale(xscale):
        out, um = run(nets, family, mod, xk, mask)
    assert nets.saturation_count(DEV) == 0
    check_um(um, um_ref)
    e_gpu, e_model, e_plain = sm.E_per_channel(out, ref), sm.E_per_channel(model, ref), sm.E_per_channel(p32, ref)
    bound = 2 * e_model + 10 * e_plain
    worst = int((e_gpu / bound).argmax())
    print(f"mixed output channels {family} {cin}->{cout} {h}x{w} k{k} xscale {xscale:g}: worst channel {worst} (weights x 2^{-2 * (worst % 9)}): "
          f"E_gpu {e_gpu[worst]:.2e} E_model {e_model[worst]:.2e} E_plain32 {e_plain[worst]:.2e} bound {bound[worst]:.2e}; "
          f"largest E_gpu {e_gpu.max():.2e}")
    assert bool((e_gpu <= bound).all()), [(o, float(e_gpu[o]), float(bound[o])) for o in range(cout) if not e_gpu[o] <= bound[o]]


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("family,shape,k", CASES, ids=CASE_IDS)
def test_small_half_next_to_a_large_half(S, family, shape, k, xscale):
    """The left half of the image O(1), the right half 2^-12: judged on the right half's interior columns (a 3x3 window there sees small values
    only) against that half's own scale.  Criterion of the sweep."""
    from slr_sfs_amd import nets
    cin, cout, h, w = shape
    base, wt = sm.seeded(cin, cout, h, w, k, seed=3)
    base = base.clone()
    base[..., w // 2:] *= 2.0 ** -12
    xk, xe, mask = family_input(family, base, 1.0)
    model, ref, p32, um_ref = references(xe, wt, mask, xscale, k)
    mod = layer(nets, family, wt)
    nets.saturation_count(DEV)
    with nets.activation_scale(xscale):
        out, um = run(nets, family, mod, xk, mask)
    assert nets.saturation_count(DEV) == 0
    check_um(um, um_ref)
    right = slice(w // 2 + 1, w)
    assert float(ref[..., right].abs().max()) < 2.0 ** -8 * float(ref.abs().max())
    e_gpu, bound = judge(f"small right half {family} {cin}->{cout} {h}x{w} k{k} xscale {xscale:g}", out[..., right], model[..., right],
                         ref[..., right], p32[..., right])
    assert e_gpu <= bound


# ------------------------------------------------------------------------------------------------------------------ d. scale plumbing, exact

@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("family,shape,k", PLAIN_CASES, ids=PLAIN_IDS)
def test_weight_scale_moves_only_the_unscale(S, family, shape, k, xscale):
    """conv(x, w 2^p) == conv(x, w) 2^p bit for bit for p = -12, -3, 5 on the split 3x3 and 1x1 kernels: wscale follows the weights, the split
    weight buffer is byte-identical, only the inverse scale applied to the accumulators moves."""
    from slr_sfs_amd import nets
    cin, cout, h, w = shape
    base, wt = sm.seeded(cin, cout, h, w, k, seed=4)
    mod = layer(nets, family, wt)
    nets.saturation_count(DEV)
    with nets.activation_scale(xscale):
        one, _ = run(nets, family, mod, base, None)
        buf, ws, xs, arith = mod._split_weights()
        assert ws == sm.wscale(wt) and xs == xscale and arith == 0
        for p in (-12, -3, 5):
            mod_p = layer(nets, family, wt * 2.0 ** p)
            out, _ = run(nets, family, mod_p, base, None)
            buf_p, ws_p, _, _ = mod_p._split_weights()
            assert ws_p == ws * 2.0 ** -p
            assert buf_p.data_ptr() != buf.data_ptr() and torch.equal(buf_p, buf)
            assert torch.equal(out, one * 2.0 ** p), (p, sm.E(out, one * 2.0 ** p))
    assert nets.saturation_count(DEV) == 0
    print(f"weight scale {cin}->{cout} {h}x{w} k{k} xscale {xscale:g}: wscale {ws:g}; w x 2^-12, 2^-3, 2^5: same buffer bytes, outputs scale exactly")


BLOCK_MAGNITUDES = (2.0 ** 7, 1.0, 2.0 ** -8, 2.0 ** -16)


@pytest.mark.parametrize("p", (-12, -3, 5))
@pytest.mark.parametrize("which", ("skip", "main"))
@pytest.mark.parametrize("kind", ("plain", "pconv"))
def test_fused_skip_rescale_against_staged_skip(S, kind, which, p):
    """ResBlock / PconvResBlock(64, 128, "Down") on a channel-blocked input -- the form whose 1x1 skip convolution rides in the second 3x3 kernel
    as extra K chunks, the accumulators re-scaled from 1 / (xscale wscale) to the skip's own 1 / (xscale skip_wscale) in between -- with only the
    skip's weights, or only the main branch's (both 3x3 convolutions), scaled by 2^p, at input magnitudes 2^7, 1, 2^-8, 2^-16: against the staged
    form (nets.staged_skips(): 1x1 kernel, residual of the 3x3 epilogue, pool kernel)  max|fused - staged| <= 2e-6 max|staged|, the bound DESIGN 3.4
    states for the two forms, here without a floor and away from magnitude 1.  Update masks bit-identical.  Both activation scales, wherever the
    case lies inside the rung's exact domain: 7 x (input magnitude) x (the main branch's gain, if above 1) < 65472 / xscale -- seven standard
    deviations of the block input and of its intermediate activation."""
    from slr_sfs_amd import nets
    cin, cout, h, w = 64, 128, 16, 40
    torch.manual_seed(7)
    blk = (nets.PconvResBlock if kind == "pconv" else nets.ResBlock)(cin, cout, "Down").cuda()
    base, _ = sm.seeded(cin, cout, h, w, 3, seed=5)
    mask = hole_mask(h, w).cuda()
    gain = 2.0 ** p
    with torch.no_grad():
        for conv in ((blk.conv_b,) if which == "skip" else (blk.conv_aa, blk.conv_ab)):
            conv.weight.mul_(gain)

    def forward(xb):
        if kind == "pconv":
            y, m, b8 = blk(xb, mask, True)
        else:
            (y, b8), m = blk(xb, True), None
        assert b8
        return from_blocked(y).cpu(), m

    ran = 0
    for xscale in SCALES:
        for s in BLOCK_MAGNITUDES:
            if not 7.0 * s * (max(gain, 1.0) if which == "main" else 1.0) < sm.F16_MAX_SPLIT / xscale:
                continue
            ran += 1
            xb = to_blocked(base * s).cuda()
            nets.saturation_count(DEV)
            with torch.no_grad(), nets.activation_scale(xscale):
                route = nets._block_route(blk, xb, True)
                assert route.form == "fused" and route.pool is True
                fused, m1 = forward(xb)
                with nets.staged_skips():
                    assert nets._block_route(blk, xb, True).form == "staged"
                    staged, m0 = forward(xb)
            assert nets.saturation_count(DEV) == 0
            if m1 is not None:
                assert torch.equal(m1, m0)
            diff, scale = float((fused - staged).abs().max()), float(staged.abs().max())
            print(f"block {kind} {which} x 2^{p} xscale {xscale:g} std {s:.2e}: max|fused - staged| {diff:.2e} = {diff / scale:.2e} of max|staged| "
                  f"{scale:.2e} (bound 2e-6)")
            assert scale > 0 and diff <= 2e-6 * scale, (xscale, s, diff, scale)
    assert ran >= len(BLOCK_MAGNITUDES)
