"""CPU checks of tests/split_model.py, the written-out definition of the split-f16 convolutions that tests/test_gpu_conv_range.py holds the
kernels to: the split of the exact probes with and without f16 subnormals, the probe convolution's expected result, and the model accumulated
in float32 -- a kernel's only legitimate difference -- inside the bound of the GPU tests at every shape, scale and magnitude they use."""
import pytest
import torch

import conv_train_f64 as cf
import split_model as sm

SCALES = (64.0, 1.0)


@pytest.mark.parametrize("xscale", SCALES)
def test_probe_split_is_exact_with_subnormals_and_lossy_without(xscale):
    """(hi + lo) / xscale gives x back bit for bit for the classes A, B, C, E and 0 for D (below half the smallest subnormal) when subnormal halves
    are kept; flushing them changes exactly the classes B (lo half lost) and C (hi half lost)."""
    x, classes = sm.probe_values(xscale)
    assert set(classes) == ({"A", "B", "C", "D", "E"} if xscale == 64.0 else {"A", "B", "C", "D"})
    v = x * xscale
    assert torch.equal(v / xscale, x)                                        # the pre-scale is exact
    hi, lo = sm.split(v)
    back = ((hi.double() + lo.double()) / xscale).float()
    hf, lf = sm.split(v, flush=True)
    flushed = ((hf.double() + lf.double()) / xscale).float()
    for i, cls in enumerate(classes):
        want = 0.0 if cls == "D" else float(x[i])
        assert float(back[i]) == want, (cls, float(x[i]), float(back[i]))
        assert (float(flushed[i]) != float(back[i])) == (cls in "BC"), (cls, float(x[i]), float(flushed[i]))
    sub = lambda h: (h.float().abs() < sm.F16_MIN_NORMAL) & (h != 0)          # noqa: E731
    for i, cls in enumerate(classes):                                        # the classes are what their names say
        assert bool(sub(lo)[i]) == (cls == "B") and bool(sub(hi)[i]) == (cls == "C"), (cls, float(hi[i]), float(lo[i]))


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("k", (3, 1))
def test_probe_convolution_returns_the_probe(xscale, k):
    """The centre-tap identity (wscale 4096, split weight exactly 4096 + 0) on the probe tensor: the model returns x for A, B, C, E and 0 for D in
    the first Cin output channels, 0 in the others; every probe value sits in the first and in the last channel of a 16-channel chunk and in
    the first and the last column of a 32-column block."""
    cin, cout, h, w = 16, 32, 8, 32
    x, idx, classes = sm.probe_tensor(cin, h, w, xscale)
    for sel in (idx[0], idx[15], idx[:, :, 0], idx[:, :, 31]):
        assert set(sel.flatten().tolist()) == set(range(len(classes)))
    wt = sm.centre_identity(cin, cout, k)
    assert sm.wscale(wt) == 4096.0
    out = sm.conv(x, wt, xscale, k)
    keep = torch.tensor([c != "D" for c in classes])[idx]
    assert torch.equal(out[:, :cin].float(), x * keep)
    assert not out[:, cin:].any()
    lossy = sm.conv(x, wt, xscale, k, flush=True)
    changed = torch.tensor([c in "BC" for c in classes])[idx].expand_as(x)
    assert torch.equal(lossy[:, :cin] != out[:, :cin], changed)


def test_weight_scale_rule():
    assert sm.wscale(torch.tensor([1.0, -0.3])) == 4096.0
    assert sm.wscale(torch.tensor([1.0001])) == 2048.0
    assert sm.wscale(torch.tensor([0.2])) == 16384.0                          # 4096 / 0.2 = 20480
    assert sm.wscale(torch.zeros(3)) == 1.0
    w = torch.randn(8, 4, 3, 3, generator=torch.Generator().manual_seed(1))
    for k in (-12, -3, 5):
        assert sm.wscale(w * 2.0 ** k) == sm.wscale(w) * 2.0 ** -k


CASES = [(s, 3) for s in sm.SHAPES_3X3] + [(s, 1) for s in sm.SHAPES_1X1]


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("shape,k", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_float32_accumulation_stays_inside_the_gpu_bound(shape, k, xscale):
    """E(model accumulated in float32) <= 2 E_model + 10 E_plain32 at every magnitude of the sweep: the criterion of the GPU tests holds for the
    arithmetic they are meant to admit (measured: at most 1.00 x (E_model + 10 E_plain32)).  And it has teeth: the same model with f16
    subnormals flushed breaks it at input std 2^-8 and below on either scale, and at std 1 at activation scale 1."""
    cin, cout, h, w = shape
    base, wt = sm.seeded(cin, cout, h, w, k)
    for s in sm.magnitudes(xscale):
        x = base * s
        ref = sm.plain(x.double(), wt.double(), k)
        e_model = sm.E(sm.conv(x, wt, xscale, k), ref)
        e_plain = sm.E(sm.plain(x, wt, k), ref)
        e32 = sm.E(sm.conv(x, wt, xscale, k, acc=torch.float32), ref)
        e_flush = sm.E(sm.conv(x, wt, xscale, k, flush=True), ref)
        bound = 2 * e_model + 10 * e_plain
        print(f"{cin}->{cout} {h}x{w} k{k} xscale {xscale:g} std {s:.1e}: model {e_model:.2e} plain32 {e_plain:.2e} model32 {e32:.2e} "
              f"bound {bound:.2e} flushed {e_flush:.2e}")
        assert e32 <= bound, (s, e32, bound)
        if cin >= 16 and (s <= 2.0 ** -8 or (xscale == 1.0 and s <= 1.0)):
            assert e_flush > bound, (s, e_flush, bound)


def test_error_measures_have_no_floor():
    ref = torch.full((1, 2, 2, 2), 1e-6, dtype=torch.float64)
    ref[:, 1] = 1.0
    a = ref.clone()
    a[0, 0, 0, 0] = 2e-6
    assert sm.E(a * 1e-6, ref * 1e-6) == pytest.approx(1e-6)
    assert sm.E_per_channel(a, ref).tolist() == pytest.approx([1.0, 0.0])
    assert cf.E(a, ref) == sm.E(a, ref)
