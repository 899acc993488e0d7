"""tests/wino_model.py (F(2x2, 3x3) written out: the CPU model of csrc/conv_wino.hpp) against the written-out plain convolution of
tests/conv_train_f64.py: equal in float64, exact in float32 on the integer probes the GPU test demands bit equality on, and its float32 error
next to a plain float32 convolution's on the GPU test's accuracy inputs (printed with -s)."""
import pytest
import torch

import conv_train_f64 as cf
import wino_model as wm


def test_case_table_covers_every_value_and_every_cin_meets_both_grids():
    cins, couts, sizes, ns = (3, 16, 24, 40, 64, 72, 256, 272), (5, 8, 64, 72, 136), wm.RAGGED + wm.EVEN, (1, 3)
    assert {c[0] for c in wm.CASES} == set(cins) and {c[1] for c in wm.CASES} == set(couts)
    assert {c[2:4] for c in wm.CASES} == set(sizes) and {c[4] for c in wm.CASES} == set(ns)
    for cin in cins:
        grids = {c[2:4] for c in wm.CASES if c[0] == cin}
        assert grids & set(wm.RAGGED) and grids & set(wm.EVEN), cin
    for line, case in zip([ln for ln in wm.__doc__.splitlines() if ln[:6].strip().isdigit()], wm.CASES):       # the table IS the list
        f = line.split()
        assert (int(f[1]), int(f[2]), *map(int, f[3].split("x")), int(f[4])) == case, line
    assert sum(ln[:6].strip().isdigit() for ln in wm.__doc__.splitlines()) == len(wm.CASES)


@pytest.mark.parametrize("case", wm.CASES, ids=wm.CASE_IDS)
def test_float64_model_equals_the_plain_convolution(case):
    for variant in wm.VARIANTS:
        d = wm.dense_inputs(case, variant)
        for mode in wm.modes(case):
            ref, got = wm.reference(d, mode, torch.float64, cf.conv), wm.reference(d, mode, torch.float64, wm.conv)
            assert got.shape == ref.shape and wm.E(got, ref) <= 1e-12, (variant, mode, wm.E(got, ref))


@pytest.mark.parametrize("case", wm.CASES, ids=wm.CASE_IDS)
def test_integer_probes_are_exact_in_float32(case):
    """The float32 model returns the float64 convolution bit for bit on the integer probes: every operation of the algorithm is exact there,
    so a kernel that is not bit-equal on them is wrong, not differently rounded."""
    d = wm.exact_inputs(case)
    u = wm.weights(d["w"], torch.float32)
    assert torch.equal(u, u.round()) and float(u.abs().max()) <= 36 and torch.equal(u.double(), wm.weights(d["w"], torch.float64))
    for mode in wm.modes(case):
        ref = wm.reference(d, mode, torch.float64, cf.conv)
        got = wm.reference(d, mode, torch.float32, wm.conv)
        assert float(ref.abs().max()) < 2.0 ** 24 and torch.equal(got.double(), ref), mode
        assert torch.equal(wm.reference(d, mode, torch.float32, cf.conv).double(), ref), mode


@pytest.mark.parametrize("cin,cout,h,w", wm.ONE_HOT_SHAPES)
def test_one_hot_probes_are_exact_in_float32_and_land_where_the_tap_says(cin, cout, h, w):
    for tap in [None] + cf.TAPS:
        x, wt, names = wm.one_hot_inputs(cin, cout, h, w, tap)
        assert len(names) >= 10 and int((x != 0).sum()) == len(names)
        ref = cf.conv(x.double(), wt.double())
        assert torch.equal(wm.conv(x, wt).double(), ref)
        if tap is not None:                              # pixel (y, x) through tap (ky, kx) lands at (y - ky + 1, x - kx + 1), or outside
            for p, (y, xx) in enumerate(wm.one_hot_pixels(h, w).values()):
                oy, ox = y - tap[0] + 1, xx - tap[1] + 1
                hit = ref[p].abs().sum(0) != 0
                assert int(hit.sum()) == (1 if 0 <= oy < h and 0 <= ox < w else 0)
                assert not hit.any() or bool(hit[oy, ox])


@pytest.mark.parametrize("case", wm.CASES, ids=wm.CASE_IDS)
def test_float32_error_of_the_model_next_to_the_plain_convolution(case):
    """E_wino32 and E_plain32 against float64 on the accuracy inputs of the GPU test (figures: -s).  An fp32 Winograd is a small factor worse
    than a plain fp32 convolution, never orders of magnitude: E_wino32 <= 10 E_plain32 + 1e-6, the bound the GPU kernel is held to."""
    for variant in wm.VARIANTS:
        d = wm.dense_inputs(case, variant)
        for mode in wm.modes(case):
            ref = wm.reference(d, mode, torch.float64, cf.conv)
            e_plain, e_wino = wm.E(wm.reference(d, mode, torch.float32, cf.conv), ref), wm.E(wm.reference(d, mode, torch.float32, wm.conv), ref)
            print(f"model {wm.CASE_IDS[wm.CASES.index(case)]} {variant} {mode}: E_plain32 {e_plain:.2e} E_wino32 {e_wino:.2e} ratio {e_wino / e_plain:.2f}")
            assert e_wino <= 10 * e_plain + 1e-6
