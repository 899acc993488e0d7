"""The NaN tracer's helper and case table (tests/nan_tracer.py), on the CPU.

  * the case table is not vacuous: weights and incoming gradients hold no exact zero, and every (case, planted input, plant) has an
    output that is partly NaN in the float64 definition -- the reductions named in ``ALL_OR_NOTHING`` excepted, which must be exactly
    what their name says;
  * three footprints counted by hand for a 3x3 / pad 1 weight gradient;
  * ``expected`` / ``mismatches`` see a footprint that is too wide, too narrow or shifted, and bits lost outside it;
  * the definitions that were changed to select instead of multiply give the values they gave (to torch's float64 autograd)."""
import pytest
import torch

import block_train_f64 as B64
import conv_train_f64 as C64
import nan_tracer as NT


# ------------------------------------------------------------------ the table

def test_table_covers_the_kernel_families():
    families = {name.split("-")[0] for name in NT.CASES}
    assert families == {"conv3x3", "pconv3x3", "scale_bias", "conv1x1", "conv4x4", "conv4x4s2", "bn", "bn_nonzero", "pconv_epilogue", "resample", "instnorm",
                        "l1", "gate", "relu_maxpool", "adam", "spectral"}
    assert all(c.inputs()[k].shape[0] == 2 for c in NT.CASES.values() for k in c.plant if c.inputs()[k].dim() == 4 and k not in ("w",))
    assert any(c.ragged for c in NT.CASES.values())


@pytest.mark.parametrize("name", sorted(NT.CASES))
def test_case_is_not_vacuous(name):
    case = NT.CASES[name]
    inp = case.inputs()
    for key in case.dense:
        NT.assert_dense(inp[key], f"{name} {key}")
    clean = case.ref_clean()
    assert all(not torch.isnan(v).any() for v in clean.values()), "the clean definition holds a NaN"
    runs = case.runs()
    assert runs
    for key, pname, index in runs:
        if key in ("x", "g", "ga", "a", "pred") and inp[key].dim() == 4:
            assert "sample1" in case.plants(key)
        ref = case.ref(case.with_plant(key, index))
        counts = {k: (int(torch.isnan(v).sum()), v.numel()) for k, v in ref.items()}
        for k, v in ref.items():                         # only the outputs the case names hold re-derived elements (it raises otherwise)
            NT.expected(clean[k].float(), v, clean[k], k in case.rederived)
        if (name, key) in NT.ALL_OR_NOTHING or (name, key, pname) in NT.ALL_OR_NOTHING:
            assert all(n in (0, numel) for n, numel in counts.values()), (key, pname, counts)
        else:
            assert NT.partial_somewhere(counts), (key, pname, counts)


# ------------------------------------------------------------------ three footprints by hand

def _dw_case():
    gen = torch.Generator().manual_seed(3)
    return torch.randn(2, 5, 6, 7, generator=gen).double(), torch.randn(2, 4, 6, 7, generator=gen).double()


def test_corner_plant_reaches_four_taps_of_its_input_channel():
    """x[0, ci, 0, 0] is read by tap (ky, kx) at output pixel (1 - ky, 1 - kx): inside the image for ky, kx in {0, 1} only."""
    x, g = _dw_case()
    ci = 3
    dw = C64.conv_dw(NT.planted(x, (0, ci, 0, 0)), g)
    nan = torch.isnan(dw)
    want = torch.zeros_like(nan)
    want[:, ci, :2, :2] = True
    assert torch.equal(nan, want) and int(nan.sum()) == 4 * 4 and not torch.isnan(C64.conv_db(g)).any()


def test_interior_plant_reaches_all_nine_taps_of_its_input_channel():
    x, g = _dw_case()
    ci = 2
    nan = torch.isnan(C64.conv_dw(NT.planted(x, (1, ci, 3, 3)), g))
    want = torch.zeros_like(nan)
    want[:, ci] = True
    assert torch.equal(nan, want) and int(nan.sum()) == 4 * 9


def test_gradient_plant_reaches_its_output_channel_and_its_bias():
    x, g = _dw_case()
    co = 1
    gp = NT.planted(g, (0, co, 2, 5))
    dw, db = torch.isnan(C64.conv_dw(x, gp)), torch.isnan(C64.conv_db(gp))
    assert bool(dw[co].all()) and int(dw.sum()) == 5 * 9 and bool(db[co]) and int(db.sum()) == 1


# ------------------------------------------------------------------ the criterion

def test_expected_and_mismatches():
    clean = torch.arange(12, dtype=torch.float32).view(3, 4) - 5.0
    ref = clean.double().clone()
    ref[1, 2] = NT.NAN
    want, by_value, free = NT.expected(clean, ref)
    assert torch.isnan(want[1, 2]) and int(torch.isnan(want).sum()) == 1 and not by_value.any() and not free.any()
    assert NT.mismatches(want, clean, ref) == (0, 0)
    assert NT.mismatches(clean, clean, ref) == (1, 0)                        # the NaN was swallowed
    wide = want.clone()
    wide[1, 3] = NT.NAN
    assert NT.mismatches(wide, clean, ref) == (1, 0)                         # a footprint one element too wide
    shifted = clean.clone()
    shifted[2, 2] = NT.NAN
    assert NT.mismatches(shifted, clean, ref) == (2, 0)
    moved = want.clone()
    moved[0, 0] += 1e-6
    assert NT.mismatches(moved, clean, ref) == (0, 1)                        # bits lost outside the footprint
    negzero = want.clone()
    negzero[1, 1] = -0.0                                                     # clean[1, 1] is +0: the bits differ
    assert NT.mismatches(negzero, clean, ref) == (0, 1)
    with pytest.raises(AssertionError):
        NT.check("shifted", shifted, clean, ref)
    NT.check("right", want, clean, ref)


def test_a_value_the_definition_moves_is_taken_from_the_definition():
    clean = torch.tensor([1.5, -2.0, 3.25], dtype=torch.float32)
    ref_clean = clean.double()
    ref = torch.tensor([1.5, 0.0, NT.NAN], dtype=torch.float64)              # a gate closed by the plant, a NaN
    want, by_value, free = NT.expected(clean, ref, ref_clean)
    assert by_value.tolist() == [False, True, False] and want[1] == 0 and torch.isnan(want[2]) and not free.any()
    assert NT.mismatches(torch.tensor([1.5, -0.0, NT.NAN]), clean, ref, ref_clean) == (0, 0)       # either zero
    assert NT.mismatches(torch.tensor([1.5, -2.0, NT.NAN]), clean, ref, ref_clean) == (0, 1)
    rederived = torch.tensor([1.5, 0.1, 3.25], dtype=torch.float64)
    with pytest.raises(AssertionError, match="float32 does not hold"):
        NT.expected(clean, rederived, ref_clean)
    assert NT.expected(clean, rederived, ref_clean, rederived=True)[2].tolist() == [False, True, False]
    assert NT.mismatches(torch.tensor([1.5, 7.0, 3.25]), clean, rederived, ref_clean, rederived=True) == (0, 0)        # finite: all that is asked
    assert NT.mismatches(torch.tensor([1.5, NT.NAN, 3.25]), clean, rederived, ref_clean, rederived=True) == (1, 0)


def test_gather_form_of_the_4x4_backward_is_the_scatter_form_on_finite_values():
    import disc_f64 as D64
    gen = torch.Generator().manual_seed(4)
    for s, H, W in ((2, 33, 20), (1, 33, 20), (2, 5, 7), (1, 4, 4)):
        g = torch.randn(2, 5, D64.out_size(H, s), D64.out_size(W, s), generator=gen, dtype=torch.float64)
        w = torch.randn(5, 3, 4, 4, generator=gen, dtype=torch.float64)
        a, b = NT.conv4_backward_data(g, w, s, H, W), D64.conv_backward_data(g, w, s, H, W)
        assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())


def test_plants():
    p = NT.plants((2, 40, 33, 20))
    assert p["origin"] == (0, 0, 0, 0) and p["last"] == (1, 39, 32, 19) and p["sample1"] == (1, 0, 0, 0) and p["last_channel"][1] == 39
    assert 0 < p["interior"][2] < 32 and 0 < p["interior"][3] < 19
    assert "sample1" not in NT.plants((1, 8, 4, 4))
    t = torch.ones(2, 3, 4, 5)
    assert int(torch.isnan(NT.planted(t, p["origin"])).sum()) == 1 and not torch.isnan(t).any()
    assert int(torch.isnan(NT.planted(t, [(0, 0, 0, 0), (1, 2, 3, 4)])).sum()) == 2


# ------------------------------------------------------------------ the definitions that select now

def test_selecting_gate_is_autograds_gradient():
    N, C, H, W = 2, 6, 5, 7
    mask = C64.holed_mask(N, H, W, seed=5).double()
    x, gain, bias, ga = (t.double() for t in B64.bn_inputs(N, C, H, W, seed=11, mask=mask.float()))
    xa, ka, ba = (t.clone().requires_grad_(True) for t in (x, gain, bias))
    a = B64.bn_train(xa, mask, ka, ba)[0]
    want = torch.autograd.grad(a, (xa, ka, ba), ga)
    got = B64.bn_train_grads(x, mask, gain, bias, ga)
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= 1e-11 * float(w.abs().max())
    # a NaN arriving at a closed gate stops there, as in torch
    closed = (B64.bn_gate(x, *B64.bn_tables(*B64.bn_stats(x, mask)[:2], gain, bias), mask)[0] <= 0).nonzero()[0]
    gp = NT.planted(ga, tuple(int(v) for v in closed))
    assert not any(torch.isnan(t).any() for t in B64.bn_train_grads(x, mask, gain, bias, gp))
    assert not any(torch.isnan(t).any() for t in torch.autograd.grad(B64.bn_train(xa, mask, ka, ba)[0], (xa, ka, ba), gp))
    # the per-element mask's definition selects too
    import decoder_train_f64 as G64
    xz = x * G64.keep_pattern(N, C, H, W, seed=3, zero_channel=False).double()
    xa, ka, ba = (t.clone().requires_grad_(True) for t in (xz, gain, bias))
    want = torch.autograd.grad(G64.bn_nz_train(xa, ka, ba)[0], (xa, ka, ba), ga)
    got = G64.bn_nz_train_grads(xz, gain, bias, ga)
    for g, w in zip(got, want):
        assert float((g - w).abs().max()) <= 1e-11 * float(w.abs().max())
    scale, shift = B64.bn_tables(*G64.bn_nz_stats(xz)[:2], gain, bias)
    closed = (((xz * B64._t(scale) - B64._t(shift)) <= 0) | (xz == 0)).nonzero()[0]
    gp = NT.planted(ga, tuple(int(v) for v in closed))
    assert not any(torch.isnan(t).any() for t in G64.bn_nz_train_grads(xz, gain, bias, gp))
    assert not any(torch.isnan(t).any() for t in torch.autograd.grad(G64.bn_nz_train(xa, ka, ba)[0], (xa, ka, ba), gp))


@pytest.mark.parametrize("plant", sorted(NT.ITERATION_PLANTS))
def test_whole_iteration_diverges_in_float64(plant):
    """The whole iteration is the one case that is all-NaN by definition: a NaN pixel or decoder weight reaches every loss entry and,
    through the batch statistics and the spectral norm, every parameter's update.  The clean iteration holds none.  Both plants make
    everything NaN in float64, so the device test of this case reduces to "everything NaN": it proves propagation through the whole
    chain (the loss cannot stay finite over a dead network), not a footprint -- the footprints are the case table's."""
    losses, after = NT.iteration_ref(*NT.iteration_case(plant))
    assert len(losses) == 5 and len(after) == 141
    assert all(bool(torch.isnan(v)) for v in losses.values()) and all(bool(torch.isnan(v).all()) for v in after.values())
    if plant == "pixel":
        losses, after = NT.iteration_ref(*NT.iteration_case(None))
        assert not any(bool(torch.isnan(v)) for v in losses.values()) and not any(bool(torch.isnan(v).any()) for v in after.values())
