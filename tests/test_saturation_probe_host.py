"""The probe plans of tests/saturation_probe.py, checked on the CPU: that they reach what they claim to reach, and that "report" means "the
result is wrong".

The staging-round mapping under test (csrc/conv.hip, "Staging of a chunk"): a workgroup stages the 10 x 34 halo block of its 8 x 32 tile, halo pixel
p = (y - y0 + 1) * 34 + (x - x0 + 1); p < 256 is staged in round 0 (channels 0-7 of the 16-channel chunk) and round 1 (channels 8-15), p >= 256 in
round 2 (work-items < 168: pixel 256 + tid % 84, group tid / 84).  For the tile at the image origin p >= 256 is image row 6 from column 17 on and
rows 7 and 8."""
import math

import pytest
import torch

import saturation_probe as sp
import split_model as sm
from metrics_fixture import to_blocked

TILE_CASES = [c for c in sp.CASES if c.plan in ("tile", "mainx", "skipx16")]
ids = lambda cs: [c.name for c in cs]


def operand_shape(case, buf):
    return (case.N, case.cin if buf == "x" else sp.skip_cin(case), case.H, case.W)


def test_round_mapping_of_the_origin_tile():
    for y in range(9):
        for x in range(33):
            for c in (0, 7, 8, 15, 16, 39):
                own = [r for (ty, tx, _), r in zip(sp.stagings(y, x, 9, 33), sp.rounds(c, y, x, 9, 33)) if (ty, tx) == (0, 0)]
                late = y > 6 or (y == 6 and x >= 17)
                assert own == [2 if late else (c % 16) // 8], (c, y, x, own)
    assert sp.stagings(6, 20, 9, 33) == [(0, 0, 7 * 34 + 21)]                       # isolated: one tile, round 2
    assert sorted(t[:2] for t in sp.stagings(7, 31, 9, 33)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert len({p for y in range(-1, 9) for x in range(-1, 33) for _, _, p in sp.stagings(y, x, 8, 32)} - set(range(340))) == 0


def test_blocked_address_is_the_layout_of_to_blocked():
    for shape in ((2, 16, 8, 32), (1, 40, 9, 33), (1, 24, 10, 13)):
        n = shape[0] * shape[1] * shape[2] * shape[3]
        x = torch.arange(n, dtype=torch.float32).view(shape)
        flat = to_blocked(x).contiguous().view(-1)
        for idx in ((0, 0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1, shape[3] - 1), (0, 9, 3, 7), (shape[0] - 1, 13, 6, 12)):
            assert flat[sp.flat_index(shape, *idx, True)] == x[idx]
            assert x.view(-1)[sp.flat_index(shape, *idx, False)] == x[idx]


@pytest.mark.parametrize("xscale", sp.SCALES)
@pytest.mark.parametrize("case", sp.CASES, ids=ids(sp.CASES))
def test_every_planned_verdict_is_the_definitions(case, xscale):
    """The plan's expectation equals the verdict of ``staged`` in float32 and in float64 (sp.verdicts asserts the twins agree and that exactly one of
    must_report / must_be_silent holds); the clean tensors are silent under the whole-tensor definition; every plan has report and silent probes
    and its schedule has controls: launches with no change at all, the first, the last and every eighth."""
    plan = sp.case_plan(case, xscale)
    pre, mask = sp.case_pre(case), sp.case_mask(case)
    for buf in ("x", "skip"):
        sub = [p for p in plan if p.buf == buf]
        assert sp.verdicts(sub, pre, mask, xscale) == [p.report for p in sub]
        for p in sub:
            assert p.n < case.N and p.c < operand_shape(case, buf)[1] and p.y < case.H and p.x < case.W
    for dtype in (torch.float32, torch.float64):
        assert sp.must_be_silent(sp.staged(sp.case_base(case), pre, mask, xscale, dtype))
    assert any(p.report for p in plan) and any(not p.report for p in plan)
    sched = sp.schedule(plan)
    assert sched[0] is None and sched[-1] is None and [p for p in sched if p is not None] == plan
    assert all(sched[i] is None for i in range(0, len(sched) - 1, 8))
    # the boundary itself: at scale 64 +-1023 reports and nextafter(+-1023, 0) is silent; at scale 1 +-65472 and its inward neighbour
    if pre is None or any(p.buf == "skip" for p in plan):
        t = sp.T / xscale
        vals = {(p.value, p.report) for p in plan if p.buf == "skip" or pre is None}
        assert {(t, True), (-t, True), (sp.inward(t), False), (sp.inward(-t), False)} <= vals
    else:
        t = (sp.T / xscale + 0.5) / 2.0                                             # 511.75 at scale 64
        assert {(t, True), (sp.inward(t), False)} <= {(p.value, p.report) for p in plan if mask is None or float(mask[p.n, 0, p.y, p.x])}


@pytest.mark.parametrize("case", TILE_CASES, ids=ids(TILE_CASES))
def test_exhaustive_plans_touch_every_pixel_and_group_of_a_tile(case):
    """Every (pixel, 8-channel group) of the 8 x 32 tile carries a report probe and a silent one (at a masked pixel of the explicit-mask prologue:
    two silent ones), all eight channels of a group are met, and every staging round has report and silent probes that ISOLATE it."""
    plan = sp.case_plan(case, 64.0)
    buf = "skip" if case.plan == "skipx16" else "x"
    mask = sp.case_mask(case) if case.mode == "bn_mask" else None
    seen = {}
    for p in plan:
        if p.buf == buf and p.kind in ("edge", "beyond", "silent", "masked"):
            seen.setdefault((p.y, p.x, p.c // 8), []).append(p.report)
    assert set(seen) == {(y, x, g) for y in range(8) for x in range(32) for g in range(2)}
    for (y, x, g), v in seen.items():
        masked = mask is not None and float(mask[0, 0, y, x]) == 0.0
        assert (len(v) >= 2 and not any(v)) if masked else sorted(v) == [False, True], (y, x, g, v)
    assert {p.c for p in plan if p.buf == buf} == set(range(16))
    if buf == "x":                                                                  # (the skip phase stages the block's own 256 pixels in one go)
        for rnd in (0, 1, 2):
            iso = [p for p in plan if p.kind in ("edge", "beyond", "silent") and sp.rounds(p.c, p.y, p.x, case.H, case.W) == [rnd]]
            assert any(p.report for p in iso) and any(not p.report for p in iso), rnd
            signs = {1.0, -1.0} if sp.case_pre(case) is None else {1.0}            # (a ReLU prologue removes negative values: positive only)
            for kind in ("edge", "beyond", "silent"):                               # neither sign nor kind is tied to a staging round
                assert {math.copysign(1.0, p.value) for p in iso if p.kind == kind} == signs, (rnd, kind)


def test_ragged_plans_fall_in_chunks_0_1_2_and_in_every_round():
    for case in (c for c in sp.CASES if c.plan == "ragged"):
        plan = sp.case_plan(case, 64.0)
        for ch in (0, 1, 2):
            for rep in (True, False):
                assert any(sp.chunk(p.c) == ch and p.report == rep for p in plan)
        assert {p.c for p in plan} == set(range(40))
        for rnd in (0, 1, 2):                                                       # per chunk: a probe that only this round of one tile stages
            for ch in ((0, 1) if rnd == 1 else (0, 1, 2)):                              # (chunk 2 holds channels 32-39: its second group is padding)
                for rep in (True, False):
                    assert any(p.report == rep and p.kind != "masked" and sp.chunk(p.c) == ch and sp.rounds(p.c, p.y, p.x, 9, 33) == [rnd]
                               for p in plan), (case.name, rnd, ch, rep)
        px = {(p.y, p.x) for p in plan}
        assert {(7, 31), (7, 32), (8, 31), (8, 32), (8, 0), (0, 32)} <= px
        assert any(len(sp.stagings(y, x, 9, 33)) == 4 for y, x in px)


def test_lattice_keeps_boundaries_corners_and_seams():
    px = set(sp.lattice_pixels(16, 64))
    for y0 in (0, 8):
        for x0 in (0, 32):
            assert {(y0, x0), (y0, x0 + 31), (y0 + 7, x0), (y0 + 7, x0 + 31), (y0 + 6, x0 + 16), (y0 + 6, x0 + 17), (y0 + 5, x0 + 31)} <= px
    assert {(7, 31), (7, 32), (8, 31), (8, 32), (15, 63), (0, 63), (15, 0)} <= px
    for case in (c for c in sp.CASES if c.plan == "lattice"):
        plan = sp.case_plan(case, 64.0)
        for buf in ("x", "skip"):
            assert {(p.y, p.x, p.c // 8) for p in plan if p.buf == buf} == {(y, x, g) for y, x in px for g in (0, 1)}
        for rnd in (0, 1, 2):
            assert any(p.buf == "x" and p.report and sp.rounds(p.c, p.y, p.x, 16, 64) == [rnd] for p in plan)


def test_1x1_plans_cover_channels_and_pixels():
    for case in (c for c in sp.CASES if c.plan == "1x1"):
        plan = sp.case_plan(case, 64.0)
        hw = case.H * case.W
        assert hw == 130
        for pix in (0, 31, 32, 127, 128, 129):
            assert {p.c for p in plan if p.y * case.W + p.x == pix and p.report} == set(range(case.cin))
        for c in (0, case.cin - 1):
            assert {p.y * case.W + p.x for p in plan if p.c == c and p.report} == set(range(hw))
            assert {p.y * case.W + p.x for p in plan if p.c == c and not p.report} == set(range(hw))


def thinned(plan, buf, limit=160):
    """About ``limit`` evenly spaced standard probes (an odd stride: reports and their silent neighbours alternate in a plan) of one operand of a plan, and every probe of another kind (what the prologue moves)."""
    std = [p for p in plan if p.buf == buf and p.kind in ("edge", "beyond", "silent")]
    return std[::max(len(std) // limit, 1) | 1] + [p for p in plan if p.buf == buf and p.kind not in ("edge", "beyond", "silent")]


@pytest.mark.parametrize("xscale", sp.SCALES)
@pytest.mark.parametrize("case", sp.CASES, ids=ids(sp.CASES))
def test_report_means_wrong_and_silent_means_untouched(case, xscale):
    """split_model.conv carries the clamp of stage_value, saturation_probe.conv_unclamped does not.  On the outputs a probe reaches (the crop around
    it): at every silent probe the two are equal bit for bit -- the clamp did nothing; at every report probe BEYOND the boundary they differ at some
    output -- the clamp changed the result: "report" means "wrong", not merely "large".  At an EDGE probe (|staged| == 65472 exactly) the clamp is
    the identity and the two are equal: the kernel, which tests after the clamp, reports there all the same; that report is conservative (it costs
    a re-render one rung up, never a wrong frame) and the contract's ">= 65472" includes it.
    Every case and both operands of the fused forms (the skip operand: its 1x1 convolution); the exhaustive plans thinned to ~160 evenly spaced
    probes per operand -- the staging arithmetic of an element does not depend on its pixel, only the kernel's path to it does, and that is the
    GPU test's subject -- with every probe of the prologue's own kinds kept."""
    plan = sp.case_plan(case, xscale)
    counts = {"silent": 0, "edge": 0, "beyond": 0}
    for buf in ("x", "skip"):
        probes = thinned(plan, buf)
        if not probes:
            continue
        pre, mask = (sp.case_pre(case), sp.case_mask(case) if case.mode == "bn_mask" or case.mode == "bn_nonzero" else None) if buf == "x" else (None, None)
        k = 1 if (case.kind == "conv1" or buf == "skip") else 3
        R = k // 2
        cin = case.cin if buf == "x" else sp.skip_cin(case)
        wt = sp.seeded_weight(case.cout, cin, k, 0 if buf == "x" else 1)
        base = sp.case_base(case, buf)
        pad = lambda t: torch.nn.functional.pad(t, (2 * R,) * 4)
        bp, mp = pad(base), None if mask is None else pad(mask)
        X = torch.stack([bp[p.n, :, p.y:p.y + 4 * R + 1, p.x:p.x + 4 * R + 1] for p in probes]).clone()
        for i, p in enumerate(probes):
            X[i, p.c, 2 * R, 2 * R] = p.value
        M = None if mask is None else torch.stack([mp[p.n, :, p.y:p.y + 4 * R + 1, p.x:p.x + 4 * R + 1] for p in probes])
        xe = sp.convolved(X, pre, M)
        centre = (slice(None), slice(None), slice(R, 3 * R + 1), slice(R, 3 * R + 1))
        a, b = sm.conv(xe, wt, xscale, k)[centre], sp.conv_unclamped(xe, wt, xscale, k)[centre]
        for i, p in enumerate(probes):
            same = torch.equal(a[i], b[i])
            at_edge = float(sp.staged(X[i:i + 1], pre, None if M is None else M[i:i + 1], xscale).abs().max()) == sp.T
            if not p.report:
                assert same, p
                counts["silent"] += 1
            elif at_edge:
                assert same and p.kind == "edge", p
                counts["edge"] += 1
            else:
                assert not same, p
                counts["beyond"] += 1
    assert counts["silent"] and counts["edge"] and (counts["beyond"] or xscale == 1.0), counts


def test_crop_references_equal_whole_tensor_references():
    """The float64 / model / plain32 outputs the GPU test pastes from crops are the whole-tensor ones (float64 and model: to 1e-12 of the output
    scale -- the channel sum may be ordered differently; this is not a tolerance of the GPU test)."""
    case = next(c for c in sp.CASES if c.name == "3x3-nchw-bn_nonzero-co32-tile")
    pre, mask = sp.case_pre(case), sp.case_mask(case)
    wt, base = sp.seeded_weight(case.cout, case.cin, 3, 0), sp.case_base(case)
    plan = [p for p in sp.case_plan(case, 64.0) if not p.report]
    for p in plan[::97] + [q for q in plan if q.kind == "derived-nonzero"]:
        x = sp.apply(base, p)
        xe = sp.convolved(x, pre, mask)
        whole = sm.plain(xe.double(), wt.double(), 3)
        X = torch.nn.functional.pad(x, (2,) * 4)[:, :, p.y:p.y + 5, p.x:p.x + 5]
        crop = sm.plain(sp.convolved(X, pre, None).double(), wt.double(), 3)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= p.y + dy < case.H and 0 <= p.x + dx < case.W:
                    d = (whole[0, :, p.y + dy, p.x + dx] - crop[0, :, 2 + dy, 2 + dx]).abs().max()
                    assert float(d) <= 1e-12 * float(whole.abs().max())
        far = torch.ones(case.H, case.W, dtype=torch.bool)
        far[max(p.y - 1, 0):p.y + 2, max(p.x - 1, 0):p.x + 2] = False
        clean = sm.plain(sp.convolved(base, pre, mask).double(), wt.double(), 3)
        assert torch.equal(whole[0][:, far], clean[0][:, far])
