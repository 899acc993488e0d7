"""The range detector of the split-f16 convolutions, element by element on every path (csrc/conv.hip: stage_value in its three staging rounds
and every chunk position, the fused skip phase, the resampling forms, conv1x1_split_kernel; nets.SaturationLog; pipeline._render).

The promise under test (nets.check_saturation): a split-f16 convolution that clamps an activation returns a wrong frame, and that is never
silent -- the device counter moves.  Every launch here differs from a clean seeded randn tensor in exactly ONE element, so exactly one staging
item of one wave has to notice; whether it must is decided by the written-out definition tests/saturation_probe.py (``staged``, float32 and
float64 twins), never by the kernel.  tests/test_saturation_probe_host.py checks the plans themselves on the CPU.

Mechanics of a case: write the element, launch, SaturationLog.mark(), restore the element; every eighth launch is a control on the untouched
tensor; ONE host synchronisation (log.bad()).  Asserted: bad() == the planned report set, no more and no less (a failure lists the offending probes
as (operand, n, c, y, x, value, staging rounds, chunk, kind)); at every silent probe the output of that launch is held to float64 by the family's own
criterion -- E_gpu <= 2 E_model + 10 E_plain32 against tests/split_model.py (test_gpu_conv_range.py) for the plain, prologue, partial and 1x1
families; the fused-skip, pool and up forms against their staged composition as test_skip_branch_inside_the_second_convolution compares them
(2e-6 of the output scale; pool 1e-6; up bit-identical) --; at every report probe the output is finite.  Activation scale 64: the full plan;
scale 1: the exact-boundary pairs of every path.

Shapes (the smallest at which each mechanism exists; tests/saturation_probe.py: CASES):
  3x3, Cout 32 / 64 / 128 (WCO 1 / 2 / 4) x NCHW / channel-blocked x no prologue / BN / BN + mask / BN + derived mask: [1,16,8,32] EXHAUSTIVE (256
     pixels x 2 channel groups x {report, silent neighbour}, no lattice: a case takes 0.1 - 0.6 s); [1,40,9,33] (3 chunks, 4 tiles): all 40 channels
     at one pixel per staging round, at the tile seams and in the last row and column; [2,16,8,32]: sample 1 only.
  fused skip, Cout 32 / 64 / 128, Conv.forward_skip without / with the second convolution's prologue and PartialConv.forward_skip: probes in skip_x
     only (skip_cin 16 exhaustive; 40: all channels at four pixels) and in the main input only; the other operand stays clean.
  pool / up forms, Cout 128, [1,16,16,64]: the lattice saturation_probe.lattice_pixels (every tile corner, seam neighbour and round-2 boundary) in
     both operands.
  1x1, NCT 1 / 2 / 4, NCHW (Cin 16, 32, 40) and blocked (24, 16, 40), HW = 130: every channel at pixels 0, 31, 32, 127, 128, 129, every pixel at
     channels 0 and Cin - 1.
  controls that never report: the <= 4-channel kernel and everything inside nets.fp32_kernels() -- the exhaustive 3x3 cases direct and Winograd, the
     1x1 cases, the fused skip / pool / up forms at Cout 128 -- on 32 out-of-range probes of each case's own plan (16 report probes per scale).
Every test prints its counts (-s); profiles/conv_saturation.txt is that output."""
import time
import types
import warnings

import pytest
import torch

import conv_train_f64 as cf
import saturation_probe as sp
import split_model as sm
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


# ---------------------------------------------------------------------------------------------------------------- one case on the device

def zero_bias(mod):
    with torch.no_grad():
        if mod.bias is not None:
            mod.bias.zero_()
    return mod


def setup(nets, case):
    """The modules and device tensors of a case -> namespace with bufs / clean (kernel layout, by operand), launch() -> device output in kernel
    layout, composition() -> the staged composition of the fused forms (or None), k, wt (the probed convolution's weights)."""
    r = types.SimpleNamespace(case=case, composition=None)
    cin, cout, blocked = case.cin, case.cout, case.blocked
    lay = (nets.IN_B8 | nets.OUT_B8) if blocked else 0
    r.k = 1 if case.kind == "conv1" else 3
    r.wt = sp.seeded_weight(cout, cin, r.k, 0)
    r.mask, r.pre = sp.case_mask(case), sp.case_pre(case)
    partial = case.mode in ("bn_mask", "bn_nonzero", "pconv")
    mod = zero_bias((nets.PartialConv if partial else nets.Conv)(cin, cout, r.k).cuda())
    with torch.no_grad():
        mod.weight.copy_(r.wt)
    r.mod = mod
    r.base = {"x": sp.case_base(case, "x")}
    pre = None if r.pre is None else (r.pre[0].cuda(), r.pre[1].cuda())
    mask = None if r.mask is None else r.mask.cuda()
    if case.kind in ("skip", "pool", "up"):
        scin = sp.skip_cin(case)
        r.base["skip"] = sp.case_base(case, "skip")
        skip = zero_bias(nets.Conv(scin, cout, 1, bias=not partial).cuda())
        with torch.no_grad():
            skip.weight.copy_(sp.seeded_weight(cout, scin, 1, 1))
    r.clean = {b: (to_blocked(t) if blocked else t).cuda().contiguous() for b, t in r.base.items()}
    r.bufs = {b: t.clone() for b, t in r.clean.items()}
    x = r.bufs["x"]
    if case.kind in ("conv3", "conv1"):
        if case.mode == "bn_mask":
            r.launch = lambda: mod(x, mask, pre_bn=pre, layout=lay)[0]
        elif case.mode == "bn_nonzero":
            r.launch = lambda: mod(x, None, pre_bn=pre)[0]
        else:
            r.launch = lambda: mod(x, pre, layout=lay)
        return r
    sx = r.bufs["skip"]
    pool = {"skip": False, "pool": True, "up": "Up"}[case.kind]

    def fused(pool):
        if partial:
            return mod.forward_skip(x, mask, sx, skip, layout=lay, skip_b8=True, pool=pool)[0]
        return mod.forward_skip(x, pre, sx, skip, layout=lay, skip_b8=True, pool=pool)

    def two_kernels():                                   # nets.staged_skips(): 1x1 kernel -> residual of the 3x3 epilogue
        b = skip(sx, layout=lay)
        if partial:
            return mod(x, mask, residual=b, layout=lay | nets.RES_B8)[0]
        return mod(x, pre, residual=b, layout=lay | nets.RES_B8)

    r.launch = lambda: fused(pool)
    if case.kind == "skip":
        r.composition = two_kernels
    else:                                                # nets.staged_skips(pools_only=True): fused skip, resampling kernel
        r.composition = lambda: (nets.avgpool_down if case.kind == "pool" else nets.upsample_up)(fused(False), True)
    return r


def drive(nets, r, sched):
    """Run the schedule.  -> (indices of the launches during which the counter moved, {launch: output} of the silent probes, {launch: composition
    output}, {launch: all-finite flag (device)} of the report probes, indices of the composition launches that moved the counter)."""
    case = r.case
    flat = {b: t.view(-1) for b, t in r.bufs.items()}
    clean = {b: t.view(-1) for b, t in r.clean.items()}
    shapes = {b: tuple(t.shape) for b, t in r.base.items()}
    log = nets.SaturationLog(torch.device(DEV), 2 * len(sched))
    slots, kept, comp, finite = [], {}, {}, {}
    with torch.no_grad():
        for i, p in enumerate(sched):
            if p is not None:
                assert all(0 <= v < m for v, m in zip((p.n, p.c, p.y, p.x), shapes[p.buf])), p
                at = sp.flat_index(shapes[p.buf], p.n, p.c, p.y, p.x, case.blocked)
                flat[p.buf][at:at + 1].fill_(p.value)
            out = r.launch()
            log.mark()
            slots.append(("probe", i))
            if p is None or not p.report:
                kept[i] = out
                if r.composition is not None and p is not None:
                    comp[i] = r.composition()
                    log.mark()
                    slots.append(("composition", i))
            else:
                finite[i] = torch.isfinite(out).all()
            if p is not None:
                flat[p.buf][at:at + 1].copy_(clean[p.buf][at:at + 1])
    bad = log.bad()                                      # the one host synchronisation
    moved = [slots[b] for b in bad]
    return [i for tag, i in moved if tag == "probe"], kept, comp, finite, [i for tag, i in moved if tag == "composition"]


def logical(case, t):
    t = t.cpu()
    return from_blocked(t) if case.blocked else t


# ---------------------------------------------------------------------------------------------------------------- float64 at the silent probes

def partial_out(raw, mplane, mscale, cin):
    """(raw * ratio + 0) * um of the partial convolution in the dtype of ``raw`` for the mask plane ``mplane`` (tests/conv_train_f64.py:
    partial_factors, with conv(mask, ones) = box3x3(mplane) * mscale)."""
    mp = mplane.to(raw.dtype)
    box = sum(cf.shifted(mp, ky - 1, kx - 1) for ky, kx in cf.TAPS) * mscale
    um = box.clamp(0, 1)
    return raw * ((9.0 * cin) / (box + 1e-8) * um) * um


def three(case, wt, x, mask, pre, xscale, k):
    """(model, ref64, plain32) of the case's layer on the logical input ``x`` (any spatial size: the crops below)."""
    xe = sp.convolved(x, pre, mask)
    outs = [sm.conv(xe, wt, xscale, k), sm.plain(xe.double(), wt.double(), k), sm.plain(xe, wt, k)]
    if case.mode == "bn_mask":
        outs = [partial_out(o, mask, float(case.cin), case.cin) for o in outs]
    elif case.mode == "bn_nonzero":
        mp = (x != 0).sum(1, keepdim=True).float()
        outs = [partial_out(o, mp, 1.0, case.cin) for o in outs]
    return outs


def references(r, probes, xscale):
    """[(model, ref64, plain32)] of the launches ``probes`` (None: the clean tensor), each [N,Cout,H,W].  An element reaches the (2R+1)^2
    outputs around it (R = k // 2): those come from the (4R+1)^2 crop of the input around the element, everything else from the clean tensor's
    outputs (tests/test_saturation_probe_host.py holds this against the whole-tensor computation)."""
    case, k, R = r.case, r.k, r.k // 2
    base, mask = r.base["x"], r.mask
    clean = three(case, r.wt, base, mask, r.pre, xscale, k)
    real = [p for p in probes if p is not None]
    if real:
        pad = lambda t: torch.nn.functional.pad(t, (2 * R,) * 4)
        bp, mp = pad(base), None if mask is None else pad(mask)
        win = lambda t, p: t[p.n, :, p.y:p.y + 4 * R + 1, p.x:p.x + 4 * R + 1]
        X = torch.stack([win(bp, p) for p in real]).clone()
        for i, p in enumerate(real):
            X[i, p.c, 2 * R, 2 * R] = p.value
        M = None if mask is None else torch.stack([win(mp, p) for p in real])
        crops = three(case, r.wt, X, M, r.pre, xscale, k)
    out, j = [], 0
    for p in probes:
        if p is None:
            out.append(clean)
            continue
        full = [t.clone() for t in clean]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if 0 <= p.y + dy < case.H and 0 <= p.x + dx < case.W:
                    for f, c in zip(full, crops):
                        f[p.n, :, p.y + dy, p.x + dx] = c[j, :, 2 * R + dy, 2 * R + dx]
        out.append(full)
        j += 1
    return out


RUNGS = {"few": lambda nets: nets.activation_scale(64.0), "fp32": lambda nets: nets.fp32_kernels(winograd=False),
         "fp32-winograd": lambda nets: nets.fp32_kernels(winograd=True)}


def judge_silent(r, sched, kept, comp, xscale, rung=None):
    """The accuracy assertion at the silent launches -> (worst figure, its probe).  ``rung`` (the controls: fp32 arithmetic): E_gpu <= 10 E_plain32
    (test_gpu_conv_range.py: test_fp32_controls_are_scale_free), + 1e-6 for Winograd (test_gpu_conv_wino.py)."""
    case = r.case
    worst, failures = (0.0, None), []
    if r.composition is None:
        idx = sorted(kept)
        refs = references(r, [sched[i] for i in idx], xscale)
        for i, (model, ref, p32) in zip(idx, refs):
            out = logical(case, kept[i])
            e_gpu, e_model, e_plain = sm.E(out, ref), sm.E(model, ref), sm.E(p32, ref)
            bound = 2 * e_model + 10 * e_plain if rung is None else 10 * e_plain + (1e-6 if rung == "fp32-winograd" else 0.0)
            if not e_gpu <= bound:
                failures.append((sched[i], e_gpu, e_model, e_plain))
            worst = max(worst, (e_gpu / bound, sched[i]), key=lambda t: t[0])
        assert not failures, failures[:8]
        return worst
    for i in sorted(comp):
        y1, y2 = kept[i], comp[i]
        if case.kind == "up":
            ok, fig = torch.equal(y1, y2), float((y1 - y2).abs().max())
        else:
            tol = 1e-6 if case.kind == "pool" else 2e-6
            fig = float((y1 - y2).abs().max()) / max(float(y2.abs().max()), 1.0)
            ok = fig <= tol
        if not ok:
            failures.append((sched[i], fig))
        worst = max(worst, (fig, sched[i]), key=lambda t: t[0])
    assert not failures, failures[:8]
    return worst


def check_case(nets, case, xscale, plan=None, rung=None):
    """One case.  ``rung`` None: the split-f16 kernels at activation scale ``xscale``, the plan's verdicts asserted to be the definition's;
    a key of RUNGS: a control on fp32 arithmetic -- ``plan`` holds out-of-range values labelled silent, and nothing may report."""
    t0 = time.time()
    r = setup(nets, case)
    plan = sp.case_plan(case, xscale) if plan is None else plan
    if rung is None:
        for buf in ("x", "skip"):                        # the plan's verdicts ARE the definition's
            sub = [p for p in plan if p.buf == buf]
            assert sp.verdicts(sub, r.pre, r.mask, xscale) == [p.report for p in sub]
    sched = sp.schedule(plan)
    nets.saturation_count(torch.device(DEV))
    with (nets.activation_scale(xscale) if rung is None else RUNGS[rung](nets)):
        moved, kept, comp, finite, comp_moved = drive(nets, r, sched)
    t1 = time.time()
    expected = [i for i, p in enumerate(sched) if p is not None and p.report]
    missed = [sp.describe(sched[i], case.H, case.W) for i in expected if i not in moved]
    spurious = [("control",) if sched[i] is None else sp.describe(sched[i], case.H, case.W) for i in moved if i not in expected]
    n_sil, n_ctl = sum(1 for p in sched if p is not None and not p.report), sum(1 for p in sched if p is None)
    print(f"saturation {case.name} {'xscale %g' % xscale if rung is None else 'CONTROL on ' + rung}: {len(plan)} probes ({len(expected)} report, "
          f"{n_sil} silent), {n_ctl} controls; reported {len(moved)}, missed {len(missed)}, spurious {len(spurious)}; launches {t1 - t0:.2f} s")
    for tag, rows in (("MISSED", missed), ("SPURIOUS", spurious)):               # (operand, n, c, y, x, value, staging rounds, chunk, kind)
        for row in rows[:48]:
            print(f"    {tag} {row}")
    assert not missed and not spurious, {"missed": len(missed), "spurious": len(spurious), "first": (missed + spurious)[:4]}
    assert not comp_moved, [sp.describe(sched[i], case.H, case.W) for i in comp_moved][:12]
    if finite:
        flags = torch.stack(list(finite.values())).cpu()
        assert bool(flags.all()), [sp.describe(sched[i], case.H, case.W) for i, f in zip(finite, flags) if not f][:12]
    worst = judge_silent(r, sched, kept, comp, xscale, rung)
    print(f"    silent launches held to {'the staged composition' if r.composition else 'float64'}: worst figure {worst[0]:.3g} "
          f"({'of its bound' if not r.composition else 'of the output scale'}) at {worst[1]}; case {time.time() - t0:.2f} s")
    nets.saturation_count(torch.device(DEV))


@pytest.mark.parametrize("xscale", sp.SCALES)
@pytest.mark.parametrize("case", sp.CASES, ids=[c.name for c in sp.CASES])
def test_one_element_moves_the_counter_exactly_when_it_must(S, case, xscale):
    """bad() == the planned report set; silent launches right, report launches finite (module docstring)."""
    from slr_sfs_amd import nets
    check_case(nets, case, xscale)


# ---------------------------------------------------------------------------------------------------------------- controls

FEW = sp.Case("3x3-nchw-none-co3-tile", "conv3", 1, 16, 3, 8, 32, False, None, "tile")
# the fp32 rung: every exhaustive 3x3 case (NCHW / blocked x the four prologues x Cout 32 / 64 / 128), every 1x1 case, and the fused skip / pool / up
# forms where the rung has them (more than 64 output channels; none in the Winograd kernel: nets._block_route); Winograd: the 3x3 cases
ON_FP32 = [c for c in sp.CASES if c.plan in ("tile", "1x1") or (c.kind in ("skip", "pool", "up") and c.cout > 64)]
CONTROLS = [(FEW, "few")] + [(c, "fp32") for c in ON_FP32] + [(c, "fp32-winograd") for c in sp.CASES if c.plan == "tile"]


@pytest.mark.parametrize("case,rung", CONTROLS, ids=[f"{c.name}-{g}" for c, g in CONTROLS])
def test_controls_never_report(S, case, rung):
    """The <= 4-channel kernel (fp32 FMAs on either rung) and everything inside nets.fp32_kernels(), direct and Winograd -- 3x3 in every layout and
    prologue, 1x1, the fused skip / pool / up forms -- on 32 out-of-range probes of the case's own plan (saturation_probe.control_plan: 16 report
    probes per activation scale, every probed operand): the counter does not move in any launch, and the output is held to float64 as those
    kernels' own tests do -- E_gpu <= 10 E_plain32, + 1e-6 for Winograd; the fused forms against their staged composition on the same rung
    (test_skip_branch_inside_the_second_convolution_fp32_rung: 2e-6 / pool 1e-6 / up bit-identical)."""
    from slr_sfs_amd import nets
    check_case(nets, case, 64.0, plan=sp.control_plan(case), rung=rung)


# ---------------------------------------------------------------------------------------------------------------- non-finite activations

NONFINITE = [c for c in sp.CASES if c.mode is None and c.plan in ("tile", "skipx16", "mainx", "lattice", "1x1")]
SPOTS = [(3, 2, 5), (11, 6, 20)]                          # (c, y, x): round 0 and (3x3, one tile) round 2
SPOTS_1X1 = [(3, 2, 5), (11, 9, 12)]                      # 1x1 (10 x 13 pixels): the first workgroup and the ragged wave


@pytest.mark.parametrize("case", NONFINITE, ids=[c.name for c in NONFINITE])
def test_nonfinite_activations_are_reported_or_returned(S, case):
    """+inf, -inf and NaN at one element in staging round 0 and at one in round 2 (no prologue; the fused forms: in their probed operand(s)).
    Wherever the float64 definition's output is non-finite -- the outputs the element reaches, every channel: the weights are random, none is 0 --
    the launch either reports or returns a non-finite value at those outputs; never an all-finite tensor with no report.  Prints what happened."""
    from slr_sfs_amd import nets
    r = setup(nets, case)
    bufs = ["skip"] if case.plan == "skipx16" else ["x", "skip"] if case.plan == "lattice" else ["x"]
    plan = [sp.Probe(b, 0, c, y, x, v, True, name) for b in bufs for c, y, x in (SPOTS_1X1 if case.kind == "conv1" else SPOTS)
            for v, name in ((float("inf"), "+inf"), (float("-inf"), "-inf"), (float("nan"), "nan"))]
    sched = sp.schedule(plan)
    outs = {}
    launch = r.launch
    r.launch = lambda: outs.setdefault(len(outs), launch())
    nets.saturation_count(torch.device(DEV))
    with nets.activation_scale(64.0):
        moved, _, _, _, _ = drive(nets, r, sched)
    R = r.k // 2
    seen = {}
    for i, p in enumerate(sched):
        if p is None:
            assert i not in moved and bool(torch.isfinite(outs[i]).all())
            continue
        reach = torch.zeros(1, 1, case.H, case.W, dtype=torch.float64)
        reach[0, 0, max(p.y - R, 0):p.y + R + 1, max(p.x - R, 0):p.x + R + 1] = float("nan")
        if case.kind == "pool":
            reach = torch.nn.functional.avg_pool2d(reach, 3, stride=2, padding=1)
        elif case.kind == "up":
            reach = torch.nn.functional.interpolate(reach, scale_factor=2, mode="bilinear", align_corners=False)
        reach = torch.isnan(reach).expand(1, case.cout, -1, -1)
        assert bool(reach.any())
        out = logical(case, outs[i])
        returned = bool((~torch.isfinite(out))[reach].all())
        seen[(p.buf, p.kind, "second spot" if p.y >= 6 else "first spot")] = ("reported" if i in moved else "silent", "non-finite" if returned else
                                                                       "finite" if bool(torch.isfinite(out).all()) else "partly non-finite",
                                                                       sorted({tuple(v[2:]) for v in (~torch.isfinite(out)).nonzero().tolist()})[:6])
        assert i in moved or returned, sp.describe(p, case.H, case.W)
    print(f"saturation non-finite {case.name}: {seen}")


@pytest.mark.parametrize("mode", ("bn", "bn_mask", "bn_nonzero"))
def test_nonfinite_activations_behind_a_prologue(S, mode):
    """Behind relu(x * scale - shift): +inf must report; -inf must be silent and right (the ReLU removes it); NaN is out of scope -- every ReLU of the
    package is fmaxf, which returns its other operand, on the fp32 rung as in the staged kernels -- printed, nothing asserted."""
    from slr_sfs_amd import nets
    case = next(c for c in sp.CASES if c.name == f"3x3-nchw-{mode}-co32-tile")
    inf = float("inf")
    plan = [sp.Probe("x", 0, c, y, x, v, rep, name) for c, y, x in SPOTS for v, rep, name in ((inf, True, "+inf"), (-inf, False, "-inf"))]
    check_case(nets, case, 64.0, plan=plan)
    r = setup(nets, case)
    nan_plan = [sp.Probe("x", 0, c, y, x, float("nan"), False, "nan") for c, y, x in SPOTS]
    sched = sp.schedule(nan_plan)
    with nets.activation_scale(64.0):
        moved, kept, _, _, _ = drive(nets, r, sched)
    print(f"saturation non-finite behind {mode}: NaN (asserting nothing): " +
          str([("reported" if i in moved else "silent", "finite output" if bool(torch.isfinite(kept[i]).all()) else "non-finite output")
               for i, p in enumerate(sched) if p is not None]))
    nets.saturation_count(torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------- the animator's partial escalation

FRAMES, FH, FW, FC = 10, 16, 64, 16


def clip_table():
    """10 frames [16,16,64] ~ N(0, 1); frame 5 holds one element of 2000 (out of range at rung 0 only), frame 8 one of 1e5 (at both split rungs);
    element [t,0,0,0] = t / 16 names the frame."""
    table = sp.seeded_base(FRAMES, FC, FH, FW, 3)
    table[5, 9, 6, 20] = 2000.0                          # staging round 2 of its tile
    table[8, 3, 11, 40] = 1.0e5
    table[:, 0, 0, 0] = torch.arange(FRAMES) / 16.0
    return table


def clamps(frame, rung):
    """The oracle: does rung ``rung`` clamp an activation of this frame?"""
    return rung < 2 and sp.must_report(sp.staged(frame, None, None, (64.0, 1.0)[rung]))


def animator_rig(nets):
    table = clip_table()
    dev_table = table.cuda()
    conv = zero_bias(nets.Conv(FC, 32, 3).cuda())
    calls = []

    def features_batch(ts, gen, afl):
        gen.copy_(dev_table[list(ts)])

    def decode_batch(gen, afl):
        ids = [int(round(v * 16)) for v in gen[:, 0, 0, 0].tolist()]
        rung = 2 if nets._S.f32_kernels else (0 if nets._S.act_scale == 64.0 else 1)
        assert rung == 2 or nets._S.act_scale in (64.0, 1.0)
        calls.append((ids, rung))
        with torch.no_grad():
            return conv(gen)

    clip = types.SimpleNamespace(fs=dev_table[:1], C=FC, v1=False, features_batch=features_batch)
    return table, dev_table, conv, calls, clip, decode_batch


def alone(nets, conv, frames, rung):
    with torch.no_grad(), nets.rung_context(rung):
        return conv(frames)


def hold_frames_to_float64(conv, table, result, rung_of):
    wt = conv.weight.detach().cpu()
    for t in range(FRAMES):
        x = table[t:t + 1]
        ref, p32 = sm.plain(x.double(), wt.double(), 3), sm.plain(x, wt, 3)
        e_gpu, e_plain = sm.E(result[t:t + 1], ref), sm.E(p32, ref)
        rung = rung_of[t]
        bound = 10 * e_plain if rung == 2 else 2 * sm.E(sm.conv(x, wt, (64.0, 1.0)[rung], 3), ref) + 10 * e_plain
        print(f"    frame {t} (rung {rung}): E_gpu {e_gpu:.2e} bound {bound:.2e}")
        assert e_gpu <= bound, (t, rung, e_gpu, bound)


def test_animator_renders_again_only_the_batches_that_clamped(S):
    """pipeline._render, policy "auto", batches of 2 over the 10 frames of clip_table(): pass 1 renders frames 0..9 at activation scale 64, pass 2 only
    frames 4, 5, 8, 9 at scale 1, pass 3 only frames 8, 9 on the fp32 rung; the owner ends on rung 2 with one warning per step up; every frame
    is bit-equal to a render of its batch alone on the rung it ended on, and held to the float64 convolution (2 E_model + 10 E_plain32; fp32
    rung: 10 E_plain32)."""
    from slr_sfs_amd import nets, pipeline
    table, dev_table, conv, calls, clip, decode_batch = animator_rig(nets)
    result = torch.zeros(FRAMES, 32, FH, FW, device="cuda")

    def store(pos, outs):
        result[pos] = outs

    owner = types.SimpleNamespace(_conv_rung=0)
    nets.saturation_count(torch.device(DEV))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pipeline._render(owner, clip, range(FRAMES), 2, False, (decode_batch, store), "auto", None)
    pairs = [[t, t + 1] for t in range(0, FRAMES, 2)]
    print(f"saturation animator: decode_batch calls (frames, rung) {calls}")
    assert calls == [(p, 0) for p in pairs] + [([4, 5], 1), ([8, 9], 1), ([8, 9], 2)]
    assert owner._conv_rung == 2
    assert len([x for x in w if "exact range" in str(x.message)]) == 2
    rung_of = {t: 0 for t in range(FRAMES)}
    rung_of.update({4: 1, 5: 1, 8: 2, 9: 2})
    for p in pairs:
        assert not any(clamps(table[t:t + 1], rung_of[t]) for t in p)
        assert torch.equal(result[p], alone(nets, conv, dev_table[p], rung_of[p[0]])), p
    hold_frames_to_float64(conv, table, result.cpu(), rung_of)
    nets.saturation_count(torch.device(DEV))


def test_animator_checks_every_batch_before_it_leaves(S):
    """The same clip through the ``on_frame`` branch: every batch is delivered exactly once, in order; no delivered batch was rendered on a rung at
    which the oracle says it clamps; the rung only ever rises."""
    from slr_sfs_amd import nets, pipeline
    table, dev_table, conv, calls, clip, decode_batch = animator_rig(nets)
    result = torch.zeros(FRAMES, 32, FH, FW, device="cuda")
    stored, delivered = [], []

    def store(pos, outs):
        stored.append((list(pos), calls[-1]))
        result[pos] = outs

    owner = types.SimpleNamespace(_conv_rung=0)
    nets.saturation_count(torch.device(DEV))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pipeline._render(owner, clip, range(FRAMES), 2, False, (decode_batch, store), "auto", delivered.append)
    print(f"saturation animator (on_frame): decode_batch calls {calls}; stored {stored}")
    assert delivered == list(range(FRAMES))
    assert [pos for pos, _ in stored] == [[t, t + 1] for t in range(0, FRAMES, 2)]
    rung_of = {}
    for pos, (ids, rung) in stored:
        assert ids == pos
        assert not any(clamps(table[t:t + 1], rung) for t in pos), (pos, rung)
        rung_of.update({t: rung for t in pos})
    rungs = [rung for _, rung in calls]
    assert rungs == sorted(rungs) and owner._conv_rung == 2 == rungs[-1]
    assert calls == [([0, 1], 0), ([2, 3], 0), ([4, 5], 0), ([4, 5], 1), ([6, 7], 1), ([8, 9], 1), ([8, 9], 2)]
    assert len([x for x in w if "exact range" in str(x.message)]) == 2
    for pos, (ids, rung) in stored:
        assert torch.equal(result[pos], alone(nets, conv, dev_table[pos], rung)), pos
    hold_frames_to_float64(conv, table, result.cpu(), rung_of)
    nets.saturation_count(torch.device(DEV))
