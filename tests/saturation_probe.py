"""Single-element probes of the split-f16 range detector (csrc/conv.hip: stage_value, the skip phase, conv1x1_split_kernel) -- infrastructure
only, no tests.  tests/test_saturation_probe_host.py checks the plans on the CPU, tests/test_gpu_conv_saturation.py runs them.

The contract (nets.check_saturation, stage_value): a split-f16 convolution that clamps an activation returns a wrong frame; that is never
silent: the device counter moves; convs="auto" and convs="split" rest on it.

WHAT THE KERNEL STAGES, written out (``staged``; reproducible in torch float32 because the library is built with -ffp-contract=off):
    no prologue             x * xscale
    prologue                fmax(x * (scale * xscale) - (shift * xscale), 0) * mk      mk: 1 (PRE_BN), the explicit mask value (PRE_BN_MASK),
                                                                                       (x != 0) (PRE_BN_NONZERO)
    skip input              skip_x * xscale
``must_report``: some element inside the image has |staged| >= 65472; ``must_be_silent``: all are below.  Every verdict is formed in float32
AND in float64; a probe whose two verdicts differ is not allowed (``verdicts`` asserts it).  |staged| == 65472 EXACTLY reports although the
clamp is the identity there (the kernel tests AFTER the clamp and cannot tell): such a report is conservative, not wrong -- the plans carry
"edge" probes (== 65472), "beyond" probes (> 65472: the clamped result differs from the unclamped one) and "silent" neighbours.

WHERE AN ELEMENT IS STAGED (conv.hip "Staging of a chunk"): a workgroup covers an 8 x 32 output tile and stages the (8+2) x (32+2) halo block
of every chunk of 16 input channels, halo pixel p = (y - y0 + 1) * 34 + (x - x0 + 1), in three rounds:
    round 0: p < 256, channels 0-7 of the chunk;  round 1: p < 256, channels 8-15;  round 2: p >= 256 (84 pixels), both channel groups.
For the tile at the image origin round 2 is image row 6 from column 17 on, and rows 7 and 8.  A pixel next to a tile seam is staged by every tile
whose halo holds it (``stagings``); a probe ISOLATES a round when every tile stages it in that round."""
import collections
import math

import numpy as np
import torch

import split_model as sm

T = sm.F16_MAX_SPLIT
TILE_H, TILE_W, HALO_W = 8, 32, 34
SCALES = (64.0, 1.0)
PRE_SCALE, PRE_SHIFT = 2.0, 0.5              # dyadic: x * (2 xscale) - 0.5 xscale is exact wherever the plans put a value
IN_SCALE = 2.0 ** -3                        # the "moved in" channels: scale 2^-3, shift 0
IN_CHANNELS = (5, 13)                       # ... one per 8-channel group of chunk 0

Probe = collections.namedtuple("Probe", "buf n c y x value report kind")      # buf: "x" (main input) or "skip"; kind: edge | beyond | silent | a name


# ---------------------------------------------------------------------------------------------------------------- the definition

def prologue(cin, mode):
    """(scale [cin], shift [cin], mode) of the probe prologue: scale 2, shift 0.5; channels IN_CHANNELS scale 2^-3, shift 0."""
    sc, sh = torch.full((cin,), PRE_SCALE), torch.full((cin,), PRE_SHIFT)
    for c in IN_CHANNELS:
        if c < cin:
            sc[c], sh[c] = IN_SCALE, 0.0
    return sc, sh, mode


def _stage(v, sc, sh, mk, xscale, dtype):
    v = v.to(dtype)
    if sc is None:
        return v * xscale
    ps, ph = (sc.float() * xscale).to(dtype), (sh.float() * xscale).to(dtype)           # the kernel's table: fp32 products
    return torch.fmax(v * ps - ph, torch.zeros((), dtype=dtype)) * mk.to(dtype)


def staged(x, pre, mask, xscale, dtype=torch.float32):
    """The activations of [N,C,H,W] ``x`` as the kernel stages them.  pre: None or (scale, shift, mode), mode "bn" | "bn_mask" | "bn_nonzero";
    mask: [N,1,H,W] (used by "bn_mask" only: without a prologue the partial convolution's input is already masked)."""
    if pre is None:
        return _stage(x, None, None, None, xscale, dtype)
    sc, sh, mode = pre
    mk = mask if mode == "bn_mask" else (x != 0).to(x.dtype) if mode == "bn_nonzero" else torch.ones(())
    return _stage(x, sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1), mk, xscale, dtype)


def convolved(x, pre, mask):
    """The tensor the convolution itself sees (float32): the prologue without the pre-scale of the split."""
    return x if pre is None else staged(x, pre, mask, 1.0)


def must_report(st):
    return bool((st.abs() >= T).any())


def must_be_silent(st):
    return bool((st.abs() < T).all())


def verdicts(probes, pre, mask, xscale):
    """[report?] of every probe from ``staged`` at its one element (the base tensor is far inside the range), float32 and float64 twins
    asserted equal, exactly one of must_report / must_be_silent asserted to hold (finite probes)."""
    if not probes:
        return []
    v = torch.tensor([p.value for p in probes], dtype=torch.float32)
    out = []
    for dtype in (torch.float32, torch.float64):
        if pre is None or probes[0].buf == "skip":
            st = _stage(v, None, None, None, xscale, dtype)
        else:
            sc, sh, mode = pre
            c = torch.tensor([p.c for p in probes])
            mk = torch.tensor([float(mask[p.n, 0, p.y, p.x]) for p in probes]) if mode == "bn_mask" else (v != 0).float() if mode == "bn_nonzero" \
                else torch.ones(len(probes))
            st = _stage(v, sc[c], sh[c], mk, xscale, dtype)
        rep = [must_report(s) for s in st]
        assert all(r != must_be_silent(s) for r, s in zip(rep, st))
        out.append(rep)
    assert out[0] == out[1], "a probe's verdict differs between the float32 and the float64 definition"
    return out[0]


# ---------------------------------------------------------------------------------------------------------------- geometry and addresses

def flat_index(shape, n, c, y, x, blocked):
    """Element offset of logical (n, c, y, x) in an NCHW tensor, or in its channel-blocked form [N, C/8, H, W, 8] (metrics_fixture.to_blocked)."""
    N, C, H, W = shape
    if blocked:
        return (((n * (C // 8) + c // 8) * H + y) * W + x) * 8 + c % 8
    return ((n * C + c) * H + y) * W + x


def stagings(y, x, H, W):
    """[(ty, tx, halo pixel)] of every 3x3 workgroup tile that stages image pixel (y, x)."""
    out = []
    for ty in range((H + TILE_H - 1) // TILE_H):
        for tx in range((W + TILE_W - 1) // TILE_W):
            pr, pc = y - ty * TILE_H + 1, x - tx * TILE_W + 1
            if 0 <= pr < TILE_H + 2 and 0 <= pc < HALO_W:
                out.append((ty, tx, pr * HALO_W + pc))
    return out


def rounds(c, y, x, H, W):
    """The staging rounds in which channel c of pixel (y, x) is staged, one per tile that stages it: halo pixel < 256 -> round (c % 16) // 8,
    else round 2."""
    return [((c % 16) // 8 if p < 256 else 2) for _, _, p in stagings(y, x, H, W)]


def chunk(c):
    return c // 16


def describe(p, H, W):
    return (p.buf, p.n, p.c, p.y, p.x, p.value, rounds(p.c, p.y, p.x, H, W), chunk(p.c), p.kind)


# ---------------------------------------------------------------------------------------------------------------- values

def f32(v):
    return float(np.float32(v))


def inward(v):
    return float(np.nextafter(np.float32(v), np.float32(0.0)))


def outward(v):
    return float(np.nextafter(np.float32(v), np.float32(math.copysign(math.inf, v))))


def threshold(pre, xscale, c=0):
    """The smallest positive x of channel c that reports: 65472 / xscale; behind the probe prologue (65472 / xscale + shift[c]) / scale[c]
    (exact: dyadic scale and shift)."""
    t = T / xscale
    return t if pre is None else (t + float(pre[1][c])) / float(pre[0][c])


def pair(buf, n, c, y, x, k, thr, signed):
    """(report probe, its silent inward neighbour) number k at one element.  With j = k // 2 + k % 2 (in the exhaustive plans k = 2 pixel + group,
    so j = pixel + group: neither the sign nor the kind is tied to the channel group, i.e. to the staging round) the sign is (-1)^j where the path
    keeps signs and the report value is edge / nextafter outward / 2 edge for j % 3 = 0 / 1 / 2: all six combinations occur in every group."""
    j = k // 2 + k % 2
    sgn = -1.0 if (signed and j % 2) else 1.0
    edge = sgn * thr
    which = j % 3
    value, kind = ((edge, "edge"), (outward(edge), "beyond"), (2.0 * edge, "beyond"))[which]
    return [Probe(buf, n, c, y, x, value, True, kind), Probe(buf, n, c, y, x, inward(edge), False, "silent")]


# ---------------------------------------------------------------------------------------------------------------- plans

def plan_tile(cin, H, W, pre, xscale, buf="x", n=0, pixels=None, channels="group"):
    """Pairs at ``pixels`` (default: every pixel of the image) x every 8-channel group (channels="group": one channel per group, (3y + x) % 8
    within it so that all eight lanes of a staging item are met; "all": every channel)."""
    pre = pre if buf == "x" else None
    out, k = [], 0
    for y, x in (pixels if pixels is not None else [(y, x) for y in range(H) for x in range(W)]):
        for g in range(cin // 8 if channels == "group" else cin):
            c = 8 * g + (3 * y + x) % 8 if channels == "group" else g
            out += pair(buf, n, c, y, x, k, threshold(pre, xscale, c), pre is None)
            k += 1
    return out


def plan_prologue_extras(cin, H, W, pre, mask, xscale):
    """What the prologue moves into or out of range (the false-positive side), at one round-0/1 and one round-2 pixel each."""
    if pre is None:
        return []
    t = T / xscale
    out = []
    for y, x in ((2, 5), (6, 20)):
        for c in IN_CHANNELS:                                                    # moved in: 5000 under scale 2^-3 (at xscale 64; 4.9 t at any)
            out.append(Probe("x", 0, c, y, x, f32(t * 4.0), False, "moved-in"))
        out.append(Probe("x", 0, 2, y, x, f32(t * 0.625), True, "moved-out"))     # 639 under scale 2 at xscale 64: below t itself
        out.append(Probe("x", 0, 9, y, x, -1.0e6 * (64.0 / xscale), False, "relu"))
        out.append(Probe("x", 0, 9, y, x, -3.0e38, False, "relu"))
    if pre[2] == "bn_mask":
        for n_, y, x in masked_pixels(mask):
            out.append(Probe("x", n_, 1, y, x, f32(t * 8.0), False, "masked"))
    if pre[2] == "bn_nonzero":
        for n_, y, x in masked_pixels(mask):                                      # the base is 0 there; a probe makes the element non-zero
            out.append(Probe("x", n_, 1, y, x, f32(t * 8.0), True, "derived-nonzero"))
            out.append(Probe("x", n_, 10, y, x, 1.0, False, "derived-nonzero"))
    return out


def masked_pixels(mask):
    return [] if mask is None else [tuple(int(v) for v in (i[0], i[2], i[3])) for i in (mask == 0).nonzero()]


def probe_mask(N, H, W):
    """[N,1,H,W] of ones with zeros at one round-0/1 pixel, one isolated round-2 pixel and one seam pixel of the origin tile (where the image has them)."""
    m = torch.ones(N, 1, H, W)
    for y, x in ((1, 3), (6, 25), (7, 31)):
        if y < H and x < W:
            m[:, :, y, x] = 0.0
    return m


ROUND_PIXELS = [(2, 5), (6, 20), (7, 10)]            # rounds 0/1; round 2 in one tile only; round 2 in the tile, rounds 0/1 in the tile below


def ragged_pixels(H, W):
    """One pixel per staging round, the tile seams (x = 31, 32; y = 7, 8), the last row and the last column."""
    px = ROUND_PIXELS + [(7, 31), (7, 32), (8, 31), (8, 32), (0, W - 1), (H - 1, 0), (H - 1, 16), (H - 1, W - 1)]
    return sorted({(y, x) for y, x in px if y < H and x < W})


def lattice_pixels(H, W):
    """Every corner of the image and of every 8 x 32 tile, every seam neighbour, and the round-2 boundary of every tile (rows 6 / 7 of the tile at
    columns 15, 16, 17 and 0, 31, and the halo row below it)."""
    px = set()
    for y0 in range(0, H, TILE_H):
        for x0 in range(0, W, TILE_W):
            ys = [y0, y0 + 5, y0 + 6, y0 + 7, y0 + 8]
            xs = [x0 - 1, x0, x0 + 15, x0 + 16, x0 + 17, x0 + 30, x0 + 31, x0 + 32]
            px |= {(y, x) for y in ys for x in xs}
    px |= {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    return sorted((y, x) for y, x in px if 0 <= y < H and 0 <= x < W)


def one_by_one_pixels(HW, W):
    """1x1 kernel, pixels 0, 31, 32, 127, 128, 129 (wave and workgroup boundaries; HW = 130 is one workgroup plus a ragged wave)."""
    return [(p // W, p % W) for p in (0, 31, 32, 127, 128, 129) if p < HW]


def plan_1x1(cin, H, W, xscale):
    """Every channel at pixels 0, 31, 32, 127, 128, 129; every pixel at channels 0 and Cin - 1."""
    out = plan_tile(cin, H, W, None, xscale, pixels=one_by_one_pixels(H * W, W), channels="all")
    k = 0
    for c in (0, cin - 1):
        for y in range(H):
            for x in range(W):
                out += pair("x", 0, c, y, x, k, T / xscale, True)
                k += 1
    return out


def boundary_only(plan):
    """The exact-boundary pairs of a plan (activation scale 1 runs these): edge probes and the silent neighbour behind each."""
    return [p for i, p in enumerate(plan) if p.kind == "edge" or (p.kind == "silent" and i > 0 and plan[i - 1].kind == "edge")]


def control_plan(case):
    """The out-of-range probes the fp32-arithmetic controls run: 16 report probes of the case's plan per activation scale (evenly thinned, every
    operand of the plan), relabelled silent -- nothing may report there."""
    out = []
    for xscale in SCALES:
        rep = [p for p in case_plan(case, xscale) if p.report]
        out += [p._replace(report=False, kind="control") for p in rep[::max(len(rep) // 16, 1)][:16]]
    return out


def schedule(plan, every=8):
    """The launches of a case: the probes in order with a control (None: the untouched tensor) as every ``every``-th launch, first and last included."""
    out = [None]
    for p in plan:
        if len(out) % every == 0:
            out.append(None)
        out.append(p)
    out.append(None)
    return out


# ---------------------------------------------------------------------------------------------------------------- the unclamped model

def conv_unclamped(x, w, xscale, k, acc=torch.float64):
    """split_model.conv without the clamp of stage_value: what the split arithmetic would return if activations beyond the f16 range were
    converted as they are (inf and NaN included)."""
    ws = sm.wscale(w)
    xh, xl = (t.to(acc) for t in sm.split(x.float() * xscale))
    wh, wl = (t.to(acc) for t in sm.split(w.float() * ws))
    out = sm.plain(xh, wh, k) + sm.plain(xh, wl, k) + sm.plain(xl, wh, k)
    return out * (1.0 / (xscale * ws))


def apply(base, probe):
    x = base.clone()
    x[probe.n, probe.c, probe.y, probe.x] = probe.value
    return x


def seeded_base(N, C, H, W, seed):
    g = torch.Generator().manual_seed(7000 + 100 * C + 10 * H + W + seed)
    return torch.randn(N, C, H, W, generator=g)


def seeded_weight(cout, cin, k, seed):
    g = torch.Generator().manual_seed(9000 + 100 * cin + cout + k + seed)
    return torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)


# ---------------------------------------------------------------------------------------------------------------- the cases (CPU and GPU)

Case = collections.namedtuple("Case", "name kind N cin cout H W blocked mode plan")
# kind: "conv3" | "conv1" | "skip" (probes in the skip input or the main input of a fused-skip 3x3) | "pool" | "up"; mode: None | bn | bn_mask | bn_nonzero
# (the fused forms: None | "bn" = Conv.forward_skip without / with the second convolution's prologue, "pconv" = PartialConv.forward_skip);
# plan: "tile" exhaustive | "ragged" | "batch" (sample 1 only) | "skipx" / "mainx" (fused forms: which operand is probed) | "lattice" | "1x1"


def case_mask(case):
    return probe_mask(case.N, case.H, case.W) if case.mode in ("bn_mask", "bn_nonzero", "pconv") else None


def case_pre(case):
    return prologue(case.cin, case.mode) if case.mode in ("bn", "bn_mask", "bn_nonzero") else None


def case_base(case, buf="x"):
    """The clean tensor of a case: randn (|x| < 6: far below the range on either scale); zero at the mask's zeros for the derived mask (that IS the mask)."""
    c = case.cin if buf == "x" else skip_cin(case)
    base = seeded_base(case.N, c, case.H, case.W, 0 if buf == "x" else 1)
    if buf == "x" and case.mode == "bn_nonzero":
        base = base * case_mask(case)
    assert float(base.abs().max()) < 8.0
    return base


def skip_cin(case):
    return 40 if case.plan.endswith("40") else 16


def case_plan(case, xscale):
    """The probes of a case at activation scale ``xscale``: the full plan at 64, the exact-boundary pairs at 1."""
    pre, mask = case_pre(case), case_mask(case)
    N, cin, H, W = case.N, case.cin, case.H, case.W
    if case.plan == "tile":
        plan = plan_tile(cin, H, W, pre, xscale) + plan_prologue_extras(cin, H, W, pre, mask, xscale)
    elif case.plan == "ragged":
        plan = plan_tile(cin, H, W, pre, xscale, pixels=ragged_pixels(H, W), channels="all")
    elif case.plan == "batch":
        plan = plan_tile(cin, H, W, pre, xscale, n=1, pixels=[(0, 0), (3, 16), (6, 17), (7, 31)], channels="all")
    elif case.plan in ("skipx16", "skipx40"):
        sc = skip_cin(case)
        plan = plan_tile(sc, H, W, None, xscale, buf="skip", pixels=None if sc == 16 else [(0, 0), (6, 20), (7, 31), (H - 1, W - 1)],
                         channels="group" if sc == 16 else "all")
    elif case.plan == "mainx":
        plan = plan_tile(cin, H, W, pre, xscale) + plan_prologue_extras(cin, H, W, pre, None, xscale)
    elif case.plan == "lattice":
        plan = plan_tile(cin, H, W, pre, xscale, pixels=lattice_pixels(H, W)) + \
            plan_tile(16, H, W, None, xscale, buf="skip", pixels=lattice_pixels(H, W))
    elif case.plan == "1x1":
        plan = plan_1x1(cin, H, W, xscale)
    else:
        raise ValueError(case.plan)
    if case.mode == "bn_mask":                                               # PRE_BN_MASK multiplies by the mask value: nothing reports at a masked pixel
        plan = [p._replace(report=False, kind="masked") if p.buf == "x" and float(mask[p.n, 0, p.y, p.x]) == 0.0 and p.report else p for p in plan]
    return plan if xscale == 64.0 else boundary_only(plan)


def _cases():
    out = []
    for cout in (32, 64, 128):                                           # WCO 1 / 2 / 4
        for blocked in (False, True):
            for mode in (None, "bn", "bn_mask", "bn_nonzero"):
                if blocked and mode == "bn_nonzero":                       # (the library refuses a derived mask on a channel-blocked input)
                    continue
                tag = f"{'b8' if blocked else 'nchw'}-{mode or 'none'}-co{cout}"
                out.append(Case(f"3x3-{tag}-tile", "conv3", 1, 16, cout, 8, 32, blocked, mode, "tile"))
                out.append(Case(f"3x3-{tag}-ragged", "conv3", 1, 40, cout, 9, 33, blocked, mode, "ragged"))
                out.append(Case(f"3x3-{tag}-batch", "conv3", 2, 16, cout, 8, 32, blocked, mode, "batch"))
    for cout in (32, 64, 128):
        for mode in (None, "bn", "pconv"):
            tag = f"{mode or 'none'}-co{cout}"
            out.append(Case(f"skip-{tag}-skipx16", "skip", 1, 16, cout, 8, 32, True, mode, "skipx16"))
            out.append(Case(f"skip-{tag}-mainx", "skip", 1, 16, cout, 8, 32, True, mode, "mainx"))
            out.append(Case(f"skip-{tag}-skipx40", "skip", 1, 16, cout, 9, 33, True, mode, "skipx40"))
    for kind in ("pool", "up"):
        for mode in (None, "pconv"):
            out.append(Case(f"{kind}-{mode or 'none'}-co128-lattice", kind, 1, 16, 128, 16, 64, True, mode, "lattice"))
    for cin, cout, blocked in ((16, 32, False), (32, 64, False), (40, 128, False), (24, 32, True), (16, 64, True), (40, 128, True)):   # NCT 1 / 2 / 4
        out.append(Case(f"1x1-{'b8' if blocked else 'nchw'}-{cin}to{cout}", "conv1", 1, cin, cout, 10, 13, blocked, None, "1x1"))
    return out


CASES = _cases()
