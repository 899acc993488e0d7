"""The cases of the deterministic ``splat_blend`` tests and, from the flow alone (numpy, no GPU), which paths of the forward they take.

A tile is 8 x 64 output pixels.  An ENTRY of a tile (or of a range of its columns) is a source pixel whose 2 x 2 footprint touches it; a
RECORD is one (source, corner) pair on an output pixel -- all four corners of a representable target that lie in the image, also those
of weight 0.  The constants below are quoted from ``slr-sfs_amd/csrc/slr_tuning.hpp`` / ``splat_op.hip`` /``splat_tile.hpp`` and are
compared with the sources by tests/test_splat_blend_deterministic_host.py.

Which path a piece of work takes (csrc/splat_op.hip, splat_rows.hpp, splat_tile.hpp):
  scan front end   a tile of at most SCAN_DEFER_AT entries is rendered in place: ``MODE 1`` walk, the balanced gather when its longest
                   list exceeds ceil(positions / 512) + BAL_SLACK (positions: list lengths padded to odd); a tile above it goes to the
                   sink launch: tasks of SEG entries, dealt to min(SINK_TASKS, tasks) slots, lists of HEAVY_SLACK + 16 records and more
                   walked by the whole wave;
  rows front end   a whole tile of at most SEG entries: ``MODE 0``; a tile above SEG is cut by the plan into ranges of column octants
                   (``plan_pieces``: the greedy cut of rows_plan on the octants' entry counts), walked in ``MODE 1``, with 8 / 4 / 2 lanes
                   per output pixel in pieces of 8 / 16 / 32 columns; a piece above SEG goes to the pass-by-pass launch (``MODE 2``,
                   passes of PASS_SEG entries).
"""
import numpy as np

TILE_H, TILE_W = 8, 64
SEG = 1024                 # SLR_EPT_ONE * 512
PASS_SEG = 2048            # SLR_EPT_DEFER * 512
SCAN_DEFER_AT = 896
BAL_SLACK = 24
HEAVY_SLACK = 24
SINK_TASKS = 16
ROWS_FILL = 7
TUNING = dict(SLR_EPT_ONE=2, SLR_EPT_DEFER=4, SLR_SCAN_DEFER_AT=SCAN_DEFER_AT, SLR_BAL_SLACK=BAL_SLACK, SLR_HEAVY_SLACK=HEAVY_SLACK,
              SLR_SINK_TASKS=SINK_TASKS, SLR_ROWS_FILL=ROWS_FILL, SLR_TILE_H=TILE_H)


def paths(flow):
    """flow [N,2,H,W] float32 -> per sample: entries per tile [N,ty,tx] and per column octant [N,ty,tx,8], records per output pixel
    [N,H,W], sources dropped [N,H,W]."""
    flow = np.asarray(flow, np.float32)
    N, _, H, W = flow.shape
    ty, tx = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    tiles, octs = np.zeros((N, ty, tx), np.int64), np.zeros((N, ty, tx, 8), np.int64)
    recs, drop = np.zeros((N, H, W), np.int64), np.zeros((N, H, W), bool)
    for n in range(N):
        with np.errstate(invalid="ignore", over="ignore"):
            X, Y = (x + flow[n, 0]).astype(np.float32), (y + flow[n, 1]).astype(np.float32)
            ok = (np.abs(X) < 2.0 ** 30) & (np.abs(Y) < 2.0 ** 30)
        drop[n] = ~ok
        x0 = np.floor(np.where(ok, X, 0)).astype(np.int64)[ok]
        y0 = np.floor(np.where(ok, Y, 0)).astype(np.int64)[ok]
        for dy in (0, 1):
            for dx in (0, 1):
                cx, cy = x0 + dx, y0 + dy
                m = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
                np.add.at(recs[n], (cy[m], cx[m]), 1)
        # an entry of (tile row r, octant o): some corner row in the tile row and some corner column in the octant, both in the image
        ya, yb = y0, y0 + 1
        xa, xb = x0, x0 + 1
        ya_ok, yb_ok, xa_ok, xb_ok = (ya >= 0) & (ya < H), (yb >= 0) & (yb < H), (xa >= 0) & (xa < W), (xb >= 0) & (xb < W)
        ra, rb = ya // TILE_H, yb // TILE_H
        oa, ob = xa // 8, xb // 8                                   # global octant index (8 per tile column)
        ca, cb = xa // TILE_W, xb // TILE_W
        for r, r_ok, first_r in ((ra, ya_ok, True), (rb, yb_ok & (~ya_ok | (rb != ra)), False)):
            for o, o_ok in ((oa, xa_ok), (ob, xb_ok & (~xa_ok | (ob != oa)))):
                m = r_ok & o_ok
                np.add.at(octs[n], (r[m], o[m] // 8, o[m] % 8), 1)
            for c, c_ok in ((ca, xa_ok), (cb, xb_ok & (~xa_ok | (cb != ca)))):
                m = r_ok & c_ok
                np.add.at(tiles[n], (r[m], c[m]), 1)
    return dict(tiles=tiles, octants=octs, records=recs, dropped=drop)


def tile_lists(records, n, r, c):
    """The 512 list lengths of tile (r, c) of sample n (pixels past the image: 0)."""
    t = np.zeros((TILE_H, TILE_W), np.int64)
    blk = records[n, r * TILE_H:(r + 1) * TILE_H, c * TILE_W:(c + 1) * TILE_W]
    t[:blk.shape[0], :blk.shape[1]] = blk
    return t


def balanced(lists):
    """The scan tile kernel's rule for the balanced gather (stream_planes): longest list > ceil(positions / 512) + BAL_SLACK."""
    positions = int((lists | 1).sum())
    return int(lists.max()) > (positions + 511) // 512 + BAL_SLACK


def plan_pieces(cnt, octants, scale=None):
    """rows_plan's cut of a tile of `cnt` > SEG entries into ranges of column octants, on the octants' entry counts (the kernel uses a
    histogram estimate of them in units of 16, scaled to cnt + cnt / 8; `scale`: per-octant factors standing for that estimate's error).
    -> [(first octant, octants)]."""
    octants = np.asarray(octants, np.float64) * (1.0 if scale is None else np.asarray(scale, np.float64))
    limit = SEG * ROWS_FILL // 8
    osum = cnt + cnt // 8
    co = octants * (osum / max(octants.sum(), 1.0))
    even = int(osum / np.ceil(osum / limit))
    pieces, start, s = [], 0, 0
    for o in range(8):
        c = int(co[o])
        if (s + c > limit or s + c // 2 >= even) and o > start:
            pieces.append((start, o - start))
            start, s = o, 0
        s += c
    pieces.append((start, 8 - start))
    return pieces


def robust_pieces(cnt, octants, noise=0.08, trials=32):
    """plan_pieces, the same under `trials` draws of +-noise on every octant (the histogram's rounding); None when a draw cuts otherwise."""
    base = plan_pieces(cnt, octants)
    rng = np.random.default_rng(0)
    for _ in range(trials):
        if plan_pieces(cnt, octants, 1.0 + rng.uniform(-noise, noise, 8)) != base:
            return None
    return base


# ------------------------------------------------------------------ flows of our own: contractions

def _grid(H, W):
    return np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")


def jitter(shape, seed, amp):
    return np.random.default_rng(seed).uniform(-amp, amp, shape).astype(np.float32)


def row_pile_flow(H, W, seed, rows=15, band=(16, 48), target=3.0):
    """Source rows [0, rows) of the columns `band` (of every 64) go to output row `target` (+ a sub-pixel jitter in x): their records pile
    onto one row of the tile; everybody else moves by less than a pixel."""
    y, x = _grid(H, W)
    fl = jitter((1, 2, H, W), seed, 0.45)
    inb = ((x % TILE_W) >= band[0]) & ((x % TILE_W) < band[1]) & (y < rows)
    fl[0, 1][inb] = (target - y)[inb]
    return fl


def point_flow(H, W, seed, centre, region, strength=0.98):
    """The sources of `region` (y0, y1, x0, x1) contract towards `centre` (y, x) by `strength`; the others move by less than a pixel."""
    y, x = _grid(H, W)
    fl = jitter((1, 2, H, W), seed, 0.45)
    m = (y >= region[0]) & (y < region[1]) & (x >= region[2]) & (x < region[3])
    fl[0, 0][m] += ((centre[1] - x) * strength)[m]
    fl[0, 1][m] += ((centre[0] - y) * strength)[m]
    return fl


def cut_flow(H, W, seed, tile_row=3, widths=(36.0, 1.5, 1.5, 12.5, 2.8, 2.8, 2.8, 2.8)):
    """Every source row goes into tile row `tile_row` (y -> 8 * tile_row + y / (H / 8)); in x, octant o of tile column 0 receives
    widths[o] source columns (piecewise linear), the source columns behind them keep their x."""
    y, x = _grid(H, W)
    fl = jitter((1, 2, H, W), seed, 0.02)
    fl[0, 1] += (TILE_H * tile_row + y * (TILE_H / H) * 0.98) - y
    edges = np.concatenate([[0.0], np.cumsum(widths)])
    tx = x.copy()
    for o in range(8):
        m = (x >= edges[o]) & (x < edges[o + 1])
        tx[m] = (8.0 * o + 0.25 + (x - edges[o]) * (7.5 / widths[o]))[m]
    fl[0, 0] += tx - x
    return fl


def blend_inputs(shape, seed, flow_f, flow_p, alpha=None):
    """Values / logits / cotangent as in tests/test_gpu_splat_blend.py's cases."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    c = dict(start_fs=rng.standard_normal(shape).astype(np.float32), end_fs=rng.standard_normal(shape).astype(np.float32),
             z_start=(0.7 * rng.standard_normal((N, 1, H, W))).astype(np.float32), z_end=(0.7 * rng.standard_normal((N, 1, H, W))).astype(np.float32),
             go=rng.standard_normal(shape).astype(np.float32))
    c["flow_f"], c["flow_p"] = np.ascontiguousarray(flow_f, np.float32), np.ascontiguousarray(flow_p, np.float32)
    c["alpha"] = rng.uniform(0.1, 0.9, N).astype(np.float32) if alpha is None else np.asarray(alpha, np.float32)
    return c


# ------------------------------------------------------------------ the cases

CASES = {
    "plain": dict(shape=(2, 8, 16, 128), front_ends=("scan", "rows")),
    "ragged": dict(shape=(1, 9, 20, 200), front_ends=("scan", "rows")),
    "row_pile": dict(shape=(1, 16, 16, 128), front_ends=("scan",)),
    "sink": dict(shape=(1, 16, 64, 128), front_ends=("scan",)),
    "cut": dict(shape=(1, 16, 64, 128), front_ends=("rows",)),
    "channels": dict(shape=(2, 65, 16, 128), front_ends=("scan", "rows")),
}
SINK_CENTRE, SINK_REGION = (27.3, 40.6), (0, 64, 0, 72)


def make_case(name, oracle, channels=None, option="default"):
    """The inputs of case `name` (`channels`: another plane count; `option`: tests/test_gpu_splat_blend.py's OPTIONS)."""
    import test_gpu_gradients as TG
    import test_gpu_splat_blend as SB
    N, C, H, W = CASES[name]["shape"]
    shape = (N, channels or C, H, W)
    seed = 4100 + 10 * list(CASES).index(name)
    if name in ("plain", "channels"):
        flows = [TG.family_case(oracle, "uniform3", shape, "softmax", seed + d, 1.0)[1] for d in (1, 2)]
        alpha = (0.3, 0.8)
    elif name == "ragged":
        flows = [TG.family_case(oracle, "nan", shape, "softmax", seed + d, 1.0)[1] for d in (1, 2)]
        alpha = None
    elif name == "row_pile":
        flows = [row_pile_flow(H, W, seed + 1, rows=14, target=3.0), row_pile_flow(H, W, seed + 2, rows=14, target=11.0)]
        alpha = None
    elif name == "sink":
        flows = [point_flow(H, W, seed + 1, SINK_CENTRE, SINK_REGION, 0.985), point_flow(H, W, seed + 2, (44.7, 90.2), (0, 64, 56, 128), 0.985)]
        alpha = None
    elif name == "cut":
        flows = [cut_flow(H, W, seed + 1, tile_row=3), cut_flow(H, W, seed + 2, tile_row=5)]
        alpha = None
    else:
        raise KeyError(name)
    c = blend_inputs(shape, seed, flows[0], flows[1], alpha)
    return SB.with_option(c, option)


def conditions(name, c):
    """[(what, holds)] for case `name`: the paths its flows must reach, from the flows alone."""
    N, C, H, W = c["start_fs"].shape
    pf, pp = paths(c["flow_f"]), paths(c["flow_p"])
    out = []
    add = lambda what, ok: out.append((what, bool(ok)))                # noqa: E731
    both = (("flow_f", pf), ("flow_p", pp))
    if name in ("plain", "channels", "ragged", "row_pile"):
        for d, p in both:
            add(f"{d}: every tile is rendered in place by the scan tile kernel (<= SLR_SCAN_DEFER_AT entries: MODE 1) and is a whole tile of "
                f"the rows front end (<= SEG: MODE 0)", p["tiles"].max() <= SCAN_DEFER_AT <= SEG)
            add(f"{d}: lists of several records (their order matters)", p["records"].max() >= 4 and np.median(p["records"][p["records"] > 0]) >= 3)
    if name in ("plain", "channels"):
        add("two samples with different alpha", N == 2 and c["alpha"][0] != c["alpha"][1])
        add("more than one tile per sample", pf["tiles"].shape[1] * pf["tiles"].shape[2] > 1)
    if name == "channels":
        nt = N * pf["tiles"].shape[1] * pf["tiles"].shape[2]
        add("an odd channel unit (C = 8 k + 1) and several channel groups per tile", C % 8 == 1 and min(4, 512 // nt, C // 8) > 1)
    if name == "ragged":
        add("image edges inside tiles", H % TILE_H != 0 and W % TILE_W != 0)
        add("a tail chunk of one plane", C % 4 == 1)
        for d, p in both:
            add(f"{d}: dropped sources", p["dropped"].any())
    if name == "row_pile":
        for d, p in both:
            bal = [balanced(tile_lists(p["records"], 0, r, q)) for r in range(p["tiles"].shape[1]) for q in range(p["tiles"].shape[2])]
            add(f"{d}: a tile whose longest list exceeds its positions per work-item by more than SLR_BAL_SLACK (balanced gather)", any(bal))
            add(f"{d}: and a tile that keeps the register path", not all(bal))
    if name == "sink":
        for d, p in both:
            big = int(p["tiles"].max())
            tasks = (big + SEG - 1) // SEG
            r, q = [int(v) for v in np.argwhere(p["tiles"][0] == big)[0]]
            longest = int(tile_lists(p["records"], 0, r, q).max())
            add(f"{d}: a tile of several thousand entries -> the sink launch, several task slots", big >= 3000 and 3 <= tasks <= SINK_TASKS)
            add(f"{d}: one pixel with more than SEG records: its list spans tasks", longest > SEG)
            add(f"{d}: ... and is walked cooperatively in a task (>= 16 + SLR_HEAVY_SLACK records per task)", longest // tasks >= 16 + HEAVY_SLACK)
            add(f"{d}: the call's entries fit the entry array (2^20) -- no fallback", int(p["tiles"][p["tiles"] > SCAN_DEFER_AT].sum()) < 2 ** 20)
            add(f"{d}: at least 30 % ordinary sources", (np.abs(c[d]) < 1.0).all(1).mean() >= 0.3)
    if name == "cut":
        for d, p in both:
            big = int(p["tiles"][:, :, 0].max())
            r = int(np.argwhere(p["tiles"][0, :, 0] == big)[0][0])
            octs = p["octants"][0, r, 0]
            pieces = robust_pieces(big, octs)
            add(f"{d}: a tile above SEG that the plan cuts the same way under +-8 % on every octant", big > SEG and pieces is not None)
            widths = {8 * n for _, n in (pieces or [])}
            add(f"{d}: pieces of 8, 16 and 17..32 columns: lane groups of 8, 4 and 2 (MODE 1)", 8 in widths and 16 in widths and bool(widths & {24, 32}))
            add(f"{d}: every piece but the heavy octant's fits a segment", all(octs[a:a + n].sum() <= SEG for a, n in (pieces or []) if (a, n) != (0, 1)))
            add(f"{d}: one octant above SEG -> the pass-by-pass launch, in two passes", pieces is not None and pieces[0] == (0, 1) and PASS_SEG < octs[0] <= 2 * PASS_SEG)
    return out


# ------------------------------------------------------------------ a call that must take a capacity fallback
# A grid of more than SLR_SCAN_MAX_TILES tiles forced onto the scan front end gets the small workspace pools (csrc/splat_ws.hpp: 1 MiB of
# entries = 65 536, 8 MiB of slabs); a flow that halves every x makes every tile it reaches a sink, and their entries exceed the array.
SCAN_MAX_TILES, SMALL_ENT_CAP = 1024, (1 << 20) // 16
FALLBACK_SHAPE = (1, 2, 264, 2048)


def fallback_case():
    N, C, H, W = FALLBACK_SHAPE
    y, x = _grid(H, W)
    flows = []
    for seed in (4801, 4802):
        fl = jitter((1, 2, H, W), seed, 0.3)
        fl[0, 0] += x * 0.5 - x
        flows.append(fl)
    return blend_inputs(FALLBACK_SHAPE, 4800, flows[0], flows[1])


def fallback_conditions(c):
    N, C, H, W = c["start_fs"].shape
    out = []
    for d in ("flow_f", "flow_p"):
        t = paths(c[d])["tiles"]
        out.append((f"{d}: more than SLR_SCAN_MAX_TILES tiles: the small pools", t.size > SCAN_MAX_TILES))
        out.append((f"{d}: the sinks' entries exceed the entry array", int(t[t > SCAN_DEFER_AT].sum()) > SMALL_ENT_CAP))
    return out
