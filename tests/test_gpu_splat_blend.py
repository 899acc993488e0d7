"""slr_sfs_amd.splat_blend / TrainingSynthesis on the GPU against the float64 definition of tests/blend_f64.py.

Criterion (tests/test_gpu_gradients.py): per tensor E = max|got - ref64| / max|ref64| and E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the same
definition run in float32 on the CPU; the cotangent go * clamp(norm64, max=1) is made once from the float64 run; every figure is printed
before it is asserted (run with -s).  Applied to `out` and to all six gradients.

Condition on the inputs, stated with the reference alone and asserted before the GPU is used: every float64 gradient finite and at
least 30 % of its elements >= 1e-3 * max.  The main case ([2,64,256,256], steps (30, 59) of 60, smooth_motion(seed 21 + b, amp 2.0),
values and cotangent N(0,1), logits 0.7 * N(0,1), rng seed 2025) meets it as it is; a family case that misses it is re-seeded, then
halved in amplitude (three seeds per amplitude), like test_mode_gradients_vs_float64 -- never skipped."""
import itertools

import numpy as np
import pytest
import torch

import blend_f64 as B64
import test_gpu_gradients as TG

pytestmark = pytest.mark.gpu

NAMES = ("start_fs", "z_start", "flow_f", "end_fs", "z_end", "flow_p")
NF = 60
OPTIONS = {"default": {}, "v1": dict(subtract_max=False), "noclamp": dict(clamp_z=None), "znone": {}, "shared": {}}


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def blend_factor(t):
    """alpha of animating_softmax_splating.py:585-586 for start 0, middle t, end NF - 1, in float32 like the reference."""
    t = torch.tensor([float(v) for v in t])
    return (1.0 - (t - 0.0) / (torch.full_like(t, NF - 1.0) - 0.0 + 1.0)).numpy().astype(np.float32)


def euler_case(oracle, shape, seed=2025, amp=2.0, option="default"):
    """The main case's recipe at any shape: Euler fields of smooth_motion(seed 21 + b) at t = 30 (, 59) forward and NF - t backward."""
    N, C, H, W = shape
    t = (30, 59)[:N]
    rng = np.random.default_rng(seed)
    c = dict(start_fs=rng.standard_normal(shape).astype(np.float32), end_fs=rng.standard_normal(shape).astype(np.float32),
             z_start=(0.7 * rng.standard_normal((N, 1, H, W))).astype(np.float32), z_end=(0.7 * rng.standard_normal((N, 1, H, W))).astype(np.float32),
             go=rng.standard_normal(shape).astype(np.float32))
    mo = np.concatenate([TG.smooth_motion(H, W, 21 + b, amp=amp) for b in range(N)])
    c["flow_f"] = np.concatenate([oracle.euler_integration(mo[b:b + 1], t[b])[0] for b in range(N)])
    c["flow_p"] = np.concatenate([oracle.euler_integration(-mo[b:b + 1], NF - t[b])[0] for b in range(N)])
    c["alpha"], c["motion"], c["t"] = blend_factor(t), mo, t
    return with_option(c, option)


def family(oracle, kind, shape, seed, s, option="default"):
    """Flows of test_gpu_gradients.family_case (two draws: one per direction), values / logits / cotangent as in the main case."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    c = dict(start_fs=rng.standard_normal(shape).astype(np.float32), end_fs=rng.standard_normal(shape).astype(np.float32),
             z_start=(0.7 * rng.standard_normal((N, 1, H, W))).astype(np.float32), z_end=(0.7 * rng.standard_normal((N, 1, H, W))).astype(np.float32),
             go=rng.standard_normal(shape).astype(np.float32))
    c["flow_f"] = TG.family_case(oracle, kind, shape, "softmax", seed + 1, s)[1]
    c["flow_p"] = TG.family_case(oracle, kind, shape, "softmax", seed + 2, s)[1]
    c["alpha"] = rng.uniform(0.1, 0.9, N).astype(np.float32)
    return with_option(c, option)


def with_option(c, option):
    c = dict(c, option=option, opts=OPTIONS[option])
    if option == "znone":
        c["z_start"] = c["z_end"] = None
    if option == "shared":                             # one tensor for both directions: autograd adds the two gradients
        c["end_fs"], c["z_end"] = c["start_fs"], c["z_start"]
    return c


def leaf_names(c):
    return [k for k in NAMES if c[k] is not None and not (c["option"] == "shared" and k in ("end_fs", "z_end"))]


def reference(c, dtype, cot=None):
    """out, the gradients w.r.t. leaf_names(c) and the cotangent, from the plain definition in `dtype` on the CPU."""
    lv = {k: None if c[k] is None else torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in NAMES}
    if c["option"] == "shared":
        lv["end_fs"], lv["z_end"] = lv["start_fs"], lv["z_start"]
    threads = torch.get_num_threads()
    if c["start_fs"].size < 2 ** 20:
        torch.set_num_threads(1)
    try:
        out, norm = B64.blend_f64(*[lv[k] for k in NAMES], torch.from_numpy(c["alpha"]), dtype, return_norm=True, **c["opts"])
        if cot is None:
            cot = (torch.from_numpy(c["go"]).double() * norm.detach().clamp(max=1.0)).float()
        names = leaf_names(c)
        grads = torch.autograd.grad(out, [lv[k] for k in names], cot.to(dtype))
    finally:
        torch.set_num_threads(threads)
    return out.detach(), dict(zip(names, grads)), cot, norm.detach()


def gpu_run(S, c, cot, subset=None):
    lv = {k: None if c[k] is None else TG.dev(c[k]) for k in NAMES}
    if c["option"] == "shared":
        lv["end_fs"], lv["z_end"] = lv["start_fs"], lv["z_start"]
    names = leaf_names(c)
    for k in (names if subset is None else subset):
        lv[k].requires_grad_(True)
    out = S.splat_blend(*[lv[k] for k in NAMES], TG.dev(c["alpha"]), **c["opts"])
    out.backward(cot.cuda())
    return out.detach(), {k: lv[k].grad for k in names}


def shares(r64):
    return {k: float((r.abs() >= 1e-3 * float(r.abs().max())).double().mean()) for k, r in r64.items()}


def meets_condition(r64):
    return all(bool(torch.isfinite(r).all()) for r in r64.values()) and min(shares(r64).values()) >= 0.30


def dropped(flow):
    """Sources whose target coordinate is not representable (tests/splat_f64.py: non-finite or |.| >= 2^30)."""
    N, _, H, W = flow.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(x + flow[:, 0]) < 2.0 ** 30) & (np.abs(y + flow[:, 1]) < 2.0 ** 30)
    return torch.from_numpy(~ok)[:, None]


def check_case(S, c, where, group="blend"):
    """False (nothing asserted) when the inputs miss the condition; else out and the gradients by the criterion, exact zeros in holes of
    the output and at dropped sources.  -> dict of the float64 / float32 references, the cotangent and the GPU's results."""
    out64, r64, cot, norm64 = reference(c, torch.float64)
    if not meets_condition(r64):
        return False
    print(f"  {where}: shares >= 1e-3 max: " + "  ".join(f"{k} {v:.2f}" for k, v in shares(r64).items()))
    out32, r32, _, _ = reference(c, torch.float32, cot)
    out, g = gpu_run(S, c, cot)
    TG.judge(group, "out", out, out32, out64, where)
    for k in r64:
        TG.judge(group, k, g[k], r32[k], r64[k], where)
    holes = (norm64 == 0.0).expand_as(out64)
    assert bool((out.cpu()[holes] == 0.0).all()) and not bool(torch.signbit(out.cpu()[holes]).any()), (where, "holes of out are not +0.0")
    for d, names in (("flow_f", ("start_fs", "z_start", "flow_f")), ("flow_p", ("end_fs", "z_end", "flow_p"))):
        if c["option"] == "shared":
            names = (d,)                                 # (a shared tensor's gradient is the sum over both directions)
        m = dropped(c[d])
        for k in names:
            if k in g:
                assert bool((g[k].cpu()[m.expand_as(g[k])] == 0).all()), (where, k, "gradient at a dropped source")
    return dict(out64=out64, r64=r64, out32=out32, r32=r32, cot=cot, out=out, g=g, norm64=norm64)


SHAPES = ((2, 64, 256, 256), (2, 65, 256, 256), (1, 64, 256, 480), (2, 6, 40, 72), (1, 17, 9, 65), (2, 3, 5, 7), (1, 1, 1, 1), (1, 16, 768, 1280))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_euler_flows_at_every_shape(S, oracle, shape):
    """Euler t = 30 / 59 of smooth_motion, default options; [2,64,256,256] is the main case (asserted as it is: no re-seeding),
    [1,16,768,1280] the timed grid with a channel count whose float64 run fits in memory."""
    for attempt in range(60):
        seed, amp = 2025 + 100000 * attempt, 2.0 * 0.5 ** (attempt // 3)
        c = euler_case(oracle, shape, seed, amp)
        where = f"euler {'x'.join(str(v) for v in shape)} seed {seed} amplitude {amp:g}"
        if check_case(S, c, where):
            break
        assert shape != SHAPES[0], "the main case misses the condition on the inputs"
    else:
        raise AssertionError(f"no seed / amplitude of {shape} meets the condition on the inputs")


KINDS = ("uniform3", "integer", "collapse", "nan")
FAMILY_CASES = [(k, s) for k in KINDS for s in ((2, 6, 40, 72), (1, 17, 9, 65), (2, 3, 5, 7))] + [("uniform3", (1, 64, 256, 480)), ("nan", (2, 64, 256, 256))]


@pytest.mark.parametrize("kind,shape", FAMILY_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(str(n) for n in v))
def test_flow_families(S, oracle, kind, shape):
    """Uniform +-3, integer, collapsing flows and 2 % NaN / inf entries (test_gpu_gradients.family_case)."""
    for attempt in range(60):
        seed, s = 7000 + 1000 * KINDS.index(kind) + 10 * SHAPES.index(shape) + 100000 * attempt, 0.5 ** (attempt // 3)
        c = family(oracle, kind, shape, seed, s)
        where = f"{kind} {'x'.join(str(v) for v in shape)} seed {seed} amplitude {s:g}"
        res = check_case(S, c, where)
        if res:
            break
    else:
        raise AssertionError(f"no seed / amplitude of {kind} {shape} meets the condition on the inputs")
    norm64 = res["norm64"]
    if kind == "collapse" and shape[2] >= 40:
        assert bool((norm64 == 0).any()), "a collapsing flow leaves destinations that nobody reaches"
    if kind == "nan" and shape[2] * shape[3] >= 64:
        assert bool(dropped(c["flow_f"]).any()) and bool(dropped(c["flow_p"]).any())


@pytest.mark.parametrize("shape", ((2, 64, 256, 256), (2, 6, 40, 72)), ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("option", ("v1", "noclamp", "znone", "shared"))
def test_options(S, oracle, option, shape):
    """subtract_max=False, clamp_z=None, z_* = None, one tensor shared by both directions -- on Euler flows, and at the small shape on
    flows with NaN / inf entries."""
    for kind in ("euler", "nan") if shape[2] < 256 else ("euler",):
        for attempt in range(60):
            seed, s = 2025 + 100000 * attempt, 0.5 ** (attempt // 3)
            c = euler_case(oracle, shape, seed, 2.0 * s, option) if kind == "euler" else family(oracle, "nan", shape, 9000 + seed, s, option)
            if check_case(S, c, f"{option} {kind} {'x'.join(str(v) for v in shape)} seed {seed} amplitude {s:g}"):
                break
        else:
            raise AssertionError(f"no seed / amplitude of {option} {kind} {shape} meets the condition on the inputs")


def chain(S, c, cot):
    """The composed chain of test_training_step_chain_gradients from the displacement fields on, generalised to two feature / logit
    tensors, built from the package's unchanged drop-ins."""
    lv = {k: TG.dev(c[k]).requires_grad_(True) for k in NAMES}
    B, _, H, W = c["start_fs"].shape
    a = TG.dev(c["alpha"]).view(B, 1, 1, 1)
    splat = S.ModuleSoftsplat("summation")
    ones = lv["start_fs"].new_ones((B, 1, H, W))
    Zf = torch.clamp(lv["z_start"] - lv["z_start"].max(), min=-20.0, max=20.0)
    ten_f = torch.cat([lv["start_fs"] * Zf.exp() * a, Zf.exp() * a], 1)
    gen_f = splat(tenInput=ten_f, tenFlow=lv["flow_f"], tenMetric=ones)
    ten_norm, gen = gen_f[:, -1:, :, :], gen_f[:, :-1, :, :]
    Zp = torch.clamp(lv["z_end"] - lv["z_end"].max(), min=-20.0, max=20.0)
    ten_p = torch.cat([lv["end_fs"] * Zp.exp() * (1 - a), Zp.exp() * (1 - a)], 1)
    gen_p = splat(tenInput=ten_p, tenFlow=lv["flow_p"], tenMetric=ones)
    ten_norm += gen_p[:, -1:, :, :]
    gen += gen_p[:, :-1, :, :]
    gen = gen / torch.clamp(ten_norm, min=1e-8)
    gen.backward(cot.cuda())
    return gen.detach(), {k: lv[k].grad for k in NAMES}


def plant_blocks(c):
    """A block of z_start and one of z_end at -30: Z - max < -20, the clamp bites, no gradient there."""
    c = dict(c, z_start=c["z_start"].copy(), z_end=c["z_end"].copy())
    c["z_start"][0, 0, 40:56, 100:140] = -30.0
    c["z_end"][1, 0, 200:230, 10:60] = -30.0
    return c


def test_main_case_against_the_composed_chain(S, oracle):
    """The main case through splat_blend and through the composed chain, both judged by the criterion, their E side by side."""
    c = euler_case(oracle, SHAPES[0])
    res = check_case(S, c, "main")
    assert res, "the main case misses the condition on the inputs"
    out64, r64, out32, r32, cot, out, g = (res[k] for k in ("out64", "r64", "out32", "r32", "cot", "out", "g"))
    cout, cg = chain(S, c, cot)
    E = lambda got, ref: float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())
    print("  main case, E against float64:      splat_blend   composed chain   plain float32")
    print(f"    {'out':>9s}  {E(out, out64):.3e}  {E(cout, out64):.3e}  {E(out32, out64):.3e}")
    for k in NAMES:
        print(f"    {k:>9s}  {E(g[k], r64[k]):.3e}  {E(cg[k], r64[k]):.3e}  {E(r32[k], r64[k]):.3e}")
    TG.judge("chain2", "out", cout, out32, out64, "main")
    for k in NAMES:
        TG.judge("chain2", k, cg[k], r32[k], r64[k], "main")


def test_clamped_blocks_and_the_maximums_correction(S, oracle):
    """With a block of z_start and one of z_end at -30 the gradient is exactly 0 on the blocks, and the element that holds the maximum
    carries minus the sum of everybody's gradient (float64: printed; the largest element of dL/dZ)."""
    c = plant_blocks(euler_case(oracle, SHAPES[0]))
    res = check_case(S, c, "main + clamp blocks")
    assert res, "the main case with the blocks planted misses the condition on the inputs"
    r64, r32, g = res["r64"], res["r32"], res["g"]
    assert bool((g["z_start"][0, 0, 40:56, 100:140] == 0).all()) and bool((g["z_end"][1, 0, 200:230, 10:60] == 0).all())
    assert bool((r64["z_start"][0, 0, 40:56, 100:140] == 0).all()) and bool((r64["z_end"][1, 0, 200:230, 10:60] == 0).all())
    for k in ("z_start", "z_end"):
        j = int(np.argmax(c[k]))
        ref, got, got32 = float(r64[k].reshape(-1)[j]), float(g[k].reshape(-1)[j]), float(r32[k].reshape(-1)[j])
        scale = float(r64[k].abs().max())
        print(f"  d/d{k} at the maximum's element: float64 {ref:.6f}  GPU {got:.6f}  plain float32 {got32:.6f}  (max|d/d{k}| {scale:.6f})")
        # (a statement about the reference: being the largest element, the correction is what the criterion above judged d/dZ by)
        assert int(r64[k].abs().reshape(-1).argmax()) == j, "the correction is not the largest element of the gradient"
        # d/dZ sums to zero (the output does not change when a constant is added to Z, as long as the same elements stay clamped): the
        # correction is minus the sum of everybody else's gradient.  Tolerance: 2^17 float32 terms below `scale`, each stored with a
        # relative error of 2^-24, and the correction's own rounding -- far below 1e-3 of the scale.
        assert abs(float(g[k].double().sum())) <= 1e-3 * scale


def test_every_subset_of_gradients_gives_the_same_bits(S, oracle):
    """All 63 subsets of the six gradient pointers through the raw C ABI on the same saved tensors: bit-identical to the full call;
    the autograd route returns None for inputs that do not require grad."""
    from slr_sfs_amd._lib import check, lib, ptr, stream_of
    L = lib()
    c = plant_blocks(euler_case(oracle, SHAPES[0]))
    c["flow_f"][0, 0, 7, 9], c["flow_p"][1, :, 100, 100] = np.nan, np.inf
    N, C, H, W = c["start_fs"].shape
    T = {k: TG.dev(c[k]) for k in NAMES}
    alpha, go = TG.dev(c["alpha"]), TG.dev(c["go"])
    out, norm = S.splat_blend(*[T[k] for k in NAMES], alpha, return_norm=True)
    zmax = [S.training._global_max(T["z_start"]), S.training._global_max(T["z_end"])]
    assert float(zmax[0]) == float(c["z_start"].max()) and float(zmax[1]) == float(c["z_end"].max())
    nb = int(L.slr_splat_blend_ws_bytes(N, C, H, W))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")

    def backward(want):
        gr = [torch.full_like(T[k], float("nan")) if k in want else None for k in NAMES]
        check(L.slr_splat_blend_backward(*[ptr(T[k]) for k in NAMES], ptr(alpha), ptr(zmax[0]), ptr(zmax[1]), -20.0, 20.0, 1e-8, ptr(out), ptr(norm),
                                         ptr(go), *[ptr(t) for t in gr], N, C, H, W, ptr(scratch), nb, stream_of(out)), str(want))
        return dict(zip(NAMES, gr))
    full = backward(NAMES)
    again = backward(NAMES)
    for k in NAMES:
        assert bool(torch.isfinite(full[k]).all()) and torch.equal(full[k], again[k]), (k, "not reproducible")
    for r in range(1, 6):
        for want in itertools.combinations(NAMES, r):
            got = backward(want)
            for k in NAMES:
                assert (got[k] is None) if k not in want else torch.equal(got[k], full[k]), (want, k)
    for subset in (("start_fs",), ("z_end", "flow_f"), ("flow_p",), ("end_fs", "z_start", "z_end")):
        _, g = gpu_run(S, c, go.cpu(), subset)
        for k in NAMES:
            assert (g[k] is not None) == (k in subset), (subset, k)
    # without logits there is nothing to differentiate them by: the ABI refuses the pointer, the autograd route has no such input
    rc = L.slr_splat_blend_backward(ptr(T["start_fs"]), None, ptr(T["flow_f"]), ptr(T["end_fs"]), None, ptr(T["flow_p"]), ptr(alpha), None, None, -20.0, 20.0,
                                    1e-8, ptr(out), ptr(norm), ptr(go), None, ptr(full["z_start"]), None, None, None, None, N, C, H, W, ptr(scratch), nb,
                                    stream_of(out))
    assert rc == -1


def test_training_synthesis_without_a_host_synchronisation(S, oracle, monkeypatch):
    """TrainingSynthesis forward + backward on [2,64,256,256] with the index tensors on the device under set_sync_debug_mode("error");
    out, d/dfs, d/dZ by the criterion, d/dmotion by the bound of test_training_step_chain_gradients (summation order of the Euler
    backward over both directions' terms plus the difference of the field gradients carried along the same paths)."""
    import argparse
    c = euler_case(oracle, SHAPES[0])
    out64, r64, cot, _ = reference(c, torch.float64)
    assert meets_condition(r64)
    out32, r32, _, _ = reference(c, torch.float32, cot)
    B, t, mo = 2, c["t"], c["motion"]
    seen = {}
    orig = S.training.splat_blend

    def spy(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, **kw):
        if flow_f.requires_grad:
            flow_f.retain_grad()
            flow_p.retain_grad()
        seen.update(flow_f=flow_f, flow_p=flow_p, alpha=alpha, kw=kw)
        return orig(start_fs, z_start, flow_f, end_fs, z_end, flow_p, alpha, **kw)
    monkeypatch.setattr(S.training, "splat_blend", spy)
    model = S.TrainingSynthesis(argparse.Namespace(train_Z=True))
    lv = {k: TG.dev(c[k]).requires_grad_(True) for k in ("start_fs", "z_start", "end_fs", "z_end")}
    mo_d, cot_d = TG.dev(mo).requires_grad_(True), cot.cuda()
    start, middle, end = torch.zeros(B).cuda(), torch.tensor([float(v) for v in t]).cuda(), torch.full((B,), NF - 1.0).cuda()
    S.splat_blend(*[TG.dev(c[k]) for k in NAMES], TG.dev(c["alpha"]))          # (the cached workspace exists before the guarded region)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = model(lv["start_fs"], lv["z_start"], lv["end_fs"], lv["z_end"], mo_d, start, middle, end)
        (out * cot_d).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert seen["kw"] == dict(clamp_z=(-20.0, 20.0), subtract_max=True)
    assert np.array_equal(TG.host(seen["alpha"]), c["alpha"])
    assert np.array_equal(TG.host(seen["flow_f"]), c["flow_f"]) and np.array_equal(TG.host(seen["flow_p"]), c["flow_p"])
    TG.judge("module", "out", out.detach(), out32, out64, "TrainingSynthesis")
    for k in lv:
        TG.judge("module", k, lv[k].grad, r32[k], r64[k], "TrainingSynthesis")
    for k in ("flow_f", "flow_p"):
        TG.judge("module", k, seen[k].grad, r32[k], r64[k], "TrainingSynthesis")
    gf_ref, gp_ref = r64["flow_f"].float().numpy(), r64["flow_p"].float().numpy()
    gf_gpu, gp_gpu = TG.host(seen["flow_f"].grad), TG.host(seen["flow_p"].grad)
    gm = TG.host(mo_d.grad)
    for b in range(B):
        mb, nf, np_ = mo[b:b + 1], t[b], NF - t[b]
        ref = oracle.euler_backward(mb, nf, gf_ref[b:b + 1]) - oracle.euler_backward(-mb, np_, gp_ref[b:b + 1])
        Af, Kf = TG.euler_bound(oracle, mb, nf, gf_ref[b:b + 1])
        Ap, Kp = TG.euler_bound(oracle, -mb, np_, gp_ref[b:b + 1])
        carried = oracle.euler_backward(mb, nf, np.abs(gf_gpu[b:b + 1] - gf_ref[b:b + 1])) + \
            oracle.euler_backward(-mb, np_, np.abs(gp_gpu[b:b + 1] - gp_ref[b:b + 1]))
        bound = 2.0 * np.maximum(Kf + Kp - 1.0, 0.0) * 2.0 ** -24 * (Af + Ap) + 1e-7 + carried
        dev_ = np.abs(gm[b:b + 1] - ref)
        print(f"  TrainingSynthesis d/dmotion sample {b}: max|dev| {float(dev_.max()):.3e}, max|ref| {float(np.abs(ref).max()):.3e}, "
              f"max dev/bound {float((dev_ / bound).max()):.3f}, max carried {float(carried.max()):.3e}")
        assert float(np.abs(ref).max()) > 1.0
        assert (dev_ <= bound).all(), (b, float((dev_ - bound).max()))
    # train_Z off: the logits are ignored (weights alpha / 1 - alpha)
    plain = S.TrainingSynthesis()(TG.dev(c["start_fs"]), None, TG.dev(c["end_fs"]), None, TG.dev(mo), start, middle, end)
    ref0 = B64.blend_f64(torch.from_numpy(c["start_fs"]), None, torch.from_numpy(c["flow_f"]), torch.from_numpy(c["end_fs"]), None,
                         torch.from_numpy(c["flow_p"]), torch.from_numpy(c["alpha"]))
    assert float((plain.cpu().double() - ref0).abs().max()) <= 1e-5 * float(ref0.abs().max())
