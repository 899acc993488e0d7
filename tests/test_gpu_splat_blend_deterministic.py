"""``splat_blend(..., deterministic=True)`` on the GPU: the same bits from run to run, the same bits whoever builds a record list, and
still the definition of tests/blend_f64.py.

The cases and the paths their flows take are tests/blend_det_cases.py's; every case's conditions are evaluated with numpy and asserted
before the GPU is used (``_case``), and once more without a GPU in tests/test_splat_blend_deterministic_host.py.

1. repeat     16 deterministic calls, 8 of them while a second stream runs a loop of matmuls: ``torch.equal`` on `out` and the
              normaliser; the workspace's fallback count reads 0 afterwards.  The DEFAULT operator's number of distinct results over the
              same 16 calls is printed, never asserted (it would fail by chance): it is what shows that the case can see the problem.
2. same list  scan front end, 32 channels, 1 / 2 / 4 channel groups per tile (slr_splat_set_scan_shape): every plane bit-equal.  Each
              group's workgroup builds the tile's lists itself; only a canonical order makes them agree.
3. right      `out` and all six gradients by the project's criterion E_gpu <= 10 E_plain32 + 1e-6 against float64
              (test_gpu_splat_blend.check_case, with the deterministic operator in the package's place), exact zeros in holes and at
              dropped sources.  Against the definition, never against the default operator.
4. iteration  two ``Trainer`` iterations (discriminator, deferred gradient pair, two accumulation steps) of
              ``TrainingModel(..., deterministic=True)`` from the same state WITHOUT ``_SameSplat``, under
              ``set_sync_debug_mode("error")``: every loss, PredImg, the 141 generator gradients, every tensor of the state and both
              optimisers' states bit-equal.  The default operator's largest PredImg difference over the same pair is printed.

Distinct results of the default operator over 16 calls, measured on an MI355X: see DESIGN 3.7 ("deterministic forward")."""
import functools

import numpy as np
import pytest
import torch

import blend_det_cases as K

pytestmark = pytest.mark.gpu

FRONT = {"scan": 1, "rows": 2}
REPEATS = 16


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


class _front_end:
    """slr_splat_set_front_end (and the scan shape) for the block, restored afterwards."""

    def __init__(self, S, name, groups=0):
        self.L, self.fe, self.groups = S._lib.lib(), FRONT[name], groups

    def __enter__(self):
        self.prev = self.L.slr_splat_set_front_end(self.fe)
        self.L.slr_splat_set_scan_shape(0, self.groups, 0, 0)

    def __exit__(self, *exc):
        self.L.slr_splat_set_scan_shape(0, 0, 0, 0)
        self.L.slr_splat_set_front_end(self.prev)
        return False


@functools.lru_cache(maxsize=None)
def _case_cached(name, channels, option):
    from oracle import oracle as o
    o.build()
    c = K.make_case(name, o, channels=channels, option=option)
    for what, ok in K.conditions(name, c):
        assert ok, (name, what)
    return c


def _case(name, channels=None, option="default"):
    return _case_cached(name, channels, option)


def _tensors(c):
    import test_gpu_splat_blend as SB
    import test_gpu_gradients as TG
    lv = {k: None if c[k] is None else TG.dev(c[k]) for k in SB.NAMES}
    if c["option"] == "shared":
        lv["end_fs"], lv["z_end"] = lv["start_fs"], lv["z_start"]
    return [lv[k] for k in SB.NAMES] + [TG.dev(c["alpha"])]


def _forward(S, args, c, deterministic):
    return S.splat_blend(*args, return_norm=True, deterministic=deterministic, **c["opts"])


def _busy(side, a, n):
    with torch.cuda.stream(side):
        for _ in range(n):
            a = (a @ a) * 1e-3
    return a


def _repeat(S, c, front, where):
    args = _tensors(c)
    side, a = torch.cuda.Stream(), torch.randn(2048, 2048, device="cuda")
    with _front_end(S, front):
        count = S.training.splat_blend_fallback_count(args[0])
        before = int(count.item())
        results = {}
        for det in (True, False):
            runs = [_forward(S, args, c, det) for _ in range(REPEATS // 2)]
            torch.cuda.synchronize()
            _busy(side, a, 150)                                     # (enqueued: they run while the calls below do)
            runs += [_forward(S, args, c, det) for _ in range(REPEATS // 2)]
            torch.cuda.synchronize()
            results[det] = runs
        after = int(count.item())
    distinct = lambda runs: len({(o.cpu().numpy().tobytes(), n.cpu().numpy().tobytes()) for o, n in runs})   # noqa: E731
    worst = max(float((o - results[False][0][0]).abs().max()) for o, _ in results[False])
    print(f"  {where}: distinct results over {REPEATS} calls: default {distinct(results[False])} (largest difference {worst:.3e}), "
          f"deterministic {distinct(results[True])}; fallback count {before} -> {after}")
    o0, n0 = results[True][0]
    assert bool(torch.isfinite(o0).all()) and bool(torch.isfinite(n0).all())
    for k, (o, n) in enumerate(results[True]):
        assert torch.equal(o, o0) and torch.equal(n, n0), (where, "deterministic call", k, float((o - o0).abs().max()), float((n - n0).abs().max()))
    assert before == 0 and after == 0, (where, "capacity fallbacks", before, after)


def _right(S, c, front, where, monkeypatch):
    import test_gpu_splat_blend as SB

    class Det:                                                       # the package, with the deterministic operator in splat_blend's place
        splat_blend = staticmethod(lambda *a, **k: S.splat_blend(*a, deterministic=True, **k))
    real = SB.reference
    memo = c.setdefault("_reference", {})                            # the float64 / float32 definitions: once per case

    def reference(c_, dtype, cot=None):
        if dtype not in memo:
            memo[dtype] = real(c_, dtype, cot)
        return memo[dtype]
    monkeypatch.setattr(SB, "reference", reference)
    with _front_end(S, front):
        res = SB.check_case(Det, c, where)
    assert res, (where, "the inputs miss the condition on the gradients (tests/test_gpu_splat_blend.py)")
    return res


CASES = [(name, fe) for name in K.CASES for fe in K.CASES[name]["front_ends"]]


@pytest.mark.parametrize("name,front", CASES, ids=lambda v: v)
def test_sixteen_calls_give_the_same_bits(S, name, front):
    _repeat(S, _case(name), front, f"{name} {front}")


@pytest.mark.parametrize("name,front", CASES, ids=lambda v: v)
def test_deterministic_forward_against_float64(S, name, front, monkeypatch):
    _right(S, _case(name), front, f"{name} {front} deterministic", monkeypatch)


@pytest.mark.parametrize("name", ("plain", "row_pile", "sink"))
def test_same_bits_whoever_builds_the_lists(S, name):
    """1, 2 and 4 channel groups per tile of the scan front end on the 32-channel form."""
    c = _case(name, channels=32)
    args = _tensors(c)
    got = {}
    for g in (1, 2, 4):
        with _front_end(S, "scan", groups=g):
            got[g] = _forward(S, args, c, True)
            torch.cuda.synchronize()
    for g in (2, 4):
        for k, what in enumerate(("out", "norm")):
            d = (got[g][k] != got[1][k]).reshape(got[g][k].shape[0], got[g][k].shape[1], -1).any(-1)
            assert torch.equal(got[g][k], got[1][k]), (name, what, f"{g} channel groups against 1: planes that differ", d.nonzero().tolist()[:8])
    assert int(S.training.splat_blend_fallback_count(args[0]).item()) == 0


@pytest.mark.parametrize("option", ("znone", "shared", "v1", "noclamp"))
@pytest.mark.parametrize("name", ("plain", "sink"))
def test_options(S, name, option, monkeypatch):
    """Every weight form of the RAW kernels: no logits, shared tensors, nothing subtracted, no clamp."""
    c = _case(name, option=option)
    _repeat(S, c, "scan", f"{name} {option}")
    _right(S, c, "scan", f"{name} {option} deterministic", monkeypatch)


def test_a_capacity_fallback_is_counted_and_still_right(S):
    """A grid forced onto the scan front end with the small pools, every reached tile a sink: the deferred pieces do not all find room in
    the entry array.  The default operator does not count; every deterministic call does, the word only grows, and `out` is still the
    definition's (the fallbacks are other summation trees, not other results).  Bit-equality is not promised here and not asserted."""
    import blend_f64 as B64
    import test_gpu_gradients as TG
    import test_gpu_splat_blend as SB
    c = SB.with_option(K.fallback_case(), "default")
    for what, ok in K.fallback_conditions(c):
        assert ok, what
    cpu = [None if c[k] is None else torch.from_numpy(c[k]) for k in SB.NAMES]
    out64 = B64.blend_f64(*[None if t is None else t.double() for t in cpu], torch.from_numpy(c["alpha"]), torch.float64)
    out32 = B64.blend_f64(*cpu, torch.from_numpy(c["alpha"]), torch.float32)
    args = _tensors(c)
    with _front_end(S, "scan"):
        count = S.training.splat_blend_fallback_count(args[0])
        assert count.dtype == torch.int32 and count.is_cuda and count.numel() == 1
        S.splat_blend(*args)
        c0 = int(count.item())
        out = S.splat_blend(*args, deterministic=True)
        c1 = int(count.item())
        S.splat_blend(*args, deterministic=True)
        c2 = int(count.item())
    print(f"  fallback count: after a default call {c0}, after one deterministic call {c1}, after two {c2}")
    assert c0 == 0 and c1 > 0 and c2 > c1
    TG.judge("blend", "out", out, out32, out64, "capacity fallback, deterministic")


def test_argument_is_a_bool_on_the_device_too(S):
    c = _case("plain")
    args = _tensors(c)
    with pytest.raises(TypeError):
        S.splat_blend(*args, deterministic=1)
    with pytest.raises(TypeError):
        S.TrainingSynthesis(None, deterministic="yes")


# ------------------------------------------------------------------ the whole iteration

def _iteration(S, deterministic):
    import test_gpu_train_step as TS
    import train_step_f64 as T
    opts = T.options(discriminator_losses="pix2pixHD")
    model = S.TrainingModel(opts, TS._vgg(S), encoder_widths=T.ENC_WIDTHS, decoder_widths=T.DEC_WIDTHS, decoder_updown=T.UPDOWN,
                            deterministic=deterministic)
    torch.manual_seed(T.DISC_SEED)
    trainer = S.Trainer(model, opts).to(TS.DEV).train()
    model.load_reference_state_dict(TS._fixture()[1])
    model.defer_weight_grad(True)
    opt, out = trainer.optimizers, {}
    gen = lambda: {"model.module." + k: t for k, t, learns in trainer.model.reference_parameters() if learns}          # noqa: E731
    step = opt.optimizer_G.step

    def recording(*a, **k):
        out["grads_G"] = TS._snapshot((k_, t.grad) for k_, t in gen().items())
        return step(*a, **k)
    opt.optimizer_G.step = recording
    batches = TS._batches(2)
    torch.cuda.synchronize()
    with TS._no_sync():
        losses, images = trainer(iter(batches), num_steps=2)
    out["losses"] = TS._snapshot(losses.items())
    out["PredImg"] = {"PredImg": images["PredImg"].detach().clone()}
    out["tensors"] = dict(trainer.reference_state_dict())
    out["state_G"] = {k: TS._snapshot(opt.optimizer_G.state[t].items()) for k, t in gen().items()}
    out["state_D"] = {"netD." + k: TS._snapshot(opt.optimizer_D.state[p].items()) for k, p in trainer.netD.named_parameters()}
    return out


def test_two_whole_iterations_are_bit_equal(S):
    import test_gpu_train_step as TS
    import train_step_f64 as T
    S.splat_blend(*_tensors(_case("plain")), deterministic=True)          # (the library's kernels are loaded before the guarded region)
    torch.cuda.synchronize()
    a, b = _iteration(S, True), _iteration(S, True)
    assert len(a["grads_G"]) == 141 and all(g is not None for g in a["grads_G"].values())
    for part in ("losses", "PredImg", "grads_G", "tensors", "state_G", "state_D"):
        TS._same(a[part], b[part], part)
    img = TS._batches(1)[0]["images"][0]
    feats = img.new_empty(img.shape[0], T.FEAT, *img.shape[2:])
    assert int(S.training.splat_blend_fallback_count(feats).item()) == 0
    assert all(bool(torch.isfinite(v).all()) for v in a["losses"].values())
    x, y = _iteration(S, False), _iteration(S, False)
    print(f"  two iterations, default operator, no _SameSplat: largest PredImg difference "
          f"{float((x['PredImg']['PredImg'] - y['PredImg']['PredImg']).abs().max()):.3e}; deterministic operator: 0 (asserted)")
    print(f"  deterministic against default, PredImg: {float((a['PredImg']['PredImg'] - x['PredImg']['PredImg']).abs().max()):.3e}")
