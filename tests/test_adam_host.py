"""The optimiser step without a device: the C ABI of csrc/adam.hip (declarations, argument errors, the plan slr_adam_plan_fill writes,
decoded from the layout include/slr_splat.h documents), the refusals of slr_sfs_amd.Adam, the reference's rules in TrainingOptimizers,
and the criterion of tests/test_gpu_adam.py held against the formulas it has to tell apart.  Figures are printed (run with -s)."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_f64 as A64
from slr_sfs_amd import optim  # noqa: F401  (without the optimiser nothing here can run: fail at import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("slr_adam_plan_bytes", "slr_adam_plan_fill", "slr_adam_step")
P = 0x10000                                             # a 16-byte aligned non-null "pointer": nothing dereferences it on these paths


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def test_entry_points_are_declared_in_the_header_and_the_signature_table(L):
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.ABI_VERSION >= 19 and L.slr_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+SLR_ADAM_ZERO_GRADS\s+(\d+)", hdr).group(1)) == 1
    assert optim.ZERO_GRADS == 1


# ------------------------------------------------------------------ argument errors

def _refused(L, rc, *words):
    msg = L.slr_last_error()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def test_step_refuses_bad_arguments_before_anything_is_launched(L):
    def step(plan=P, n=3, n_work=5, lr=P, betas=(0.9, 0.999), eps=1e-8, flags=0):
        b = None if betas is None else (ctypes.c_double * 2)(*betas)
        return L.slr_adam_step(plan, n, n_work, lr, b, eps, flags, None)

    _refused(L, step(plan=None), b"slr_adam_step", b"null")
    _refused(L, step(lr=None), b"slr_adam_step", b"null")
    _refused(L, step(betas=None), b"slr_adam_step", b"null")
    for n in (0, -1):
        _refused(L, step(n=n), b"slr_adam_step", b"n_tensors")
    _refused(L, step(n_work=-1), b"slr_adam_step", b"n_work")
    for betas in ((1.0, 0.9), (0.9, 1.0), (-0.1, 0.9), (0.9, -1e-9), (float("nan"), 0.9), (0.9, 1.5)):
        _refused(L, step(betas=betas), b"slr_adam_step", b"betas")
    for eps in (0.0, -1e-8, float("nan")):
        _refused(L, step(eps=eps), b"slr_adam_step", b"eps")
    for flags in (2, 3, 4, -1, 1 << 16):
        _refused(L, step(flags=flags), b"slr_adam_step", b"flags")
    _refused(L, step(plan=P + 8), b"slr_adam_step", b"aligned")


def _arrays(numel, base=P):
    """Made-up addresses, 4-byte aligned and distinct per tensor and stream: [5][n] (p, g, m, v, step) and the element counts."""
    n = len(numel)
    addr = np.empty((5, n), dtype=np.uint64)
    for k in range(5):
        addr[k] = base + (k << 40) + 4 * np.arange(n, dtype=np.uint64) * (1 << 16)
    return addr, np.asarray(numel, dtype=np.int64)


def _fill(L, numel, nbytes=None, n=None, null=None):
    addr, cnt = _arrays(numel)
    need = L.slr_adam_plan_bytes(len(numel), cnt.ctypes.data)
    buf = np.full(max(need, 64) + 64, 0xAB, dtype=np.uint8)            # 64 guard bytes behind the plan
    ptrs = [addr[k].ctypes.data for k in range(5)] + [cnt.ctypes.data]
    if null is not None:
        ptrs[null] = None
    rc = L.slr_adam_plan_fill(buf.ctypes.data, need if nbytes is None else nbytes, len(numel) if n is None else n, *ptrs)
    return rc, buf, need, addr, cnt


def test_plan_fill_refuses_bad_arguments(L):
    numel = [5, 0, 70]
    rc, _, need, _, cnt = _fill(L, numel)
    assert rc == 0 and need > 0
    _refused(L, _fill(L, numel, nbytes=need - 1)[0], b"slr_adam_plan_fill", b"bytes")
    _refused(L, _fill(L, numel, nbytes=0)[0], b"slr_adam_plan_fill", b"bytes")
    for n in (0, -2):
        _refused(L, _fill(L, numel, n=n)[0], b"slr_adam_plan_fill", b"n ")
    for k in range(6):
        _refused(L, _fill(L, numel, null=k)[0], b"slr_adam_plan_fill", b"null")
    assert L.slr_adam_plan_fill(None, need, 3, P, P, P, P, P, cnt.ctypes.data) == -1
    _refused(L, _fill(L, [5, -1])[0], b"slr_adam_plan_fill", b"numel")
    assert L.slr_adam_plan_bytes(0, cnt.ctypes.data) == 0 and L.slr_adam_plan_bytes(3, None) == 0
    bad = np.array([4, -1], dtype=np.int64)
    assert L.slr_adam_plan_bytes(2, bad.ctypes.data) == 0


# ------------------------------------------------------------------ the plan, decoded from the documented layout

def _decode(buf, need):
    """(header dict, tensor records [n][6] uint64, work records as (tensor, count, start) arrays, scratch bytes), read with numpy from the
    layout of include/slr_splat.h alone."""
    magic, chunk, n, n_work = buf[:16].view(np.uint32)
    tensors_off, work_off, scratch_off, nbytes = (int(x) for x in buf[16:48].view(np.uint64))
    assert not buf[48:64].any()
    align = lambda v, a: (v + a - 1) // a * a                              # noqa: E731
    n, n_work = int(n), int(n_work)
    assert tensors_off == 64 and work_off == align(64 + 48 * n, 16) and scratch_off == align(work_off + 16 * n_work, 16)
    assert nbytes == align(scratch_off + 8 * n, 256) == need
    tens = buf[tensors_off:tensors_off + 48 * n].view(np.uint64).reshape(n, 6)
    assert not buf[tensors_off + 48 * n:work_off].any()
    work = buf[work_off:work_off + 16 * n_work]
    w32 = work.view(np.int32).reshape(n_work, 4)
    start = work.view(np.int64).reshape(n_work, 2)[:, 1]
    assert not buf[work_off + 16 * n_work:nbytes].any()                   # padding and the scratch table start as zeros
    return dict(magic=int(magic), chunk=int(chunk), n=n, n_work=n_work, bytes=nbytes), tens, (w32[:, 0], w32[:, 1], start)


def _plan_lists():
    C = A64.chunk()
    return {"sizes": A64.sizes(), "600x7": [7] * 600, "one_empty": [0], "two_chunks_exactly": [2 * C]}


@pytest.mark.parametrize("which", sorted(_plan_lists()))
def test_plan_covers_every_element_exactly_once_and_nothing_else(L, which):
    numel = _plan_lists()[which]
    C = A64.chunk()
    assert C % 1024 == 0
    rc, buf, need, addr, cnt = _fill(L, numel)
    assert rc == 0, L.slr_last_error()
    assert (buf[need:] == 0xAB).all(), "written behind the plan"
    head, tens, (wt, wc, ws) = _decode(buf[:need], need)
    assert head["magic"] == 0x4d414441 and head["chunk"] == C and head["n"] == len(numel)
    assert head["n_work"] == sum((m + C - 1) // C for m in numel)
    for t in range(len(numel)):
        assert [int(x) for x in tens[t, :5]] == [int(addr[k, t]) for k in range(5)] and int(tens[t, 5]) == numel[t]
    seen = [np.zeros(m, dtype=np.int32) for m in numel]
    for t, c, s in zip(wt, wc, ws):
        assert 0 <= t < len(numel) and 1 <= c <= C and s >= 0 and s % C == 0 and s + c <= numel[t], (t, c, s)
        seen[t][s:s + c] += 1
    assert all((a == 1).all() for a in seen)
    assert list(wt) == sorted(wt) and all(ws[i] < ws[i + 1] for i in range(len(ws) - 1) if wt[i] == wt[i + 1])
    print(f"{which}: {len(numel)} tensors, {int(sum(numel))} elements, {head['n_work']} work items, {need} bytes")


# ------------------------------------------------------------------ the Python class without a device

def test_adam_refuses_what_it_does_not_run():
    import slr_sfs_amd as S
    assert S.Adam is S.optim.Adam and S.TrainingOptimizers is S.optim.TrainingOptimizers and issubclass(S.Adam, torch.optim.Optimizer)
    with pytest.raises(NotImplementedError):
        S.Adam([torch.zeros(3, requires_grad=True)])
    with pytest.raises(TypeError):
        S.Adam([torch.zeros(3, dtype=torch.float64, requires_grad=True)])
    with pytest.raises(TypeError):
        S.Adam([torch.zeros(3, dtype=torch.float16, requires_grad=True)])
    for kw in ({"weight_decay": 1e-2}, {"amsgrad": True}, {"maximize": True}, {"weight_decay": 0.0}):
        with pytest.raises(TypeError):
            S.Adam([torch.zeros(3, requires_grad=True)], **kw)
    for kw in ({"lr": -1.0}, {"betas": (1.0, 0.9)}, {"betas": (0.9, -0.1)}, {"eps": 0.0}):
        with pytest.raises(ValueError):
            S.Adam([torch.zeros(3, requires_grad=True)], **kw)


def _host_only(monkeypatch):
    """The optimisers around CPU tensors: only what never reaches the device is used (groups, learning rates, state-dict keys)."""
    import slr_sfs_amd as S
    monkeypatch.setattr(S.optim, "_require_parameter", lambda *a, **k: None)
    return S


def test_training_optimizers_follow_the_reference(monkeypatch):
    S = _host_only(monkeypatch)
    gp, dp = [torch.zeros(3, requires_grad=True), torch.zeros(2, 2, requires_grad=True)], [torch.zeros(5, requires_grad=True)]
    # with a discriminator: both (beta1, beta2), lr_g / lr_d; the reference's defaults where opts has none
    both = S.TrainingOptimizers(gp, dp)
    assert both.optimizer_G.param_groups[0]["betas"] == (0.0, 0.9) and both.optimizer_D.param_groups[0]["betas"] == (0.0, 0.9)
    assert both.optimizer_G.param_groups[0]["lr"] == 5e-4 and both.optimizer_D.param_groups[0]["lr"] == 2e-3
    assert both.optimizer_G.param_groups[0]["eps"] == both.optimizer_D.param_groups[0]["eps"] == 1e-8
    assert [p is q for p, q in zip(both.optimizer_G.param_groups[0]["params"], gp)] == [True, True]
    assert both.optimizer_D.param_groups[0]["params"][0] is dp[0]
    # without: (0.99, beta2) whatever beta1 says
    opts = argparse.Namespace(beta1=0.5, beta2=0.95, lr_g=3e-4, lr_d=7e-4, niter_decay=4)
    alone = S.TrainingOptimizers(gp, None, opts)
    assert alone.optimizer_D is None and alone.optimizer_G.param_groups[0]["betas"] == (0.99, 0.95)
    assert alone.optimizer_G.param_groups[0]["lr"] == 3e-4
    for o in (opts, vars(opts)):                          # a Namespace or a dict
        both = S.TrainingOptimizers(gp, dp, o)
        assert both.optimizer_G.param_groups[0]["betas"] == (0.5, 0.95) == both.optimizer_D.param_groups[0]["betas"]
        assert (both.optimizer_G.param_groups[0]["lr"], both.optimizer_D.param_groups[0]["lr"]) == (3e-4, 7e-4)
    # update_learning_rate: models/base_model.py:80-93, restated
    lr_g, lr_d = 3e-4, 7e-4
    for _ in range(3):
        both.update_learning_rate()
        alone.update_learning_rate()
        lr_g, lr_d = lr_g - lr_g / 4, lr_d - lr_d / 4
        assert both.optimizer_G.param_groups[0]["lr"] == lr_g == both.lr_g == alone.optimizer_G.param_groups[0]["lr"]
        assert both.optimizer_D.param_groups[0]["lr"] == lr_d == both.lr_d
    assert alone.lr_d == 7e-4                             # (no discriminator: its rate is not touched)
    # the checkpoint's keys
    assert sorted(both.state_dict()) == ["optimizerD", "optimizerG"] and sorted(alone.state_dict()) == ["optimizerG"]
    fresh = S.TrainingOptimizers(gp, dp, opts)
    fresh.load_state_dict(dict(both.state_dict(), model="ignored"))
    assert fresh.optimizer_G.param_groups[0]["lr"] == lr_g and fresh.optimizer_D.param_groups[0]["lr"] == lr_d


def test_state_dicts_go_both_ways_between_the_classes(monkeypatch):
    """Structure only (the device test runs the steps): a torch.optim.Adam state dict with a CPU-tensor or a number as ``step`` loads,
    ``step`` becomes a float32 scalar; a group that asks for what the class does not offer is refused; this class's state dict loads into
    torch.optim.Adam, which can then step."""
    S = _host_only(monkeypatch)
    params = [torch.ones(3, requires_grad=True), torch.ones(2, 2, requires_grad=True)]
    ref = torch.optim.Adam(params, lr=2e-3, betas=(0.5, 0.9))
    for p in params:
        p.grad = torch.full_like(p, 0.25)
    ref.step(), ref.step()
    sd = ref.state_dict()
    assert not sd["state"][0]["step"].is_cuda
    ours = S.Adam(params, lr=1.0)
    ours.load_state_dict(sd)
    assert ours.param_groups[0]["lr"] == 2e-3 and ours.param_groups[0]["betas"] == (0.5, 0.9)
    for p in params:
        st = ours.state[p]
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], ref.state[p]["exp_avg"]) and st["exp_avg"].data_ptr() != ref.state[p]["exp_avg"].data_ptr()
        assert st["exp_avg_sq"].shape == p.shape and st["exp_avg_sq"].is_contiguous()
    old = ref.state_dict()
    for st in old["state"].values():
        st["step"] = 7                                    # a Python number, as old checkpoints hold it
    ours.load_state_dict(old)
    assert all(float(ours.state[p]["step"]) == 7.0 and ours.state[p]["step"].dtype == torch.float32 for p in params)
    for name, value in (("weight_decay", 1e-2), ("amsgrad", True), ("maximize", True)):
        bad = ref.state_dict()
        bad["param_groups"][0][name] = value
        with pytest.raises(TypeError, match=name):
            S.Adam(params).load_state_dict(bad)
    back = torch.optim.Adam(params, lr=1.0)
    back.load_state_dict(ours.state_dict())
    assert back.param_groups[0]["lr"] == 2e-3 and back.param_groups[0]["weight_decay"] == 0 and not back.param_groups[0]["amsgrad"]
    back.step()
    assert all(float(back.state[p]["step"]) == 8.0 for p in params)


# ------------------------------------------------------------------ the criterion has teeth on the inputs of the device test

def test_criterion_tells_the_update_from_its_usual_mistakes():
    """On the inputs of tests/test_gpu_adam.py: E_plain32 per tensor and state, and the error of two wrong formulas evaluated in float64
    -- eps inside the root, the second bias correction dropped -- against the bound 10 E_plain32 + 1e-6 the kernel is held to."""
    worst_plain = 0.0
    for si, (beta1, beta2, lr, gs, t0) in enumerate(A64.SETTINGS):
        for K in A64.KS:
            e_eps, e_bc2, e_plain = 0.0, 0.0, 0.0
            for t in A64.case(si):
                if t["p0"].numel() == 0:
                    continue
                r64, r32 = t["ref"][K, torch.float64], t["ref"][K, torch.float32]
                e_plain = max(e_plain, max(A64.E(r32[k], r64[k]) for k in range(3)))
                wrong = lambda f: A64.run(t["p0"], t["grads"][:K], t["m0"], t["v0"], t0, lr, beta1, beta2, update=f)   # noqa: E731
                e_eps = max(e_eps, A64.E(wrong(A64.step_eps_inside_sqrt)[0], r64[0]))
                e_bc2 = max(e_bc2, A64.E(wrong(A64.step_without_second_correction)[0], r64[0]))
            bound = 10 * e_plain + 1e-6
            print(f"setting {si} K {K}: E_plain32 {e_plain:.2e} bound {bound:.2e}  eps inside the root {e_eps:.2e}  "
                  f"no second correction {e_bc2:.2e}")
            # (the worst tensor of the list: a gradient element below 1e-4 of the others' size is what eps inside the root moves)
            if t0 == 0:                                  # (the resumed state: v >= 1e-3 hides eps, and 1 - 0.9^1000 = 1)
                assert e_eps > 100 * bound, (si, K, e_eps, bound)
                assert e_bc2 > 100 * bound, (si, K, e_bc2, bound)
            worst_plain = max(worst_plain, e_plain)
    assert worst_plain < 1e-6                             # the device test's bound stays within 1e-6 .. 1.1e-5: fp32 rounding, nothing else
