"""The optimiser step on the device (slr_sfs_amd.optim, csrc/adam.hip) against torch.optim.Adam's update written out in float64
(tests/adam_f64.py).

Criterion (tests/test_gpu_conv_train.py): per tensor, separately for p, exp_avg and exp_avg_sq, E = max|got - ref64| / max|ref64| and
E_gpu <= 10 * E_plain32 + 1e-6, E_plain32 the same written-out update evaluated by torch in float32 on the CPU against float64, computed
from the test's inputs and never from the kernel.  tests/test_adam_host.py measures what the bound is on these inputs (about 2e-6) and
what the usual wrong formulas miss it by.  Every result must have the same bits in two runs, on any grouping of the tensors.  Every test
prints its figures (run with -s)."""
import argparse

import pytest
import torch

import adam_f64 as A64
from slr_sfs_amd import optim  # noqa: F401  (without the optimiser nothing here can run: fail at import)
import conv_train_f64 as C64
import disc_f64 as D64

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("p", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def bound(e_plain):
    return 10.0 * e_plain + 1e-6


def held(name, got, ref64, plain32):
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    if ref64.numel() == 0:
        return
    e_gpu, e_plain = A64.E(got, ref64), A64.E(plain32, ref64)
    print(f"{name}: E_gpu {e_gpu:.3e}  E_plain32 {e_plain:.3e}  bound {bound(e_plain):.3e}")
    assert e_gpu <= bound(e_plain), (name, e_gpu, e_plain)


class _no_sync:
    """Inside: anything that synchronises the host with the device raises."""

    def __enter__(self):
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


def _dev(t):
    """A copy on the device (never the tensor itself, wherever DEV is)."""
    return torch.empty_like(t, device=DEV).copy_(t)


def _placed(values, offsets):
    """``values[i]`` on the device as a contiguous tensor of its own, or -- ``offsets[i]`` = k > 0 -- as a view at element offset k of a
    larger buffer (4 k bytes past a 16-byte boundary: the kernel's scalar path)."""
    out = []
    for v, k in zip(values, offsets):
        if k:
            buf = torch.zeros(v.numel() + 8, device=DEV)
            t = buf[k:k + v.numel()]
            t.copy_(v)
            assert t.data_ptr() % 16 == 4 * k and t.is_contiguous()
        else:
            t = _dev(v)
            assert t.numel() == 0 or t.data_ptr() % 16 == 0
        out.append(t)
    return out


def _offsets():
    n = len(A64.sizes())
    return [0] * n + [v[1] for v in A64.VIEWS], [0] * n + [v[2] for v in A64.VIEWS]


def _resumed(opt, params, ms, vs, t0):
    """The state (m, v, t0 steps taken) through load_state_dict, ``step`` as the Python number old checkpoints hold."""
    sd = opt.state_dict()
    sd["state"] = {i: dict(step=t0, exp_avg=m.clone(), exp_avg_sq=v.clone()) for i, (m, v) in enumerate(zip(ms, vs))}
    opt.load_state_dict(sd)


def _run(S, si, K, grouping="one", zero_grads=False):
    """K steps of setting ``si`` on the device.  grouping: "one" optimiser over all tensors, one "each", or one over the "flat"
    concatenation (a single tensor).  Returns per tensor (p, exp_avg, exp_avg_sq, step) on the CPU, and the gradients after the last step."""
    beta1, beta2, lr, _, t0 = A64.SETTINGS[si]
    tensors = A64.case(si)
    if grouping == "flat":
        cat = lambda key: torch.cat([t[key] for t in tensors])             # noqa: E731
        values = dict(p0=[cat("p0")], m0=[cat("m0")], v0=[cat("v0")])
        grads = [[torch.cat([t["grads"][k] for t in tensors])] for k in range(K)]
        poff = goff = [0]
    else:
        values = {key: [t[key] for t in tensors] for key in ("p0", "m0", "v0")}
        grads = [[t["grads"][k] for t in tensors] for k in range(K)]
        poff, goff = _offsets()
    params = _placed(values["p0"], poff)
    gbufs = _placed(grads[0], goff)
    for p, g in zip(params, gbufs):
        p.grad = g
    groups = [[p] for p in params] if grouping == "each" else [params]
    opts = [S.Adam(g, lr=lr, betas=(beta1, beta2)) for g in groups]
    if t0:
        for j, (o, g) in enumerate(zip(opts, groups)):
            idx = [j] if grouping == "each" else range(len(params))
            _resumed(o, g, [values["m0"][i] for i in idx], [values["v0"][i] for i in idx], t0)
    for k in range(K):
        if k:
            for g, new in zip(gbufs, grads[k]):
                g.copy_(new)                              # (the gradient tensors stay: the plan of step 1 serves every step)
        for o in opts:
            o.step(zero_grads=zero_grads)
    state = {}
    for o in opts:
        state.update(o.state)
    out = [(p.detach().cpu(), state[p]["exp_avg"].cpu(), state[p]["exp_avg_sq"].cpu(), float(state[p]["step"])) for p in params]
    return out, [g.cpu() for g in gbufs]


def _split_flat(flat, si):
    """The single flat tensor's results cut back into the tensors of the case."""
    cuts = [t["p0"].numel() for t in A64.case(si)]
    parts = [torch.split(x, cuts) for x in flat[0][:3]]
    return [(parts[0][i], parts[1][i], parts[2][i], flat[0][3]) for i in range(len(cuts))]


# ------------------------------------------------------------------ 1. the criterion

@pytest.mark.parametrize("K", A64.KS)
@pytest.mark.parametrize("si", range(len(A64.SETTINGS)))
def test_update_against_float64(S, si, K):
    got, _ = _run(S, si, K)
    t0 = A64.SETTINGS[si][4]
    names = [str(n) for n in A64.sizes()] + [f"{n}@{a}/{b}" for n, a, b in A64.VIEWS]
    for tag, t, g in zip(names, A64.case(si), got):
        r64, r32 = t["ref"][K, torch.float64], t["ref"][K, torch.float32]
        for k, name in enumerate(NAMES):
            held(f"setting {si} K {K} [{tag}] {name}", g[k], r64[k], r32[k])
        assert g[3] == t0 + K == r64[3], tag


# ------------------------------------------------------------------ 2. the same bits

@pytest.mark.parametrize("si", (0, 3))
def test_same_bits_in_two_runs_and_on_every_grouping(S, si):
    K = 5
    first, _ = _run(S, si, K)
    again, _ = _run(S, si, K)
    each, _ = _run(S, si, K, grouping="each")
    flat = _split_flat(_run(S, si, K, grouping="flat")[0], si)
    for i, a in enumerate(first):
        for other, what in ((again, "second run"), (each, "one optimiser per tensor"), (flat, "one flat tensor")):
            for k, name in enumerate(NAMES):
                assert torch.equal(a[k], other[i][k]), (what, i, name)
            assert a[3] == other[i][3], (what, i)


# ------------------------------------------------------------------ 3. gradients that are None

def test_parameters_without_gradient_are_skipped_and_the_plan_follows(S):
    beta1, beta2, lr = 0.5, 0.9, 2e-3
    gen = torch.Generator().manual_seed(31)
    sizes = [5, 70, 4097, 12, 300]
    p0 = [torch.randn(n, generator=gen) * 4 * lr for n in sizes]
    grads = [[torch.randn(n, generator=gen) for n in sizes] for _ in range(3)]
    has = [(True, False, True, False, True), (True, False, True, False, True), (True, True, False, False, True)]   # per step, per tensor
    params = [_dev(p) for p in p0]
    opt = S.Adam(params, lr=lr, betas=(beta1, beta2))
    ref = [dict(p=p.clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), t=0) for p in p0]
    for k in range(3):
        for p, g, h in zip(params, grads[k], has[k]):
            p.grad = g.to(DEV) if h else None
        before = [p.detach().clone() for p in params]
        opt.step()
        for i, h in enumerate(has[k]):
            if h:
                r = ref[i]
                r["p"], r["m"], r["v"], r["t"] = A64.run(r["p"], [grads[k][i]], r["m"], r["v"], r["t"], lr, beta1, beta2)
            else:
                assert torch.equal(params[i], before[i]), (k, i)          # its bits stay
    for i, p in enumerate(params):
        st = opt.state[p]
        if ref[i]["t"] == 0:                             # never had a gradient: no state, as in torch
            assert len(st) == 0 and torch.equal(p.cpu(), p0[i])
            continue
        assert float(st["step"]) == ref[i]["t"] == sum(h[i] for h in has), i
        plain = A64.run(p0[i], [grads[k][i] for k in range(3) if has[k][i]], torch.zeros_like(p0[i]), torch.zeros_like(p0[i]), 0, lr,
                        beta1, beta2, dtype=torch.float32)
        for k, (name, key) in enumerate(zip(NAMES, ("p", "m", "v"))):
            got = p.detach() if k == 0 else st[name]
            held(f"tensor {i} {name}", got.cpu(), ref[i][key], plain[k])


# ------------------------------------------------------------------ 4. the fused zeroing

def test_fused_zeroing_leaves_zeros_and_the_same_bits(S):
    for si in (0, 3):
        plain, g_plain = _run(S, si, 5)
        fused, g_fused = _run(S, si, 5, zero_grads=True)
        for i, (a, b) in enumerate(zip(plain, fused)):
            for k, name in enumerate(NAMES):
                assert torch.equal(a[k], b[k]), (si, i, name)
        assert all(bool((g == 0).all()) for g in g_fused)
        assert all(torch.equal(g, t["grads"][4]) for g, t in zip(g_plain, A64.case(si)))      # without the flag nothing writes a gradient


# ------------------------------------------------------------------ 5. the learning rate

@pytest.mark.parametrize("kind", ("number", "tensor"))
def test_learning_rate_changes_between_steps(S, kind):
    beta1, beta2 = 0.5, 0.9
    lrs = [2e-3, 2e-3, 5e-4, 1.25e-4]
    gen = torch.Generator().manual_seed(52)
    sizes = [3, 64, 4099, 777]
    p0 = [torch.randn(n, generator=gen) * 8e-3 for n in sizes]
    grads = [[torch.randn(n, generator=gen) for n in sizes] for _ in lrs]
    params = [_dev(p) for p in p0]
    lr_dev = torch.tensor([lrs[0]], device=DEV)
    opt = S.Adam(params, lr=lr_dev if kind == "tensor" else lrs[0], betas=(beta1, beta2))
    for k, lr in enumerate(lrs):
        if kind == "tensor":
            lr_dev.fill_(lr)
            assert opt.param_groups[0]["lr"] is lr_dev
        else:
            opt.param_groups[0]["lr"] = lr
        for p, g in zip(params, grads[k]):
            p.grad = g.to(DEV)
        opt.step()
    for i, p in enumerate(params):
        z = torch.zeros_like(p0[i])
        r64 = A64.run(p0[i], [g[i] for g in grads], z, z, 0, lrs, beta1, beta2)
        r32 = A64.run(p0[i], [g[i] for g in grads], z, z, 0, lrs, beta1, beta2, dtype=torch.float32)
        st = opt.state[p]
        for k, got in enumerate((p.detach(), st["exp_avg"], st["exp_avg_sq"])):
            held(f"lr as a {kind}, tensor {i} {NAMES[k]}", got.cpu(), r64[k], r32[k])
    # ... and a constant rate would miss it
    const = A64.run(p0[2], [g[2] for g in grads], torch.zeros_like(p0[2]), torch.zeros_like(p0[2]), 0, lrs[0], beta1, beta2)
    assert A64.E(const[0], A64.run(p0[2], [g[2] for g in grads], torch.zeros_like(p0[2]), torch.zeros_like(p0[2]), 0, lrs, beta1, beta2)[0]) > 1e-3


# ------------------------------------------------------------------ 6. interchange with torch.optim.Adam

@pytest.mark.parametrize("direction", ("torch_then_ours", "ours_then_torch"))
def test_state_dicts_continue_in_the_other_class(S, direction):
    K, beta1, beta2, lr = 3, 0.5, 0.9, 2e-3
    gen = torch.Generator().manual_seed(61)
    sizes = [1, 7, 64, 4100, (3, 5, 2)]
    shape = lambda n: n if isinstance(n, tuple) else (n,)                  # noqa: E731
    p0 = [torch.randn(*shape(n), generator=gen) * 4 * lr for n in sizes]
    grads = [[torch.randn(*shape(n), generator=gen) for n in sizes] for _ in range(2 * K)]
    params = [_dev(p) for p in p0]
    make = {"torch": lambda: torch.optim.Adam(params, lr=lr, betas=(beta1, beta2)), "ours": lambda: S.Adam(params, lr=lr, betas=(beta1, beta2))}
    a, b = direction.split("_then_")
    first = make[a]()
    for k in range(2 * K):
        if k == K:
            second = make[b]()
            second.load_state_dict(first.state_dict())
            first = second
        for p, g in zip(params, grads[k]):
            p.grad = g.to(DEV)
        first.step()
    for i, p in enumerate(params):
        z = torch.zeros_like(p0[i])
        r64 = A64.run(p0[i], [g[i] for g in grads], z, z, 0, lr, beta1, beta2)
        r32 = A64.run(p0[i], [g[i] for g in grads], z, z, 0, lr, beta1, beta2, dtype=torch.float32)
        st = first.state[p]
        for k, got in enumerate((p.detach(), st["exp_avg"], st["exp_avg_sq"])):
            held(f"{direction}, tensor {i} {NAMES[k]}", got.cpu(), r64[k], r32[k])
        assert float(st["step"]) == 2 * K == r64[3]


def test_training_optimizers_resume_from_a_reference_checkpoint(S):
    """The checkpoint keys of the reference: two torch.optim.Adam state dicts under optimizerG / optimizerD load, and the next step of
    both continues them."""
    lr_g, lr_d, K = 5e-4, 2e-3, 2
    gen = torch.Generator().manual_seed(62)
    p0 = {"G": [torch.randn(300, generator=gen) * 4 * lr_g, torch.randn(5, generator=gen) * 4 * lr_g], "D": [torch.randn(70, generator=gen) * 4 * lr_d]}
    grads = {w: [[torch.randn_like(p) for p in p0[w]] for _ in range(K + 1)] for w in "GD"}
    params = {w: [_dev(p) for p in p0[w]] for w in "GD"}
    ref = {"G": torch.optim.Adam(params["G"], lr=lr_g, betas=(0.0, 0.9)), "D": torch.optim.Adam(params["D"], lr=lr_d, betas=(0.0, 0.9))}

    def step(opts, k):
        for w in "GD":
            for p, g in zip(params[w], grads[w][k]):
                p.grad = g.to(DEV)
            opts[w].step()
    for k in range(K):
        step(ref, k)
    checkpoint = {"optimizerG": ref["G"].state_dict(), "optimizerD": ref["D"].state_dict(), "epoch": 3}
    ours = S.TrainingOptimizers(params["G"], params["D"], argparse.Namespace(beta1=0.0, beta2=0.9, lr_g=lr_g, lr_d=lr_d))
    ours.load_state_dict(checkpoint)
    step({"G": ours.optimizer_G, "D": ours.optimizer_D}, K)
    for w, lr, opt in (("G", lr_g, ours.optimizer_G), ("D", lr_d, ours.optimizer_D)):
        for i, p in enumerate(params[w]):
            z = torch.zeros_like(p0[w][i])
            gs = [g[i] for g in grads[w]]
            r64, r32 = A64.run(p0[w][i], gs, z, z, 0, lr, 0.0, 0.9), A64.run(p0[w][i], gs, z, z, 0, lr, 0.0, 0.9, dtype=torch.float32)
            held(f"resumed {w} {i} p", p.detach().cpu(), r64[0], r32[0])
            assert float(opt.state[p]["step"]) == K + 1
    assert sorted(ours.state_dict()) == ["optimizerD", "optimizerG"]


# ------------------------------------------------------------------ 7. the version-keyed weight caches see the step

def _stepped_layer(S, layer, x, g, lr):
    """forward, backward, one step of the new optimiser, forward: (y before, y after, the weights and biases after the step)."""
    y1 = layer(x)
    y1.backward(g)
    versions = layer.weight._version, layer.bias._version
    S.Adam(layer.parameters(), lr=lr, betas=(0.0, 0.9)).step()
    assert layer.weight._version > versions[0] and layer.bias._version > versions[1]
    y2 = layer(x)
    return y1.detach().cpu(), y2.detach().cpu(), layer.weight.detach().cpu(), layer.bias.detach().cpu()


def test_conv3x3_forward_after_a_step_uses_the_new_weights(S):
    N, cin, cout, H, W = 2, 40, 72, 33, 20
    gen = torch.Generator().manual_seed(71)
    r = lambda *s: torch.randn(*s, generator=gen)                          # noqa: E731
    x, w, b, g = r(N, cin, H, W), r(cout, cin, 3, 3) / (3.0 * cin ** 0.5), r(cout), r(N, cout, H, W)
    m = S.TrainableConv3x3(cin, cout).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w), m.bias.copy_(b)
    y1, y2, w2, b2 = _stepped_layer(S, m, x.to(DEV), g.to(DEV), lr=0.02)    # (a first Adam step moves every weight by lr: 40 % of their size)
    assert not torch.equal(w2, w)
    ref64, ref32 = C64.conv(x.double(), w2.double(), b2.double()), C64.conv(x, w2, b2)
    held("conv3x3 after the step", y2, ref64, ref32)
    stale = A64.E(y1, ref64)
    print(f"the forward with the weights of before the step: E {stale:.3e}")
    assert stale > 1000 * bound(A64.E(ref32, ref64))


def test_conv4x4_forward_after_a_step_uses_the_new_weights(S):
    N, cin, cout, H, W, s = 2, 24, 40, 17, 20, 2
    gen = torch.Generator().manual_seed(72)
    r = lambda *sh: torch.randn(*sh, generator=gen)                        # noqa: E731
    OH, OW = D64.out_size(H, s), D64.out_size(W, s)
    x, w, b, g = r(N, cin, H, W), r(cout, cin, 4, 4) / (4.0 * cin ** 0.5), r(cout), r(N, cout, OH, OW)
    m = S.adversarial._Conv4x4Layer(cin, cout, s, False).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w), m.bias.copy_(b)
    y1, y2, w2, b2 = _stepped_layer(S, m, x.to(DEV), g.to(DEV), lr=0.02)
    assert not torch.equal(w2, w)
    ref64, ref32 = D64.conv_forward(x.double(), w2.double(), b2.double(), s), D64.conv_forward(x, w2, b2, s)
    held("conv4x4 after the step", y2, ref64, ref32)
    assert A64.E(y1, ref64) > 1000 * bound(A64.E(ref32, ref64))


# ------------------------------------------------------------------ 8. no host synchronisation

def test_steps_do_not_synchronise_the_host(S):
    """Four steps on the tensors of item 1, the first one included (state and plan are made there), with a new learning rate, a gradient
    that appears and a gradient tensor that is replaced (two plan rebuilds) in between -- all with synchronisation made an error."""
    si = 0
    beta1, beta2, lr, _, _ = A64.SETTINGS[si]
    tensors = A64.case(si)
    poff, goff = _offsets()
    params = _placed([t["p0"] for t in tensors], poff)
    grads = [_placed([t["grads"][k] for t in tensors], goff) for k in range(3)]
    late = 9                                             # this tensor gets its first gradient in the second step
    opt = S.Adam(params, lr=lr, betas=(beta1, beta2))
    torch.cuda.synchronize()
    with _no_sync():
        for p, g in zip(params, grads[0]):
            p.grad = g
        params[late].grad = None
        opt.step()
        plan1 = opt._plans[0]["dev"]
        opt.param_groups[0]["lr"] = lr / 2
        params[late].grad = grads[1][late]              # a gradient appears: the plan follows
        opt.step()
        plan2 = opt._plans[0]["dev"]
        opt.step(zero_grads=True)                        # nothing changed: the same plan
        assert opt._plans[0]["dev"] is plan2 and plan2 is not plan1
        params[3].grad = grads[2][3]                     # a gradient tensor is replaced
        opt.param_groups[0]["lr"] = lr / 4
        opt.step()
        assert opt._plans[0]["dev"] is not plan2
    torch.cuda.synchronize()
    steps = [float(opt.state[p]["step"]) for p in params]
    assert steps == [3.0 if i == late else 4.0 for i in range(len(params))]
    assert all(bool(torch.isfinite(p).all()) for p in params)
