"""The list-wide gradient to weight_orig on the device (slr_sfs_amd.spectral_weight_grad_multi, csrc/spectral.hip (d)) and the deferred
mode of ``SpectralGroup`` that uses it.

What is asked of the pair is BIT-equality with the per-tensor entry point (``spectral_weight_grad``) on every tensor, alone or inside a
list of 130, wherever the tensors lie and with the result written over dw; the per-tensor entry point is held to float64 in
tests/test_gpu_spectral.py, and the same float64 checks run here on the list form (criterion and ``held`` of that file: E_gpu <=
10 * E_plain32 + 1e-6, against the magnitude of the terms, with the case dW = W_eff in which dropping the rank-one term misses the bound).
Shapes: the sigma list's, plus the smallest at which the chunking can go wrong -- numel 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 CHUNK + 5,
one row, one column, [C, 20] linears; [128, 1152] and [256, 2304] are the banded sizes of the sigma list (>= 32768 elements).
The deferred mode: a network's gradients, u, v with it on are the bits of the network with it off.  Every test prints its figures (-s)."""
import functools

import pytest
import torch

import block_train_f64 as B64
import spectral_f64 as S64
from test_gpu_spectral import DEV, _at, _fill, _grad_case, _net, _net_case, _no_sync, _out, bound, held
from test_spectral_f64 import SIGMA_SHAPES

pytestmark = pytest.mark.gpu

CHUNK = 4096                                             # SLR_SPECTRAL_GRAD_CHUNK (asserted against the header below)
EDGE_SHAPES = ((1, 1), (65, 63), (64, 64), (17, 241), (19, 647), (1, 300), (300, 1), (256, 20))
SHAPES = tuple(SIGMA_SHAPES) + EDGE_SHAPES


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def test_the_shapes_are_the_edges_of_the_chunking():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slr_splat.h")).read()
    assert int(re.search(r"SLR_SPECTRAL_GRAD_CHUNK\s+(\d+)", hdr).group(1)) == CHUNK
    split = int(re.search(r"SLR_SPECTRAL_SPLIT_ELEMENTS\s+(\d+)", hdr).group(1))
    numels = [r * c for r, c in EDGE_SHAPES]
    assert numels[:5] == [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
    assert any(r * c >= split for r, c in SHAPES)


@functools.lru_cache(maxsize=None)
def _case(n, first=0):
    """n tensors cycling through SHAPES from SHAPES[first]: float32 dW, W, u, v (normalised normal vectors), 1 / sigma in [0.5, 1.5)."""
    out = []
    for i in range(n):
        r, c = SHAPES[(first + i) % len(SHAPES)]
        W, u, v = S64.matrix_case(r, c, 500 + first + i)
        gen = torch.Generator().manual_seed(900 + first + i)
        out.append(dict(W=W.float(), u=u.float(), v=v.float(), dW=torch.randn(r, c, generator=gen), inv=0.5 + torch.rand(1, generator=gen)))
    return out


def _place(case, k):
    """The list on the device: tensor i's dW and W lie 4 ((i + k) % 4) and 4 ((i + k + 1) % 4) bytes past a 16-byte boundary (k = None: all
    aligned); u and v packed into the saved arrays behind a pad of 1 / 3 elements, 1 / sigma in slot n - 1 - i of [n + 2]."""
    n = len(case)
    dws = [_at(c["dW"], 0 if k is None else (i + k) % 4) for i, c in enumerate(case)]
    ws = [_at(c["W"], 0 if k is None else (i + k + 1) % 4) for i, c in enumerate(case)]
    offs, uo, vo = [], 1, 3
    for c in case:
        offs.append((uo, vo))
        uo, vo = uo + c["u"].numel(), vo + c["v"].numel()
    su, sv, inv = torch.zeros(uo), torch.zeros(vo), torch.zeros(n + 2)
    slots = [n - 1 - i for i in range(n)]
    for c, (a, b), s in zip(case, offs, slots):
        su[a:a + c["u"].numel()], sv[b:b + c["v"].numel()], inv[s] = c["u"], c["v"], c["inv"]
    return dws, ws, su.to(DEV), sv.to(DEV), offs, inv.to(DEV), slots


def _single(S, case, placed):
    dws, ws, su, sv, offs, inv, slots = placed
    return [S.spectral_weight_grad(dw, w, su[a:a + w.shape[0]], sv[b:b + w.shape[1]], inv[s:s + 1]).cpu()
            for dw, w, (a, b), s in zip(dws, ws, offs, slots)]


def _multi(S, placed, inplace=False):
    dws, ws, su, sv, offs, inv, slots = placed
    torch.cuda.synchronize()
    with _no_sync():                                     # (the plan goes up from pinned memory: nothing waits)
        out = S.spectral_weight_grad_multi(dws, ws, su, sv, offs, inv, slots=slots, inplace=inplace)
    if inplace:
        assert all(o is d for o, d in zip(out, dws))
    return [o.cpu() for o in out]


@pytest.mark.parametrize("k", [None, 0, 1, 2, 3], ids=lambda k: "aligned" if k is None else f"off{k}")
def test_one_tensor_has_the_bits_of_the_per_tensor_entry(S, k):
    for first, shape in enumerate(SHAPES):
        case = _case(1, first)
        placed = _place(case, k)
        ref = _single(S, case, placed)
        got = _multi(S, placed)
        assert torch.equal(got[0], ref[0]), (shape, k)
        assert torch.equal(placed[0][0].cpu(), case[0]["dW"]), "dw is read only unless it is the output"
        assert torch.equal(_multi(S, placed, inplace=True)[0], ref[0]), (shape, k, "out is dw")
    print(f"{len(SHAPES)} shapes, one tensor each, offset {k}: bit-equal, also with out = dw")


def test_a_list_of_130_has_the_bits_of_the_per_tensor_entry(S):
    case = _case(130)
    placed = _place(case, 1)
    ref = _single(S, case, placed)
    a = _multi(S, placed)
    b = _multi(S, placed)
    for i, (x, y, r) in enumerate(zip(a, b, ref)):
        assert torch.equal(x, r), (i, tuple(r.shape))
        assert torch.equal(x, y), (i, "two calls, two results")
    aligned = _multi(S, _place(case, None))
    inplace = _multi(S, placed, inplace=True)
    for i, r in enumerate(ref):
        assert torch.equal(aligned[i], r) and torch.equal(inplace[i], r), (i, tuple(r.shape))
    # a tensor alone gives what it gives in the list (the seeds of _case(1, i) are the list's)
    for i in range(len(SHAPES)):
        alone = _multi(S, _place(_case(1, i), None))[0]
        assert torch.equal(alone, ref[i]), SHAPES[i]
    print("130 tensors: bit-equal per tensor, run to run, aligned or not, in place or not, alone or in the list")


def _f64_list(shapes, dW=None):
    cases = [_grad_case(r, c, seed=300 + r + c, dW=dW) for r, c in shapes]
    case = [dict(W=c["W"].float(), u=c["u"].float(), v=c["v"].float(), dW=c["dW"].float(), inv=c["inv"].float().reshape(1)) for c in cases]
    return cases, case


def test_the_list_against_float64(S):
    cases, case = _f64_list(SHAPES)
    got = _multi(S, _place(case, 2))
    for shape, c, g in zip(SHAPES, cases, got):
        held(f"d weight_orig {shape} (against its terms)", g, c["ref"], c["plain"], c["terms"])
        if shape != (1, 1):                              # ([1, 1]: u v^T = +-1 and the result is zero but for rounding -- only the terms measure it)
            held(f"d weight_orig {shape}", g, c["ref"], c["plain"])


def test_rank_one_term_is_not_lost_in_the_list(S):
    """dW = W_eff for every tensor of the list: <dW, W_eff> u v^T is as large as dW.  The pair holds the bound against the terms; the
    result without the term misses it by orders of magnitude."""
    shapes = ((65, 576), (64, 20), (19, 647))
    cases, case = _f64_list(shapes, dW=lambda W, inv: W * inv)
    got = _multi(S, _place(case, 3), inplace=True)
    for shape, c, g in zip(shapes, cases, got):
        e = held(f"d weight_orig {shape} with dW = W_eff", g, c["ref"], c["plain"], c["terms"])
        dropped = (c["dW"] * c["inv"]).float()
        e_drop = B64.E_terms(dropped, c["ref"], c["terms"])
        b = bound(B64.E_terms(c["plain"], c["ref"], c["terms"]))
        print(f"{shape} without the rank-one term: E {e_drop:.3e} = {e_drop / b:.0f} x the bound {b:.3e} (with it: {e:.3e})")
        assert e_drop > 1000 * b


def test_refusals_on_the_device(S):
    case = _case(2)
    dws, ws, su, sv, offs, inv, slots = _place(case, None)
    with pytest.raises(ValueError, match="outside the saved arrays"):
        S.spectral_weight_grad_multi(dws, ws, su, sv, [(su.numel(), 0), offs[1]], inv, slots=slots)
    with pytest.raises(ValueError, match="outside the saved arrays"):
        S.spectral_weight_grad_multi(dws, ws, su, sv, offs, inv, slots=[0, inv.numel()])
    with pytest.raises(ValueError, match="dw"):
        S.spectral_weight_grad_multi([dws[1], dws[0]], ws, su, sv, offs, inv, slots=slots)
    with pytest.raises(ValueError, match="not contiguous"):
        S.spectral_weight_grad_multi([dws[0].t().contiguous().t(), dws[1]], ws, su, sv, offs, inv, slots=slots)


# ------------------------------------------------------------------ the deferred mode of SpectralGroup

def _step(S, kind, deferred, twice=False, backwards=1):
    """One forward (``twice``: two, on x and on 0.5 x, before the backward) and the backward of a narrow network of
    tests/test_gpu_spectral.py; returns (outputs, {name: grad}, {name: buffer}, the network)."""
    c = _net_case(kind)
    net = _net(S, c)
    S.defer_weight_grad(net, deferred)
    noise = [tuple(t.to(DEV) for t in nz) for nz in c["noise"]]
    g = c["g"].to(DEV)
    from slr_sfs_amd import spectral
    calls, real_call = {}, spectral.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return real_call(name, *a)
    spectral.call = counting
    try:
        ys = _run(c, net, noise, g, twice, backwards)
    finally:
        spectral.call = real_call
    # the path that ran, not only its result: deferred, the list-wide pair once per forward and the per-tensor entry never; off, the
    # per-tensor entry for every normalised tensor of every forward and no plan of the list-wide one
    group = spectral.group_of(net)
    runs = backwards * (2 if twice else 1)
    multi, single = calls.get("slr_spectral_weight_grad_multi", 0), calls.get("slr_spectral_weight_grad", 0)
    assert (multi, single) == ((runs, 0) if deferred else (0, runs * len(group.leaves))), (deferred, multi, single)
    assert bool(group._grad_plans) == bool(deferred)
    grads = {n: (None if p.grad is None else p.grad.cpu()) for n, p in net.named_parameters()}
    return ys, grads, {n: b.cpu() for n, b in net.named_buffers()}, net


def _run(c, net, noise, g, twice, backwards):
    ys = []
    for _ in range(backwards):
        x = c["x"].to(DEV).requires_grad_(True)
        torch.cuda.synchronize()
        with _no_sync():
            y = _out(c, net(x, noise=noise))
            if twice:
                y = y + 2.0 * _out(c, net(x * 0.5, noise=noise))
            y.backward(g)
        ys += [y.detach().cpu(), x.grad.cpu()]
    return ys


def _same(a, b, what):
    assert a.keys() == b.keys()
    for n in a:
        assert (a[n] is None) == (b[n] is None), (what, n)
        if a[n] is not None:
            assert torch.equal(a[n], b[n]), (what, n)


@pytest.mark.parametrize("mode", ["once", "twice", "accumulate"])
@pytest.mark.parametrize("kind", ["decoder", "encoder"])
def test_deferred_gradient_has_the_bits_of_the_per_layer_path(S, kind, mode):
    """once: one forward, one backward.  twice: the network called twice before its backward -- each call's own u, v, 1 / sigma, the two
    contributions a two-term sum.  accumulate: two forward/backward pairs into the same .grad."""
    kw = dict(twice=mode == "twice", backwards=2 if mode == "accumulate" else 1)
    y0, g0, b0, _ = _step(S, kind, False, **kw)
    y1, g1, b1, net = _step(S, kind, True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(y0, y1))
    _same(g0, g1, "gradient")
    _same(b0, b1, "buffer")
    n_sn = sum(1 for n in g1 if n.endswith("weight_orig"))
    assert n_sn > 40 and all(g1[n] is not None for n in g1)
    print(f"{kind} {mode}: {len(g1)} gradients ({n_sn} through the normalisation) and {len(b1)} buffers bit-equal, deferred on and off")


def test_deferred_plan_is_uploaded_once_per_set_of_addresses(S, monkeypatch):
    from slr_sfs_amd import spectral
    c = _net_case("decoder")
    net = _net(S, c)
    S.defer_weight_grad(net)
    group = spectral.group_of(net)
    state = group.run()
    uploads = []
    real = spectral._grad_plan
    monkeypatch.setattr(spectral, "_grad_plan", lambda *a: uploads.append(len(a[0])) or real(*a))
    used = tuple(range(0, len(group.leaves), 2))
    ws = [group.leaves[i].weight_orig.detach() for i in used]
    raw = [torch.randn_like(w) for w in ws]
    ref = [spectral.spectral_weight_grad(d, w, state.saved_u[o[0]:o[0] + o[2]], state.saved_v[o[1]:o[1] + o[3]], state.inv_sigma[i:i + 1])
           for d, w, i, o in ((d, w, i, group.offsets[i]) for d, w, i in zip(raw, ws, used))]
    for _ in range(3):
        dws = [d.clone() for d in raw]
        for rnd in range(2):                             # the same tensors twice: one plan
            for d, r_ in zip(dws, raw):
                d.copy_(r_)
            group._weight_grads(state, used, dws, ws)
            assert all(torch.equal(d, r) for d, r in zip(dws, ref))
        del dws
    assert 1 <= len(uploads) <= 3 and all(n == len(used) for n in uploads)
    before = len(uploads)
    dws = [d.clone() for d in raw]
    group._weight_grads(state, used[:-1], dws[:-1], ws[:-1])                   # another set of leaves: another plan
    assert len(uploads) == before + 1 and uploads[-1] == len(used) - 1
    assert all(torch.equal(d, r) for d, r in zip(dws[:-1], ref[:-1]))
    assert len(group._grad_plans) <= group.GRAD_PLANS_MAX


def test_unused_leaf_gets_no_gradient_and_no_grad_mode_builds_nothing(S):
    from slr_sfs_amd import spectral

    class Pair(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = spectral.SpectralLinear(20, 24), spectral.SpectralLinear(20, 9)

    def run(deferred):
        torch.manual_seed(5)
        pair = Pair().to(DEV).train()
        S.defer_weight_grad(pair, deferred)
        x = torch.randn(3, 20, generator=torch.Generator().manual_seed(6)).to(DEV)
        spectral.begin(pair, force=True)
        y = pair.a(x)                                    # b is normalised with a (its u and v move) and never used
        y.square().sum().backward()
        with torch.no_grad():
            spectral.begin(pair, force=True)
            z = pair.a(x)
        assert not z.requires_grad
        return pair.a.weight_orig.grad.cpu(), pair.b.weight_orig.grad, pair.b.weight_u.cpu(), y.detach().cpu(), z.cpu()

    off, on = run(False), run(True)
    assert off[1] is None and on[1] is None
    for a, b in zip((off[0],) + off[2:], (on[0],) + on[2:]):
        assert torch.equal(a, b)
