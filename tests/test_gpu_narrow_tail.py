"""The narrow end without its widest tensor, kernel level (csrc/conv.hip: the tail phase of conv3x3_split_kernel, narrow_gather_kernel,
conv_tail_weights_kernel): a 128-channel block's second partial convolution followed by the next block's 128 -> 3 first convolution and 1x1
skip, against

  * a float64 definition of that chain (and the split-f16 model / a plain float32 run of it for the bound), and
  * the two-kernel path (slr_pconv3x3_forward -> slr_pconv3x3_forward_skipout).

Bound, for `a` (the activated input of the narrow block's second convolution) and `skip`: the project's E_gpu <= 2 E_model + 10 E_plain32
(tests/split_model.py; E = max|x - ref64| / max|ref64|).  The model runs BOTH convolutions of the chain in the split arithmetic, as the tail
does.  The update mask is bit-equal to the two-kernel path's.  Every test prints its figures (-s)."""
import functools

import pytest
import torch

import conv_train_f64 as cf
import split_model as sm
from metrics_fixture import from_blocked, to_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALES = (64.0, 1.0)
# (N, input channels of the wide convolution, H, W): one tile; seams in both directions and two samples; partial tiles in both directions;
# three chunks of input channels
SHAPES = [(1, 128, 8, 32), (2, 128, 16, 64), (1, 128, 17, 45), (1, 48, 8, 32)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def masks(N, H, W, holes):
    """[N,1,H,W]: all ones, or 10 % holes and one fully masked 5x5 patch (update mask 0 on its inner 3x3, ratio 0 there)."""
    if not holes:
        return torch.ones(N, 1, H, W)
    g = torch.Generator().manual_seed(17 * H + W)
    m = (torch.rand(N, 1, H, W, generator=g) > 0.1).float()
    m[:, :, 1:6, 3:8] = 0.0
    return m


@functools.lru_cache(maxsize=None)
def inputs(N, cin, H, W, holes):
    g = torch.Generator().manual_seed(1000 * cin + 10 * H + W)
    r = lambda *s: torch.randn(*s, generator=g)
    m = masks(N, H, W, holes)
    d = dict(m=m, xa=torch.relu(r(N, cin, H, W)) * m, res=r(N, 128, H, W), w6=r(128, cin, 3, 3) / (cin * 9) ** 0.5, b6=0.1 * r(128),
             mean1=0.2 * r(128), var1=0.5 + torch.rand(128, generator=g), waa=r(3, 128, 3, 3) / (128 * 9) ** 0.5, baa=0.1 * r(3),
             mean2=0.2 * r(3), var2=0.5 + torch.rand(3, generator=g), wb=r(3, 128, 1, 1) / 128 ** 0.5)
    return d


def modules(nets, d, cin):
    wide = nets.PartialConv(cin, 128, 3).cuda()
    nxt = nets.PconvResBlock(128, 3).cuda()
    with torch.no_grad():
        wide.weight.copy_(d["w6"]); wide.bias.copy_(d["b6"])
        nxt.conv_aa.weight.copy_(d["waa"]); nxt.conv_aa.bias.copy_(d["baa"]); nxt.conv_b.weight.copy_(d["wb"])
        nxt.bn1.stored_mean.copy_(d["mean1"]); nxt.bn1.stored_var.copy_(d["var1"])
        nxt.bn2.stored_mean.copy_(d["mean2"]); nxt.bn2.stored_var.copy_(d["var2"])
    return wide, nxt


def chain(d, tables, dtype, convs):
    """(a, update mask, skip, x6) of the chain in ``dtype``; ``convs`` = (wide 3x3, narrow 3x3, 1x1) on (input, weight)."""
    (sc1, sh1), (sc2, sh2) = tables
    t = lambda v: v.to(dtype)
    v4 = lambda v: t(v).view(1, -1, 1, 1)
    cin = d["xa"].shape[1]
    ratio, um, _ = cf.partial_factors(t(d["m"]), cin)
    o = (t(convs[0](d["xa"], d["w6"])) * ratio + v4(d["b6"])) * um + t(d["res"])
    act = torch.relu(o * v4(sc1) - v4(sh1)) * um
    ratio2, um2, _ = cf.partial_factors(um, 128)
    a = (t(convs[1](act, d["waa"])) * ratio2 + v4(d["baa"])) * um2
    a = torch.relu(a * v4(sc2) - v4(sh2)) * um2
    return a, um2, t(convs[2](o, d["wb"])), o


def references(d, tables, xscale):
    f64 = lambda k: (lambda x, w: sm.plain(x.double(), w.double(), k))
    f32 = lambda k: (lambda x, w: sm.plain(x.float(), w.float(), k))
    mdl = lambda k: (lambda x, w: sm.conv(x.float(), w, xscale, k))
    ref = chain(d, tables, torch.float64, (f64(3), f64(3), f64(1)))
    model = chain(d, tables, torch.float64, (mdl(3), mdl(3), mdl(1)))
    p32 = chain(d, tables, torch.float32, (f32(3), f32(3), f32(1)))
    return ref, model, p32


def run_both(nets, wide, nxt, d):
    """((a, um, skip) of the tail route, the same of the two-kernel path), host tensors."""
    xa, m, res = to_blocked(d["xa"]).cuda(), d["m"].cuda(), to_blocked(d["res"]).cuda()
    with torch.no_grad():
        tail = wide.forward_tail(xa, m, res, nxt)
        x6, um = wide(xa, m, residual=res, layout=nets.IN_B8 | nets.OUT_B8 | nets.RES_B8)
        two = nxt.conv_aa.forward_skipout(x6, um, nxt.conv_b, nxt.bn2.scale_shift(), nxt.bn1.scale_shift(), layout=nets.IN_B8)
    return [t.cpu() for t in tail], [t.cpu() for t in two]


@pytest.mark.parametrize("xscale", SCALES)
@pytest.mark.parametrize("holes", (False, True), ids=("ones", "holes"))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_tail_and_gather_against_float64_and_the_two_kernel_path(S, shape, holes, xscale):
    from slr_sfs_amd import nets
    N, cin, H, W = shape
    d = inputs(N, cin, H, W, holes)
    wide, nxt = modules(nets, d, cin)
    tables = [tuple(t.cpu() for t in bn.scale_shift()) for bn in (nxt.bn1, nxt.bn2)]
    nets.saturation_count(DEV)
    with nets.activation_scale(xscale):
        tail, two = run_both(nets, wide, nxt, d)
    assert nets.saturation_count(DEV) == 0
    ref, model, p32 = references(d, tables, xscale)
    assert torch.equal(tail[1], two[1]) and torch.equal(tail[1].double(), ref[1])
    if holes:
        assert bool((ref[1] == 0).any()) and bool((ref[1] == 1).any())
    worst = 0.0
    for name, k in (("a", 0), ("skip", 2)):
        e_gpu, e_two, e_model, e_plain = sm.E(tail[k], ref[k]), sm.E(two[k], ref[k]), sm.E(model[k], ref[k]), sm.E(p32[k], ref[k])
        bound = 2 * e_model + 10 * e_plain
        worst = max(worst, e_gpu / bound)
        print(f"narrow tail {N}x{cin}->128x{H}x{W} {'holes' if holes else 'ones'} xscale {xscale:g} {name}: E_gpu {e_gpu:.2e} two-kernel {e_two:.2e} "
              f"E_model {e_model:.2e} E_plain32 {e_plain:.2e} bound {bound:.2e} ratio {e_gpu / bound:.3f}")
        assert e_gpu <= bound, (name, e_gpu, bound)
        assert e_two <= bound, (name, e_two, bound)
    print(f"narrow tail {N}x{cin}->128x{H}x{W} {'holes' if holes else 'ones'} xscale {xscale:g}: worst ratio to the bound {worst:.3f}")


def raw_calls(S, nets, wide, d, tables, wtail, wscales, xscale):
    """The two entry points on prepared column weights, no next-BN behind the gather: (a, um, skip) device tensors."""
    lib = S._lib
    N, cin, H, W = d["xa"].shape
    xa, m, res = to_blocked(d["xa"]).cuda(), d["m"].cuda(), to_blocked(d["res"]).cuda()
    buf, wscale, _, _ = wide._split_weights()
    z, um = torch.empty(N, 32, H, W, device=DEV), torch.empty(N, 1, H, W, device=DEV)
    lib.call("slr_pconv3x3_forward_tail", xa.device, xa, m, buf, wscale, xscale, wide.bias, res, tables[0], tables[1], wtail, z, um, N, cin, 128, H, W)
    a, m2, skip = (torch.empty(N, c, H, W, device=DEV) for c in (3, 1, 3))
    zero = torch.zeros(3, device=DEV)
    lib.call("slr_narrow_gather", xa.device, z, um, zero, None, None, None, a, m2, skip, N, 128, H, W, wscales[0], wscales[1], xscale)
    return a, m2, skip, z


def test_one_hot_sweeps_find_every_k_slot_and_tap_offset(S):
    """For every input channel ci a column-weight set whose single non-zero is w_aa[ci % 3, ci, tap ci % 9] = 1, then the same for the skip
    (w_b[ci % 3, ci] = 1): the output channel ci % 3 is the activated channel ci shifted by the tap, times the partial ratio (the raw channel
    for the skip), within ONE split rounding -- 2^-22 relative (the lo half's 11 bits behind the hi half's 11), next to the fp32 rounding of
    the ratio product (2^-24) and, for halves that are f16 subnormals, 2^-25 / xscale absolute; every other output is exactly zero.  A
    wrong K permutation or tap offset moves a channel or a pixel."""
    from slr_sfs_amd import nets
    xscale = 64.0
    N, cin, H, W = SHAPES[0]
    d = inputs(N, cin, H, W, False)
    wide, nxt = modules(nets, d, cin)
    t1 = nxt.bn1.scale_shift()
    lib = S._lib
    with torch.no_grad(), nets.activation_scale(xscale):
        xa, m, res = to_blocked(d["xa"]).cuda(), d["m"].cuda(), to_blocked(d["res"]).cuda()
        x6, um = wide(xa, m, residual=res, layout=nets.IN_B8 | nets.OUT_B8 | nets.RES_B8)
        x6 = from_blocked(x6)
        act = torch.relu(x6 * t1[0].view(1, -1, 1, 1) - t1[1].view(1, -1, 1, 1)) * um          # the device's fp32 operations, in its order
        ratio = cf.partial_factors(um, 128)[0]
        wtail = torch.empty(lib.lib().slr_conv_tail_weight_bytes(128), dtype=torch.uint8, device=DEV)
        worst = torch.zeros(2, device=DEV)
        stray = torch.zeros((), device=DEV)
        nets.saturation_count(DEV)
        for branch in (0, 1):
            for ci in range(128):
                waa, wb = torch.zeros(3, 128, 3, 3, device=DEV), torch.zeros(3, 128, 1, 1, device=DEV)
                co, tap = ci % 3, ci % 9
                if branch == 0:
                    waa[co, ci, tap // 3, tap % 3] = 1.0
                else:
                    wb[co, ci, 0, 0] = 1.0
                lib.call("slr_conv_tail_weights", torch.device(DEV), waa, wb, wtail, 128, 4096.0, 4096.0)
                a, _, skip, _ = raw_calls(S, nets, wide, d, t1, wtail, (4096.0, 4096.0), xscale)
                if branch == 0:
                    expect = cf.shifted(act[:, ci:ci + 1], tap // 3 - 1, tap % 3 - 1) * ratio
                    got, other = a, skip
                    tol = expect.abs() * (2.0 ** -22 + 2.0 ** -24) + (2.0 ** -25 / xscale) * ratio
                else:
                    expect = x6[:, ci:ci + 1]
                    got, other = skip, a
                    tol = expect.abs() * 2.0 ** -22 + 2.0 ** -25 / xscale
                err = (got[:, co:co + 1] - expect).abs()
                worst[branch] = torch.maximum(worst[branch], (err / tol).max())
                rest = got.clone()
                rest[:, co] = 0.0
                stray += rest.abs().sum() + other.abs().sum()
    assert nets.saturation_count(DEV) == 0
    print(f"one-hot sweeps: worst error / (one split rounding): activated {float(worst[0]):.3f}, skip {float(worst[1]):.3f}; stray outputs {float(stray)}")
    assert float(stray) == 0.0
    assert float(worst[0]) <= 1.0 and float(worst[1]) <= 1.0


@pytest.mark.parametrize("xscale", SCALES)
def test_a_clamped_activated_value_is_counted(S, xscale):
    """One channel's BN scale lifts ONE pixel's activated value beyond 65472 / xscale while the raw value stays in range: the device counter
    moves; the in-range control leaves it at 0."""
    from slr_sfs_amd import nets
    N, cin, H, W = SHAPES[0]
    d = dict(inputs(N, cin, H, W, False))
    wide, nxt = modules(nets, d, cin)
    with torch.no_grad(), nets.activation_scale(xscale):
        xa, m, res = to_blocked(d["xa"]).cuda(), d["m"].cuda(), to_blocked(d["res"]).cuda()
        x6 = from_blocked(wide(xa, m, residual=res, layout=nets.IN_B8 | nets.OUT_B8 | nets.RES_B8)[0])
        ch = 77
        peak = float(x6[0, ch].max())
        assert 0.5 < peak < 100.0 and int((x6[0, ch] == peak).sum()) == 1
        limit = sm.F16_MAX_SPLIT / xscale
        for factor, counted in ((0.5, False), (2.0, True)):
            nxt.bn1.stored_mean.zero_()
            nxt.bn1.stored_var.fill_(1.0)
            nxt.bn1.stored_var[ch] = (peak / (factor * limit)) ** 2 - nxt.bn1.eps       # scale = factor * limit / peak
            second = float(x6[0, ch].flatten().topk(2).values[1]) * float(nxt.bn1.scale_shift()[0][ch])
            assert factor * limit * 0.99 < peak * float(nxt.bn1.scale_shift()[0][ch]) < factor * limit * 1.01
            nets.saturation_count(DEV)
            wide.forward_tail(xa, m, res, nxt)
            count = nets.saturation_count(DEV)
            print(f"saturation xscale {xscale:g}: activated peak {peak * float(nxt.bn1.scale_shift()[0][ch]):.1f} (next {second:.1f}) against {limit:g}: counter {count}")
            assert (count >= 1) if counted else (count == 0)
