"""The inference kernels (csrc/conv.hip, csrc/resample.hip, csrc/pconv.hip) with offsets past 2^31 bytes (B31), 2^32 bytes (B32) and 2^31
elements (E31 = 2^33 bytes): batches of many small samples wherever the sample is a grid coordinate, single big samples where the
boundary lies inside one sample.  Every call stays inside the limits of DESIGN.md ("Size limits of the entry points") with real tensors.

Per case: the input is torch.randn over the whole tensor (a read through a wrapped address sees other data), the output starts as NaN.
Bit-equality with the same entry point called on one sample alone holds the first sample (a wrapped write from the tail lands there), the
sample that holds each crossed boundary and the one after it, and the last sample; the first and last samples are also held to float64
with the bound of the kernel's small-shape test (tests/test_gpu_parity.py, test_gpu_conv_f32.py, test_gpu_conv_few.py).  A single big
sample is compared with float64 on three bands of 16 rows over the full width and all output channels.  Every test asserts which tensor
crosses which boundary and where its last sample (plane, channel group) starts, prints its figures (-s) and its peak device memory, and
leaves the device empty; profiles/large_offsets.txt is that output."""
import pytest
import torch
import torch.nn.functional as F

import split_model as sm
from metrics_fixture import from_blocked

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B31, B32, E31 = 1 << 29, 1 << 30, 1 << 31             # the three boundaries in fp32 elements
PEAK_BYTES = 48 << 30
IN_B8, OUT_B8, RES_B8, SKIP_B8, POOL_OUT, UP_OUT = 1, 2, 4, 32, 64, 128
BATCH = (206, 128, 250, 330)                          # 2.175 G elements (two samples start past E31); planes ragged against the 8 x 32 block, H W % 4 == 0
ELEMENTWISE = (500, 128, 150, 232)                    # 2.227 G elements, N C = 64 000 planes on grid.y; W % 4 == 0: the vector paths
NAN = float("nan")


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


@pytest.fixture(autouse=True)
def device_memory():
    """Peak device memory of the test under 48 GiB, and nothing left behind for the rest of the suite."""
    import slr_sfs_amd
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    slr_sfs_amd.nets.saturation_count(DEV)              # (one counter per device: start from a clean one)
    before = torch.cuda.memory_allocated()              # (what earlier modules of the suite still hold: their fixtures and caches)
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print(f"peak device memory {peak / 2 ** 30:.1f} GiB")
    assert peak < PEAK_BYTES, peak
    # the test's tensors are gone (the slack: workspaces the BLAS and convolution libraries behind the float64 references keep)
    assert torch.cuda.memory_allocated() <= before + (1 << 28), (before, torch.cuda.memory_allocated())


def call(S, name, *args):
    S._lib.call(name, DEV, *args)


def randn(*shape, scale=1.0):
    t = torch.randn(*shape, device=DEV)
    return t.mul_(scale) if scale != 1.0 else t


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def crossing(tag, t, *boundaries):
    """The samples of ``t`` [N, ...] to compare: the first, the last, and for each boundary (in elements) the sample that holds it and the
    next one.  Asserts that ``t`` crosses every boundary and that its last sample starts at or past it."""
    n, per = t.shape[0], t[0].numel()
    picks = {0, n - 1}
    for b in boundaries:
        assert t.numel() > b, (tag, t.numel(), b)
        assert (n - 1) * per >= b, f"{tag}: the last sample starts at element {(n - 1) * per}, below {b}"
        k = b // per
        assert k * per <= b < (k + 1) * per and k < n
        picks |= {k, min(k + 1, n - 1)}
    print(f"{tag}: {tuple(t.shape)} = {t.numel()} elements, last sample from element {(n - 1) * per}; samples {sorted(picks)}")
    return sorted(picks)


def alone(run, ins, outs, picks):
    """``run(n, ins, outs)`` on each sample of ``picks`` alone, into NaN-filled outputs of its own: bit-equal to the batch's.  Returns
    {sample: outputs} (equal to the batch's, so the float64 checks may use either)."""
    got = {}
    for k in picks:
        one_in = {a: None if t is None else t[k:k + 1] for a, t in ins.items()}
        one_out = {a: torch.full_like(t[k:k + 1], NAN) for a, t in outs.items()}
        run(1, one_in, one_out)
        for a, t in outs.items():
            assert not bool(torch.isnan(one_out[a]).any()), (a, k)
            assert torch.equal(t[k:k + 1], one_out[a]), f"sample {k}, output {a}: differs from the sample alone"
        got[k] = one_out
    return got


def no_nan(**outs):
    for a, t in outs.items():
        assert not bool(torch.isnan(t).any()), f"NaN left in {a}"


def close(tag, got, ref, rel, floor=1.0):
    """max|got - ref| <= rel * max(max|ref|, floor): the form of the small-shape tests (floor = None: an absolute bound)."""
    err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
    bound = rel if floor is None else rel * max(scale, floor)
    print(f"{tag}: max error {err:.3e} at scale {scale:.3e}, bound {bound:.3e}")
    assert err <= bound, (tag, err, bound)


def logical(t, b8):
    """The NCHW tensor a (channel-blocked) sample stands for."""
    return from_blocked(t) if b8 else t


def chan(v):
    return v.view(1, -1, 1, 1)


def partial_f(raw, mask, bias, cin):
    """(raw * ratio + b) * um of partialconv2d.py:61-74 in the dtype of ``raw`` -> (out, um)."""
    box = F.avg_pool2d(mask.to(raw.dtype), 3, stride=1, padding=1, divisor_override=1) * cin
    um = box.clamp(0, 1)
    ratio = (cin * 9) / (box + 1e-8) * um
    return (raw * ratio + chan(bias.to(raw.dtype))) * um, um


def bands(H):
    """Three bands of two block rows: the top, the middle, the bottom of an image of H rows."""
    mid = H // 2 // 8 * 8
    return [(0, 16), (mid - 8, mid + 8), (H - 16, H)]


def randomise(net):
    for m in net.modules():
        if hasattr(m, "stored_mean"):
            m.stored_mean.normal_(0, 0.3)
            m.stored_var.uniform_(0.5, 1.5)


# ------------------------------------------------------------------------------------------------------------------ 5. the memory-bound stages

@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("op", ["avgpool", "upsample"])
def test_resampling_batch_past_e31(S, op, b8):
    """slr_avgpool3x3s2: input past E31, output past B31.  slr_upsample_bilinear2x: input past B31, output past E31.  The plane is grid.y."""
    torch.manual_seed(51)
    N, C, H, W = ELEMENTWISE
    if op == "avgpool":
        x, out = randn(N, C, H, W), nans(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
        picks = set(crossing("avgpool in", x, B31, B32, E31)) | set(crossing("avgpool out", out, B31))
        name, ref = "slr_avgpool3x3s2", lambda t: F.avg_pool2d(t.double(), 3, stride=2, padding=1)
    else:
        H, W = H // 2, W // 2
        x, out = randn(N, C, H, W), nans(N, C, 2 * H, 2 * W)
        picks = set(crossing("upsample in", x, B31)) | set(crossing("upsample out", out, B31, B32, E31))
        name, ref = "slr_upsample_bilinear2x", lambda t: F.interpolate(t.double(), scale_factor=2, mode="bilinear", align_corners=False)

    def run(n, i, o):
        call(S, name, i["x"], o["out"], n, C, H, W, int(b8))
    run(N, {"x": x}, {"out": out})
    no_nan(out=out)
    one = alone(run, {"x": x}, {"out": out}, sorted(picks))
    for k in (0, N - 1):
        close(f"{op} sample {k}", logical(one[k]["out"], b8), ref(logical(x[k:k + 1], b8)), 2e-6, None)


@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
def test_conv1x1_small_batch_past_e31(S, b8):
    """slr_conv1x1_small 128 -> 3: the input is past E31, the sample is grid.y."""
    torch.manual_seed(52)
    N, C, H, W = ELEMENTWISE
    conv = S.nets.Conv(C, 3, 1).to(DEV)
    conv.bias.data.normal_()
    x, out = randn(N, C, H, W), nans(N, 3, H, W)
    picks = crossing("conv1x1_small in", x, B31, B32, E31)

    def run(n, i, o):
        call(S, "slr_conv1x1_small", i["x"], conv.weight, conv.bias, o["out"], n, C, 3, H, W, int(b8))
    run(N, {"x": x}, {"out": out})
    no_nan(out=out)
    one = alone(run, {"x": x}, {"out": out}, picks)
    for k in (0, N - 1):
        close(f"conv1x1_small sample {k}", one[k]["out"],
              F.conv2d(logical(x[k:k + 1], b8).double(), conv.weight.double(), conv.bias.double()), 5e-6, None)


@pytest.mark.parametrize("mode", ["plane", "channels", "nonzero", "none"])
def test_bn_relu_mask_batch_past_e31(S, mode):
    """slr_bn_relu_mask in its four mask modes: x, y (and the per-channel mask) past E31; (c, n) = grid (y, z), a plane in grid-stride steps."""
    torch.manual_seed(53)
    N, C, H, W = ELEMENTWISE
    x, y = randn(N, C, H, W), nans(N, C, H, W)
    x[:, :, 2:9, 3:40] = 0
    scale, shift = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
    mask = {"plane": lambda: (torch.rand(N, 1, H, W, device=DEV) > 0.3).float(),
            "channels": lambda: (torch.rand(N, C, H, W, device=DEV) > 0.3).float()}.get(mode, lambda: None)()
    mc = {"plane": 1, "channels": C, "nonzero": 0, "none": -1}[mode]
    picks = crossing("bn_relu_mask x", x, B31, B32, E31)
    if mode == "channels":
        crossing("bn_relu_mask mask", mask, E31)

    def run(n, i, o):
        call(S, "slr_bn_relu_mask", i["x"], scale, shift, i["mask"], mc, o["y"], n, C, H, W)
    run(N, {"x": x, "mask": mask}, {"y": y})
    no_nan(y=y)
    one = alone(run, {"x": x, "mask": mask}, {"y": y}, picks)
    for k in (0, N - 1):                                    # the torch composition of nets.bn_relu_mask, same order of operations: bit for bit
        xs = x[k:k + 1]
        ref = torch.relu(xs * chan(scale) - chan(shift))
        if mode != "none":
            ref = ref * ((xs != 0).float() if mask is None else mask[k:k + 1])
        assert torch.equal(one[k]["y"], ref), k


@pytest.mark.parametrize("epilogue", ["plain", "residual", "next_bn"])
def test_pconv_epilogue_batch_past_e31(S, epilogue):
    """slr_pconv_epilogue with each of its three epilogues: raw0, out (and the residual) past E31, the update mask written by channel 0."""
    torch.manual_seed(54)
    N, C, H, W = ELEMENTWISE
    raw, out, um = randn(N, C, H, W), nans(N, C, H, W), nans(N, 1, H, W)
    res = randn(N, C, H, W) if epilogue == "residual" else None
    bias, scale, shift = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
    nsc, nsh = (scale, shift) if epilogue == "next_bn" else (None, None)
    box = torch.randint(0, 10, (N, 1, H, W), device=DEV).float()
    picks = crossing("pconv_epilogue raw0", raw, B31, B32, E31)

    def run(n, i, o):
        call(S, "slr_pconv_epilogue", i["raw"], bias, i["box"], 3.0, i["res"], nsc, nsh, o["out"], o["um"], 27.0, n, C, H, W)
    ins = {"raw": raw, "box": box, "res": res}
    run(N, ins, {"out": out, "um": um})
    no_nan(out=out, um=um)
    one = alone(run, ins, {"out": out, "um": um}, picks)
    for k in (0, N - 1):                                    # the torch composition of nets.pconv_epilogue: bit for bit
        umr = box[k:k + 1] * 3.0
        umk = torch.clamp(umr, 0, 1)
        ref = (raw[k:k + 1] * (27.0 / (umr + 1e-8) * umk) + chan(bias)) * umk
        if res is not None:
            ref = ref + res[k:k + 1]
        if nsc is not None:
            ref = torch.relu(ref * chan(scale) - chan(shift)) * umk
        assert torch.equal(one[k]["out"], ref) and torch.equal(one[k]["um"], umk), k


# ------------------------------------------------------------------------------------------------------------------ 1. the 3x3 kernels

def conv_def(x, w, bias, pre, mask, res, nxt, dtype):
    """out (and the update mask) of the 3x3 entry points on the NCHW sample ``x`` in ``dtype``: prologue relu(x scale - shift) (* mask) in
    float32 as the kernel forms it, convolution, partial epilogue with an explicit mask plane, residual or next-BN."""
    t = x
    if pre is not None:
        t = torch.relu(x * chan(pre[0]) - chan(pre[1]))
        if mask is not None:
            t = t * mask
    raw = F.conv2d(t.to(dtype), w.to(dtype), None, padding=1)
    um = None
    if mask is None:
        o = raw + chan(bias.to(dtype))
    else:
        o, um = partial_f(raw, mask, bias, w.shape[1])
    if res is not None:
        o = o + res.to(dtype)
    if nxt is not None:
        o = torch.relu(o * chan(nxt[0].to(dtype)) - chan(nxt[1].to(dtype))) * um
    return o, um


CONV_VARIANTS = {       # partial, channel-blocked in / out / residual, prologue, residual, next-BN
    "plain-nchw": (False, False, False, False, False),
    "plain-b8-prologue-residual": (False, True, True, True, False),
    "pconv-b8-prologue-mask-nextbn": (True, True, True, False, True),
    "pconv-nchw-mask-residual": (True, False, False, True, False),
}


def conv3x3_case(S, shape, variant, rel, boundaries, rung=None):
    """One 3x3 call 128 -> 128 on ``shape``: samples alone bit for bit, first and last sample against float64."""
    nets = S.nets
    partial, b8, pro, with_res, with_next = CONV_VARIANTS[variant]
    N, C, H, W = shape
    conv = (nets.PartialConv if partial else nets.Conv)(C, C, 3).to(DEV)
    conv.bias.data.normal_()
    if rung is None:
        buf, wscale, xscale, arith = conv._split_weights()
    else:
        with nets.fp32_kernels(winograd=rung == "wino"):
            buf, wscale, xscale, arith = conv._split_weights()
        assert arith == 8 | (16 if rung == "wino" else 0)
    x = randn(N, C, H, W, scale=3.0)
    mask = (torch.rand(N, 1, H, W, device=DEV) > 0.3).float() if partial else None
    if partial and not pro:                               # without a prologue x is the already masked input
        x.mul_(mask)                                      # (per pixel: the same in either layout)
    pre = (torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)) if pro else None
    nxt = (torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.3) if with_next else None
    res = randn(N, C, H, W) if with_res else None
    out = nans(N, C, H, W)
    um = nans(N, 1, H, W) if partial else None
    layout = arith | (IN_B8 | OUT_B8 if b8 else 0) | (RES_B8 if b8 and with_res else 0)
    psc, psh = pre if pre else (None, None)
    nsc, nsh = nxt if nxt else (None, None)
    picks = set(crossing(f"{variant} in", x, *boundaries)) | set(crossing(f"{variant} out", out, *boundaries))

    def run(n, i, o):
        if partial:
            call(S, "slr_pconv3x3_forward", i["x"], psc, psh, i["mask"], buf, wscale, xscale, conv.bias, i["res"], nsc, nsh, o["out"], o["um"],
                 n, C, C, H, W, layout)
        else:
            call(S, "slr_conv3x3_forward", i["x"], buf, conv.bias, i["res"], o["out"], n, C, C, H, W, wscale, xscale, psc, psh, layout)
    ins = {"x": x, "mask": mask, "res": res}
    outs = {"out": out, "um": um} if partial else {"out": out}
    run(N, ins, outs)
    no_nan(**outs)
    one = alone(run, ins, outs, sorted(picks))
    assert nets.saturation_count(DEV) == 0
    for k in (0, N - 1):
        xs, rs = logical(x[k:k + 1], b8), None if res is None else logical(res[k:k + 1], b8)
        ms = None if mask is None else mask[k:k + 1]
        ref, um64 = conv_def(xs, conv.weight, conv.bias, pre, ms, rs, nxt, torch.float64)
        p32, _ = conv_def(xs, conv.weight, conv.bias, pre, ms, rs, nxt, torch.float32)
        print(f"{variant} sample {k}: E_gpu {sm.E(logical(one[k]['out'], b8), ref):.3e} E_plain32 {sm.E(p32, ref):.3e}")
        close(f"{variant} sample {k}", logical(one[k]["out"], b8), ref, rel)
        if partial:
            assert torch.equal(one[k]["um"].double(), um64)


@pytest.mark.parametrize("variant", list(CONV_VARIANTS))
def test_conv3x3_split_batch_past_e31(S, variant):
    """slr_conv3x3_forward / slr_pconv3x3_forward 128 -> 128 on the split-f16 rung: input, output (and residual) past E31; n = grid.z."""
    torch.manual_seed(11)
    conv3x3_case(S, BATCH, variant, 4e-6, (B31, B32, E31))


@pytest.mark.parametrize("rung,variant", [("f32", "plain-nchw"), ("f32", "pconv-b8-prologue-mask-nextbn"),
                                          ("wino", "plain-b8-prologue-residual"), ("wino", "pconv-nchw-mask-residual")])
def test_conv3x3_fp32_rungs_batch_past_b32(S, rung, variant):
    """The same entry points on the fp32 rung and the Winograd rung (nets.fp32_kernels(winograd=...)): input and output past B32."""
    torch.manual_seed(12)
    conv3x3_case(S, (104,) + BATCH[1:], variant, 4e-6, (B31, B32), rung)


@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("shape", [(1, 128, 2160, 3840), (1, 128, 4090, 4100)], ids=["4k", "near-limit"])
def test_conv3x3_single_big_sample(S, shape, b8):
    """slr_conv3x3_forward 128 -> 32 on ONE sample: a 4K frame (planes past B31) and one 0.05 % under the limit Cin H W < 2^31 (planes past
    B32; the int product of staging round 2).  Bands of 16 rows against float64, no NaN left anywhere."""
    torch.manual_seed(13)
    _, C, H, W = shape
    conv = S.nets.Conv(C, 32, 3).to(DEV)
    conv.bias.data.normal_()
    buf, wscale, xscale, arith = conv._split_weights()
    x, out = randn(1, C, H, W, scale=3.0), nans(1, 32, H, W)
    # the 4K frame is 4.25e9 bytes: its planes pass B31 (98.9 % of B32); the near-limit sample's pass B32 and stop 0.05 % under E31
    inside = B32 if shape[2] == 4090 else B31
    last = (C // 8 - 1) * 8 * H * W if b8 else (C - 1) * H * W
    print(f"single sample {shape}: {x.numel()} elements; the last {'channel group' if b8 else 'plane'} starts at element {last}, past {inside}")
    assert C * H * W < E31 and x.numel() > inside and last > inside
    if shape[2] == 4090:
        assert E31 - C * H * W < E31 // 1000
    call(S, "slr_conv3x3_forward", x, buf, conv.bias, None, out, 1, C, 32, H, W, wscale, xscale, None, None, arith | (IN_B8 if b8 else 0))
    no_nan(out=out)
    assert S.nets.saturation_count(DEV) == 0
    for r0, r1 in bands(H):
        lo, hi = max(r0 - 1, 0), min(r1 + 1, H)             # the band and its halo rows
        xb = x.view(1, C // 8, H, W, 8)[:, :, lo:hi].permute(0, 1, 4, 2, 3).reshape(1, C, hi - lo, W) if b8 else x[:, :, lo:hi]
        ref = F.conv2d(xb.double(), conv.weight.double(), conv.bias.double(), padding=1)[:, :, r0 - lo:r1 - lo]
        close(f"rows {r0}..{r1 - 1}", out[:, :, r0:r1], ref, 4e-6)


# ------------------------------------------------------------------------------------------------------------------ 2. fused skip branch, resampling epilogues

@pytest.mark.parametrize("kind,resample", [("plain", "Up"), ("pconv", "Down"), ("pconv", "Up"), ("plain", "Down")])
def test_fused_skip_and_resampling_epilogue(S, kind, resample):
    """slr_conv3x3_forward_skip / slr_pconv3x3_forward_skip 128 (+ 64 skip channels) -> 128 with SLR_CONV_UP_OUT (input past B32, the up-sampled
    output past E31) and SLR_CONV_POOL_OUT (input past E31); the side buffers of slr_conv_up_ws_bytes / slr_conv_pool_ws_bytes past B31.
    N * Cout / 8 = 65 440 grid rows of the second launch.  Against the sample alone, and float64 of convolution + skip + resampling."""
    torch.manual_seed(21)
    nets, L = S.nets, S._lib.lib()
    up = resample == "Up"
    N, C, CS, H, W = 4090, 128, 64, 9, 233 if up else 465
    OH, OW = (2 * H, 2 * W) if up else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    partial = kind == "pconv"
    conv = (nets.PartialConv if partial else nets.Conv)(C, C, 3).to(DEV)
    skip = nets.Conv(CS, C, 1, bias=not partial).to(DEV)
    conv.bias.data.normal_()
    if skip.bias is not None:
        skip.bias.data.normal_()
    buf, wscale, xscale, arith = conv._split_weights()
    sbuf, swscale, _, _ = skip._split_weights()
    x, xs = randn(N, C, H, W, scale=3.0), randn(N, CS, H, W)
    mask = (torch.rand(N, 1, H, W, device=DEV) > 0.3).float() if partial else None
    pre = None if partial else (torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV))
    if partial:
        x.view(N, C // 8, H, W, 8).mul_(mask.view(N, 1, H, W, 1))      # the activated, masked output of the block's first convolution
    ws_bytes = lambda n: (L.slr_conv_up_ws_bytes if up else L.slr_conv_pool_ws_bytes)(n, C, H, W)
    ws = torch.full((ws_bytes(N),), 255, dtype=torch.uint8, device=DEV)              # (0xffffffff: NaN)
    out, um = nans(N, C, OH, OW), nans(N, 1, H, W) if partial else None
    assert ws.numel() > 4 * B31, "side buffers past 2^31 bytes"
    picks = set(crossing("skip in", x, *((B31, B32) if up else (B31, B32, E31)))) | set(crossing("skip out", out, *((B31, B32, E31) if up else (B31,))))
    # the side buffers: the row lines of every sample, then the column lines of every sample; the sample whose lines straddle B31
    row_per, col_per = (C * ((H + 7) // 8) * W * (2 if up else 1), C * ((W + 31) // 32) * H * (2 if up else 1))
    assert N * (row_per + col_per) * 4 == ws.numel()
    at = B31 // row_per if N * row_per > B31 else (B31 - N * row_per) // col_per
    print(f"side buffers: {ws.numel()} bytes, {N * row_per} row and {N * col_per} column elements; B31 lies in the lines of sample {at}")
    picks |= {at, at + 1}
    layout = arith | IN_B8 | OUT_B8 | SKIP_B8 | (UP_OUT if up else POOL_OUT)

    def run(n, i, o):
        w = ws if n == N else torch.full((ws_bytes(n),), 255, dtype=torch.uint8, device=DEV)
        if partial:
            call(S, "slr_pconv3x3_forward_skip", i["x"], None, None, i["mask"], buf, wscale, xscale, conv.bias, o["out"], o["um"], n, C, C, H, W,
                 i["xs"], sbuf, CS, swscale, w, w.numel(), layout)
        else:
            call(S, "slr_conv3x3_forward_skip", i["x"], buf, conv.bias, o["out"], n, C, C, H, W, wscale, xscale, pre[0], pre[1],
                 i["xs"], sbuf, skip.bias, CS, swscale, w, w.numel(), layout)
    ins = {"x": x, "xs": xs, "mask": mask}
    outs = {"out": out, "um": um} if partial else {"out": out}
    run(N, ins, outs)
    no_nan(**outs)
    one = alone(run, ins, outs, sorted(picks))
    assert nets.saturation_count(DEV) == 0
    for k in (0, N - 1):
        a, um64 = conv_def(from_blocked(x[k:k + 1]), conv.weight, conv.bias, pre, mask[k:k + 1] if partial else None, None, None, torch.float64)
        a = a + F.conv2d(from_blocked(xs[k:k + 1]).double(), skip.weight.double(), None if skip.bias is None else skip.bias.double())
        ref = F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=False) if up else F.avg_pool2d(a, 3, stride=2, padding=1)
        close(f"{kind} {resample} sample {k}", from_blocked(one[k]["out"]), ref, 4e-6)
        if partial:
            assert torch.equal(one[k]["um"].double(), um64)


# ------------------------------------------------------------------------------------------------------------------ 3. the narrow end

@pytest.mark.parametrize("kind", ["plain", "pconv"])
def test_skipout_batch_past_e31(S, kind):
    """slr_conv3x3_forward_skipout / slr_pconv3x3_forward_skipout 128 -> 3 (csrc/conv_few.hpp) with the 1x1 skip of the same channel-blocked
    input, which is past E31."""
    torch.manual_seed(31)
    nets = S.nets
    N, C, H, W = BATCH
    partial = kind == "pconv"
    conv = (nets.PartialConv if partial else nets.Conv)(C, 3, 3).to(DEV)
    skip = nets.Conv(C, 3, 1, bias=not partial).to(DEV)
    conv.bias.data.normal_()
    if skip.bias is not None:
        skip.bias.data.normal_()
    buf, wscale, xscale, arith = conv._split_weights()
    x = randn(N, C, H, W)                                 # (unit scale: the skip's absolute bound is test_conv1x1_small's, for its inputs)
    mask = (torch.rand(N, 1, H, W, device=DEV) > 0.3).float() if partial else None
    pre = (torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV))
    nxt = (torch.rand(3, device=DEV) + 0.5, torch.randn(3, device=DEV) * 0.3) if partial else None
    out, sk = nans(N, 3, H, W), nans(N, 3, H, W)
    um = nans(N, 1, H, W) if partial else None
    picks = crossing(f"skipout {kind} in", x, B31, B32, E31)

    def run(n, i, o):
        if partial:
            call(S, "slr_pconv3x3_forward_skipout", i["x"], pre[0], pre[1], i["mask"], buf, wscale, xscale, conv.bias, None, nxt[0], nxt[1],
                 o["out"], o["um"], n, C, 3, H, W, skip._w4(), o["skip"], arith | IN_B8)
        else:
            call(S, "slr_conv3x3_forward_skipout", i["x"], buf, conv.bias, None, o["out"], n, C, 3, H, W, wscale, xscale, pre[0], pre[1],
                 skip._w4(), skip.bias, o["skip"], arith | IN_B8)
    ins = {"x": x, "mask": mask}
    outs = {"out": out, "skip": sk, "um": um} if partial else {"out": out, "skip": sk}
    run(N, ins, outs)
    no_nan(**outs)
    one = alone(run, ins, outs, picks)
    for k in (0, N - 1):
        xk = from_blocked(x[k:k + 1])
        ref, um64 = conv_def(xk, conv.weight, conv.bias, pre, mask[k:k + 1] if partial else None, None, nxt, torch.float64)
        close(f"skipout {kind} sample {k}", one[k]["out"], ref, 2e-6)
        close(f"skipout {kind} skip, sample {k}", one[k]["skip"],
              F.conv2d(xk.double(), skip.weight.double(), None if skip.bias is None else skip.bias.double()), 5e-6, None)
        if partial:
            assert torch.equal(one[k]["um"].double(), um64)


def test_tail_route_batch_past_e31(S):
    """slr_pconv3x3_forward_tail + slr_narrow_gather: the activated input and the residual past E31, Z [N,32,H,W] past B32.  Samples alone bit
    for bit; first and last sample against the two-kernel path of nets.staged_narrow_end() (slr_pconv3x3_forward ->
    slr_pconv3x3_forward_skipout) and float64 by the project's criterion E_tail <= 2 E_two_kernel + 10 E_plain32."""
    torch.manual_seed(32)
    nets = S.nets
    N, C, H, W = 410, 128, 250, 330
    blk, nxt = nets.PconvResBlock(C, C).to(DEV), nets.PconvResBlock(C, 3).to(DEV)
    randomise(blk), randomise(nxt)
    for cv in (blk.conv_ab, nxt.conv_aa):
        cv.bias.data.normal_()
    conv = blk.conv_ab
    buf, wscale, xscale, _ = conv._split_weights()
    tbuf, twscale, tswscale = nxt.conv_aa._tail_weights(nxt.conv_b)
    (tsc, tsh), (nsc, nsh) = nxt.bn1.scale_shift(), nxt.bn2.scale_shift()
    mask = (torch.rand(N, 1, H, W, device=DEV) > 0.3).float()
    a, res = randn(N, C, H, W), randn(N, C, H, W)
    a.view(N, C // 8, H, W, 8).abs_().mul_(mask.view(N, 1, H, W, 1))       # activated (>= 0) and masked, as the first convolution's next-BN leaves it
    z, um = nans(N, 32, H, W), nans(N, 1, H, W)
    out, um2, sk = nans(N, 3, H, W), nans(N, 1, H, W), nans(N, 3, H, W)
    picks = set(crossing("tail in", a, B31, B32, E31)) | set(crossing("tail Z", z, B31, B32))

    def run(n, i, o):
        call(S, "slr_pconv3x3_forward_tail", i["a"], i["mask"], buf, wscale, xscale, conv.bias, i["res"], tsc, tsh, tbuf, o["z"], o["um"],
             n, C, C, H, W)
        call(S, "slr_narrow_gather", o["z"], o["um"], nxt.conv_aa.bias, nsc, nsh, None, o["out"], o["um2"], o["skip"], n, C, H, W,
             twscale, tswscale, xscale)
    ins = {"a": a, "mask": mask, "res": res}
    outs = {"z": z, "um": um, "out": out, "um2": um2, "skip": sk}
    run(N, ins, outs)
    no_nan(**outs)
    assert float(z[:, 30:].abs().max()) == 0.0            # (planes 30 and 31 of Z are zero)
    one = alone(run, ins, outs, sorted(picks))
    assert nets.saturation_count(DEV) == 0

    def definition(k, dtype):
        av, rv, mv = from_blocked(a[k:k + 1]).to(dtype), from_blocked(res[k:k + 1]).to(dtype), mask[k:k + 1].to(dtype)
        o, m1 = partial_f(F.conv2d(av, conv.weight.to(dtype), None, padding=1), mv, conv.bias, C)
        o = o + rv
        t = torch.relu(o * chan(tsc.to(dtype)) - chan(tsh.to(dtype))) * m1
        y, m2 = partial_f(F.conv2d(t, nxt.conv_aa.weight.to(dtype), None, padding=1), m1, nxt.conv_aa.bias, C)
        y = torch.relu(y * chan(nsc.to(dtype)) - chan(nsh.to(dtype))) * m2
        return y, F.conv2d(o, nxt.conv_b.weight.to(dtype)), m2
    for k in (0, N - 1):
        with nets.staged_narrow_end():
            o2, m1 = conv(a[k:k + 1], mask[k:k + 1], residual=res[k:k + 1], layout=IN_B8 | OUT_B8 | RES_B8)
            y2, m2, s2 = nxt.conv_aa.forward_skipout(o2, m1, nxt.conv_b, (nsc, nsh), (tsc, tsh), layout=IN_B8)
        y64, s64, m64 = definition(k, torch.float64)
        y32, s32, _ = definition(k, torch.float32)
        assert torch.equal(one[k]["um"], m1) and torch.equal(one[k]["um2"], m2) and torch.equal(m2.double(), m64)
        for tag, got, two, p32, ref in (("out", one[k]["out"], y2, y32, y64), ("skip", one[k]["skip"], s2, s32, s64)):
            e_tail, e_two, e_plain = sm.E(got, ref), sm.E(two, ref), sm.E(p32, ref)
            print(f"tail sample {k} {tag}: E_tail {e_tail:.3e} E_two_kernel {e_two:.3e} E_plain32 {e_plain:.3e}")
            assert e_tail <= 2 * e_two + 10 * e_plain, (k, tag, e_tail, e_two, e_plain)


# ------------------------------------------------------------------------------------------------------------------ 4. slr_conv1x1_forward

@pytest.mark.parametrize("b8", [False, True], ids=["nchw", "b8"])
@pytest.mark.parametrize("rung", ["split", "f32"])
def test_conv1x1_batch_past_e31(S, rung, b8):
    """slr_conv1x1_forward 128 -> 72: the input past E31, the output past B32; n = grid.z, 128 pixels of a plane per workgroup."""
    torch.manual_seed(41)
    nets = S.nets
    N, C, H, W = BATCH
    CO = 72
    conv = nets.Conv(C, CO, 1).to(DEV)
    conv.bias.data.normal_()
    if rung == "split":
        buf, wscale, xscale, arith = conv._split_weights()
    else:
        with nets.fp32_kernels():
            buf, wscale, xscale, arith = conv._split_weights()
    x, out = randn(N, C, H, W, scale=3.0), nans(N, CO, H, W)
    picks = set(crossing("conv1x1 in", x, B31, B32, E31)) | set(crossing("conv1x1 out", out, B31, B32))
    layout = arith | (IN_B8 | OUT_B8 if b8 else 0)

    def run(n, i, o):
        call(S, "slr_conv1x1_forward", i["x"], buf, conv.bias, o["out"], n, C, CO, H, W, wscale, xscale, layout)
    run(N, {"x": x}, {"out": out})
    no_nan(out=out)
    one = alone(run, {"x": x}, {"out": out}, sorted(picks))
    assert nets.saturation_count(DEV) == 0
    for k in (0, N - 1):
        close(f"conv1x1 {rung} sample {k}", logical(one[k]["out"], b8),
              F.conv2d(logical(x[k:k + 1], b8).double(), conv.weight.double(), conv.bias.double()), 4e-6)


@pytest.mark.parametrize("rung", ["split", "f32"])
def test_conv1x1_single_sample_past_e31(S, rung):
    """slr_conv1x1_forward accepts one sample of more than 2^31 elements (Cin H W < 2^40): [1,264,2860,2860] -> 32 channels (the last plane starts past E31), on row bands."""
    torch.manual_seed(42)
    nets = S.nets
    C, H, W = 264, 2860, 2860
    conv = nets.Conv(C, 32, 1).to(DEV)
    conv.bias.data.normal_()
    if rung == "split":
        buf, wscale, xscale, arith = conv._split_weights()
    else:
        with nets.fp32_kernels():
            buf, wscale, xscale, arith = conv._split_weights()
    x, out = randn(1, C, H, W, scale=3.0), nans(1, 32, H, W)
    assert x.numel() > E31 and (C - 1) * H * W > E31
    print(f"conv1x1 single sample: {x.numel()} elements, the last plane starts at element {(C - 1) * H * W}")
    call(S, "slr_conv1x1_forward", x, buf, conv.bias, out, 1, C, 32, H, W, wscale, xscale, arith)
    no_nan(out=out)
    assert nets.saturation_count(DEV) == 0
    for r0, r1 in bands(H):
        close(f"rows {r0}..{r1 - 1}", out[:, :, r0:r1], F.conv2d(x[:, :, r0:r1].double(), conv.weight.double(), conv.bias.double()), 4e-6)


# ------------------------------------------------------------------------------------------------------------------ 6. the nets as a whole

@pytest.mark.parametrize("net", ["decoder", "encoder"])
def test_whole_nets_batch_past_e31(S, net):
    """DecoderPconv2(64, 3) on [1040,64,124,132] (its 128-channel full-resolution tensors hold 2.18 G elements) and EncoderWithZ on
    [2060,3,124,132] (its 64-channel ones 2.16 G) on the default rung.  Every kernel of either net has the sample (or the sample's planes) as
    a grid coordinate and no arithmetic that depends on it (csrc/conv.hip: blockIdx.z; csrc/resample.hip, the fix kernels: blockIdx.y), so
    the first sample, the samples around the boundary and the last one are bit-equal to their batch-of-one runs."""
    torch.manual_seed(61)
    nets = S.nets
    H, W = 124, 132
    with torch.no_grad():
        if net == "decoder":
            N, wide = 1040, 128
            model = nets.DecoderPconv2(64, 3).eval()
            randomise(model)
            model = model.to(DEV)
            x = randn(N, 64, H, W)
            x.mul_((torch.rand(N, 1, H, W, device=DEV) > 0.1).float())     # 10 % zero pixels: the derived mask of the first block
            run = lambda t: model(t, return_mask=True)
        else:
            N, wide = 2060, 64
            model = nets.EncoderWithZ(3, 64).eval()
            randomise(model)
            model = model.to(DEV)
            x = randn(N, 3, H, W)
            run = model
        per = wide * H * W
        assert N * per > E31 and (N - 1) * per >= E31
        k = E31 // per
        picks = sorted({0, k - 1, k, k + 1, N - 1})
        print(f"{net}: its [{N},{wide},{H},{W}] tensors hold {N * per} elements, the last sample from element {(N - 1) * per}; samples {picks}")
        nets.saturation_count(DEV)
        ys = run(x)
        for y in ys:
            assert not bool(torch.isnan(y).any())
        for s in picks:
            for y, y1 in zip(ys, run(x[s:s + 1].contiguous())):
                assert torch.equal(y[s:s + 1], y1), (net, s)
        assert nets.saturation_count(DEV) == 0
