"""A plain torch definition of the summation splat and of what the models build on it -- TEST INFRASTRUCTURE ONLY (no tests here).

`oracle/slr_oracle.c` restates the reference's kernels in float32 and in their order: the yardstick for bit-exactness, but it cannot
differentiate a composition, and it cannot show that a float32 result is within float32 rounding of the true value.  The functions
below are written with `scatter_add`, run in any dtype (float64 by default) and are differentiated by torch autograd; called with
`dtype=torch.float32` they are "the plain definition in float32", the yardstick the tolerances of tests/test_gpu_gradients.py use.

The position rule that makes the dtypes comparable: the position every implementation floors is the float32 sum X32 = fl32(x + flow)
(models/softsplat.py:169-170).  Here the position X has exactly the value of X32 and dX/dflow = 1, and `floor` is taken from X32 -- the
only discontinuity of the splat, which would otherwise make float64 and float32 disagree by O(1) next to integer positions, is decided
once for all dtypes.  A pixel whose X32 or Y32 is not representable (non-finite, or |.| >= 2^30: no image reaches that far) is dropped,
as by the kernels and the oracle; its gradients are exactly 0.
"""
import numpy as np
import torch


def _grid(N, H, W):
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return gx.expand(N, H, W), gy.expand(N, H, W)


def splat_sum(x, flow, dtype=torch.float64):
    """out[n,c,Y,X] = sum over sources and their four corners of x * bilinear weight (models/softsplat.py:157-202), [N,C,H,W];
    differentiable in `x` and `flow`."""
    N, C, H, W = x.shape
    assert flow.shape == (N, 2, H, W)
    gx, gy = _grid(N, H, W)
    f32 = flow.detach().to(torch.float32)
    ok = ((gx + f32[:, 0]).abs() < 2.0 ** 30) & ((gy + f32[:, 1]).abs() < 2.0 ** 30)      # (False for NaN / inf)
    # a dropped pixel's flow is replaced by 0 BEFORE any arithmetic: autograd would turn the unselected branch of a later `where`
    # into NaN * 0
    fl = torch.where(ok[:, None], flow.to(dtype), torch.zeros((), dtype=dtype))
    f32 = torch.where(ok[:, None], f32, torch.zeros((), dtype=torch.float32))
    X32, Y32 = gx + f32[:, 0], gy + f32[:, 1]
    x0, y0 = torch.floor(X32), torch.floor(Y32)
    # value: exactly X32 (fl - fl.detach() is an exact zero in every dtype); derivative w.r.t. the flow: 1
    X = X32.to(dtype) + (fl[:, 0] - fl[:, 0].detach())
    Y = Y32.to(dtype) + (fl[:, 1] - fl[:, 1].detach())
    x0d, y0d = x0.to(dtype), y0.to(dtype)
    ax, bx, ay, by = (x0d + 1) - X, X - x0d, (y0d + 1) - Y, Y - y0d
    xi, yi = x0.to(torch.int64), y0.to(torch.int64)
    v = x.to(dtype).reshape(N, C, H * W)
    out = torch.zeros(N, C, H * W, dtype=dtype)
    for (cx, cy, w) in ((xi, yi, ax * ay), (xi + 1, yi, bx * ay), (xi, yi + 1, ax * by), (xi + 1, yi + 1, bx * by)):   # NW, NE, SW, SE
        inside = ok & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        idx = torch.where(inside, cy * W + cx, torch.zeros((), dtype=torch.int64)).reshape(N, 1, H * W).expand(N, C, H * W)
        wm = torch.where(inside, w, torch.zeros((), dtype=dtype)).reshape(N, 1, H * W)
        out = out.scatter_add(2, idx, v * wm)
    return out.reshape(N, C, H, W)


def function_softsplat(x, flow, metric, mode, dtype=torch.float64, return_norm=False):
    """FunctionSoftsplat, models/softsplat.py:665-690: one summation splat of [x * w, w], w = 1 (average) | metric (linear) |
    exp(metric) (softmax), divided by the splatted w where that is not exactly zero (:684).  `return_norm`: also the normaliser
    as splatted (before zeros are replaced by 1; None for summation)."""
    assert mode in ("summation", "average", "linear", "softmax")
    x = x.to(dtype)
    if mode == "summation":
        out = splat_sum(x, flow, dtype)
        return (out, None) if return_norm else out
    if mode == "average":
        w = torch.ones(x.shape[0], 1, x.shape[2], x.shape[3], dtype=dtype)
        stacked = torch.cat([x, w], 1)
    else:
        w = metric.to(dtype).exp() if mode == "softmax" else metric.to(dtype)
        stacked = torch.cat([x * w, w], 1)
    s = splat_sum(stacked, flow, dtype)
    norm = s[:, -1:]
    out = s[:, :-1] / torch.where(norm == 0.0, torch.ones((), dtype=dtype), norm)
    return (out, norm) if return_norm else out


def training_step(fs, Z, flow_f, flow_p, alpha, dtype=torch.float64, clamp_z=(-20.0, 20.0), return_norm=False):
    """The splat half of the training step, models/animating_softmax_splating.py:601-606, 628, 651, 672, 676-678, 691-692 (what
    oracle.synth_baseline restates for forward_flow): Zn = clamp(Z - Z.max()), both directions splat [fs e a, e a] with e = exp(Zn),
    a = alpha / 1 - alpha, the sums of the two are divided, the normaliser clamped at 1e-8.  The displacement fields are inputs.
    fs [B,C,H,W], Z [B,1,H,W], flow_* [B,2,H,W], alpha [B,1,1,1] -> [B,C,H,W]."""
    fs, Z, alpha = fs.to(dtype), Z.to(dtype), alpha.to(dtype)
    Zn = Z - Z.max()
    if clamp_z is not None:
        Zn = torch.clamp(Zn, min=clamp_z[0], max=clamp_z[1])
    e = Zn.exp()
    Sf = splat_sum(torch.cat([fs * e * alpha, e * alpha], 1), flow_f, dtype)
    Sp = splat_sum(torch.cat([fs * e * (1 - alpha), e * (1 - alpha)], 1), flow_p, dtype)
    norm = Sf[:, -1:] + Sp[:, -1:]
    out = (Sf[:, :-1] + Sp[:, :-1]) / torch.clamp(norm, min=1e-8)
    return (out, norm) if return_norm else out


# ---- which path of csrc/grad.hip's grad_tile_kernel a block of source pixels takes ----------------------------------------------
TILE_H, TILE_W, STRIPS, BOX, THREADS, BENT = 8, 64, 2, 4096, 512, 2
CLASSES = ("straight", "staged1", "staged2", "staged3", "staged4", "staged6", "staged8", "bent_no_fit", "empty")


def backward_block_classes(flow):
    """The block rule of csrc/grad.hip (grad_tile_kernel: destination boxes per strip, `bent`, `staged`, the count of box cells per
    work-item) restated in numpy: flow [N,2,H,W] -> int array [N, tiles_y, tiles_x] of indices into CLASSES.  `straight`: a wave's
    destinations stay on two rows (direct gathers); `stagedK`: the boxes fit the LDS and a work-item carries K of their cells;
    `bent_no_fit`: rows bend, boxes do not fit (direct gathers, corner pairs); `empty`: nothing of the block lands in the image."""
    flow = np.asarray(flow, dtype=np.float32)
    N, _, H, W = flow.shape
    ty, tx = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    out = np.empty((N, ty, tx), np.int64)
    big = 0x7fffffff
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            X, Y = xx + flow[n, 0], yy + flow[n, 1]
            ok = (np.abs(X) < 2.0 ** 30) & (np.abs(Y) < 2.0 ** 30)
            x0 = np.where(ok, np.floor(np.where(ok, X, 0)), 0).astype(np.int64)
            y0 = np.where(ok, np.floor(np.where(ok, Y, 0)), 0).astype(np.int64)
            inx0, inx1, iny0, iny1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W), (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
            anyc = ok & (inx0 | inx1) & (iny0 | iny1)
            bx0, bx1 = np.where(anyc, np.maximum(x0, 0), big), np.where(anyc, np.minimum(x0 + 1, W - 1), -1)
            by0, by1 = np.where(anyc, np.maximum(y0, 0), big), np.where(anyc, np.minimum(y0 + 1, H - 1), -1)
            for j in range(ty):
                for i in range(tx):
                    rs, cs = slice(j * TILE_H, min(H, (j + 1) * TILE_H)), slice(i * TILE_W, min(W, (i + 1) * TILE_W))
                    a = anyc[rs, cs]
                    # rows of gradOutput one wave's destinations spread over (a wave without a destination: negative)
                    bent = max(0, max(int(by1[r, cs].max()) - int(by0[r, cs].min()) + 1 for r in range(rs.start, rs.stop)))
                    fits, some, nbox = True, False, 0
                    for q in range(STRIPS):
                        qs = slice(i * TILE_W + q * (TILE_W // STRIPS), min(W, i * TILE_W + (q + 1) * (TILE_W // STRIPS)))
                        if qs.start >= qs.stop:
                            continue
                        w_ = int(bx1[rs, qs].max()) - int(bx0[rs, qs].min()) + 1
                        h_ = int(by1[rs, qs].max()) - int(by0[rs, qs].min()) + 1
                        has = w_ > 0 and h_ > 0
                        cells = w_ * h_ if has else 0
                        fits = fits and cells <= BOX
                        nbox += cells if cells <= BOX else 0
                        some = some or has
                    assert some == bool(a.any())
                    if some and fits and nbox <= BOX and bent > BENT:
                        need = (nbox + THREADS - 1) // THREADS
                        cls = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 5}.get(max(need, 1), 6)
                    elif bent > BENT:
                        cls = 7
                    else:
                        cls = 0 if some else 8
                    out[n, j, i] = cls
    return out


def backward_block_paths(flow):
    """Blocks per class of `backward_block_classes`, a dict over CLASSES: so that a test can assert that its flow reaches the paths
    it claims to."""
    cls = backward_block_classes(flow)
    return {name: int((cls == k).sum()) for k, name in enumerate(CLASSES)}
