"""Digests of the split-f16 3x3 convolutions' outputs on seeded inputs (csrc/conv.hip: conv3x3_split_kernel), for bit-equality
between two builds of the library: the main loop of that kernel may be rescheduled, its arithmetic and the order of the products that
meet in an accumulator may not, so every output bit of every variant stays what it was.

``records(nets)`` runs the cases through the public entry points (nets.Conv / nets.PartialConv: conv, forward, forward_skip) and
returns {case id: sha256 of the launch's outputs}: the output tensor, the update mask of a partial convolution and the device's
saturation count behind the launch, in that order.  As a program it writes them as JSON:

    SLR_SFS_AMD_LIB=<library of the build that sets the expectation> python tests/conv_loop_bits.py tests/golden/conv_loop_bits.json

(a process of its own: the library is chosen when the package is imported).  tests/test_gpu_conv_loop_bits.py holds the current build
to the committed file, which was recorded with the library built from the csrc of the commit before the main loop was pipelined.

Cases -- the smallest at which the loop's software pipeline can go wrong:
  Cin 16 (one chunk: the fragment prefetch wraps at once), 32 (two chunks: both buffers, the last chunk re-staged), 144 (nine), 40 (a
  padded last chunk); grids [1,C,8,32] (one tile), [1,C,9,33] (four ragged tiles), [2,C,16,64]; Cout 32 / 64 / 128 (2 / 4 / 8 rows per
  wave: one batch per tap of 2 or 4 fragments, two batches of 4); NCHW and channel-blocked tensors; activation scale 64 and 1;
  plain convolution: prologue none / BN x epilogue bias / bias + residual;
  partial convolution: prologue none (explicit mask) / BN + mask / BN + derived mask (NCHW only) x epilogue plain / next-BN / residual;
  Cout 128, channel-blocked: forward_skip of both classes without resampling, with the pool and with the up-sampling epilogue.
Every input holds a few values beyond the split's range at scale 64 (|x| >= 1023), so the saturation count is not trivially zero."""
import hashlib
import json
import os
import sys

import torch

CINS = (16, 32, 144, 40)
GRIDS = ((1, 8, 32), (1, 9, 33), (2, 16, 64))
COUTS = (32, 64, 128)
SCALES = (64.0, 1.0)
DEV = "cuda:0"


def to_blocked(t):
    """[N,C,H,W] values in the channel-blocked memory layout [N,C/8,H,W,8], carried in a tensor of the logical shape."""
    n, c, h, w = t.shape
    return t.view(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().view(n, c, h, w)


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _inputs(cin, cout, grid, seed):
    """Seeded host tensors of one (Cin, Cout, grid): NCHW values; the blocked cases re-lay them."""
    n, h, w = grid
    g = torch.Generator().manual_seed(seed)
    t = {"x": _rand(g, n, cin, h, w, scale=2.0)}
    t["x"][:, ::3] *= (torch.rand(n, 1, h, w, generator=g) > 0.2)             # exact zeros: the derived mask has something to count
    t["x"][0, 0, 0, 0] = 1500.0                                                 # beyond the split's range at scale 64
    t["x"][n - 1, cin - 1, h - 1, w - 1] = -3000.0
    t["x"][0, cin // 2, h // 2, w // 2] = 1023.0
    t["mask"] = (torch.rand(n, 1, h, w, generator=g) > 0.25).float()
    t["res"] = _rand(g, n, cout, h, w)
    t["pre"] = (torch.rand(cin, generator=g) + 0.5, _rand(g, cin, scale=0.3))
    t["nxt"] = (torch.rand(cout, generator=g) + 0.5, _rand(g, cout, scale=0.3))
    t["w"] = _rand(g, cout, cin, 3, 3, scale=(9.0 * cin) ** -0.5)
    t["b"] = _rand(g, cout, scale=0.1)
    t["skip_x"] = _rand(g, n, 24, h, w)
    t["skip_w"] = _rand(g, cout, 24, 1, 1, scale=24.0 ** -0.5)
    t["skip_b"] = _rand(g, cout, scale=0.1)
    return t


def _digest(nets, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    h.update(int(nets.saturation_count(torch.device(DEV), reset=True)).to_bytes(8, "little"))
    return h.hexdigest()


def _module(cls, w, b, k=3):
    m = cls(w.shape[1], w.shape[0], k, bias=b is not None).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w)
        if b is not None:
            m.bias.copy_(b)
    return m


def records(nets):
    out = {}
    dev = lambda t: t.to(DEV).contiguous()
    nets.saturation_count(torch.device(DEV), reset=True)
    with torch.no_grad():
        for ic, cin in enumerate(CINS):
            for io, cout in enumerate(COUTS):
                for ig, grid in enumerate(GRIDS):
                    t = _inputs(cin, cout, grid, 1000 * ic + 100 * io + ig)
                    conv = _module(nets.Conv, t["w"], t["b"])
                    pconv = _module(nets.PartialConv, t["w"], t["b"])
                    pre, nxt, mask = tuple(map(dev, t["pre"])), tuple(map(dev, t["nxt"])), dev(t["mask"])
                    if cout == 128:
                        skip = _module(nets.Conv, t["skip_w"], t["skip_b"], 1)
                        pskip = _module(nets.Conv, t["skip_w"], None, 1)
                        skip_x = dev(to_blocked(t["skip_x"]))
                    for blocked in (False, True):
                        x, res = (dev(to_blocked(t[k]) if blocked else t[k]) for k in ("x", "res"))
                        lay = (nets.IN_B8 | nets.OUT_B8) if blocked else 0
                        rlay = lay | (nets.RES_B8 if blocked else 0)
                        for scale in SCALES:
                            key = f"cin{cin}/cout{cout}/{'x'.join(map(str, grid))}/{'b8' if blocked else 'nchw'}/s{int(scale)}"
                            with nets.activation_scale(scale):
                                for pname, p in (("none", None), ("bn", pre)):
                                    out[f"{key}/conv/{pname}/plain"] = _digest(nets, conv.conv(x, conv.bias, p, None, lay))
                                    out[f"{key}/conv/{pname}/res"] = _digest(nets, conv.conv(x, conv.bias, p, res, rlay))
                                pros = [("none", None, mask), ("bn_mask", pre, mask)] + ([] if blocked else [("bn_derived", pre, None)])
                                for pname, p, m in pros:
                                    out[f"{key}/pconv/{pname}/plain"] = _digest(nets, *pconv(x, m, pre_bn=p, layout=lay))
                                    out[f"{key}/pconv/{pname}/next_bn"] = _digest(nets, *pconv(x, m, next_bn=nxt, pre_bn=p, layout=lay))
                                    out[f"{key}/pconv/{pname}/res"] = _digest(nets, *pconv(x, m, residual=res, pre_bn=p, layout=rlay))
                                if cout == 128 and blocked:
                                    for fname, pool in (("skip", False), ("skip_pool", True), ("skip_up", "Up")):
                                        for pname, p in (("none", None), ("bn", pre)):
                                            out[f"{key}/conv/{pname}/{fname}"] = _digest(
                                                nets, conv.forward_skip(x, p, skip_x, skip, lay, skip_b8=True, pool=pool))
                                        out[f"{key}/pconv/none/{fname}"] = _digest(
                                            nets, *pconv.forward_skip(x, mask, skip_x, pskip, lay, skip_b8=True, pool=pool))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import slr_sfs_amd
    rec = records(slr_sfs_amd.nets)
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} digests from {slr_sfs_amd._lib.LIB_PATH} -> {sys.argv[1]}")
