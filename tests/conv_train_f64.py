"""The yardstick of the trainable 3x3 convolutions (slr_sfs_amd.trainable, csrc/conv_grad.hip): the forward and every gradient of the plain
and the partial 3x3 / stride 1 / zero-pad 1 convolution WRITTEN OUT as sums over the nine taps -- no autograd, no F.conv2d.  The functions
compute in the dtype of their arguments: float64 is the reference, the same code in float32 on the CPU is the "plain32" of the GPU
tests' criterion.  tests/test_conv_train_f64.py ties them to torch's float64 autograd.

Partial convolution (models/layers/partialconv2d.py:61-74, multi_channel with a channel-uniform mask [N,1,H,W], ``xm`` already masked):
    box = conv(mask, ones) = box3x3(mask) * Cin,  um = clamp(box, 0, 1),  ratio = 9 Cin / (box + 1e-8) * um,
    out = (conv(xm, w) * ratio + b) * um
so with the gradient g at out:  d raw = g * r, r = ratio * um;  dW = dW_plain(xm, g r);  db = sum g um;  dxm = dx_plain(g r, w)."""
import torch
import torch.nn.functional as F

TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def shifted(t, dy, dx):
    """s[..., y, x] = t[..., y + dy, x + dx], zero outside (dy, dx in -1 .. 1)."""
    H, W = t.shape[-2:]
    p = F.pad(t, (1, 1, 1, 1))
    return p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def conv(x, w, b=None):
    out = sum(torch.einsum("nchw,oc->nohw", shifted(x, ky - 1, kx - 1), w[:, :, ky, kx]) for ky, kx in TAPS)
    return out if b is None else out + b.view(1, -1, 1, 1)


def conv_dw(x, g):
    """dW[co][ci][ky][kx] = sum_{n,y,x} g[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]"""
    dw = x.new_zeros(g.shape[1], x.shape[1], 3, 3)
    for ky, kx in TAPS:
        dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, shifted(x, ky - 1, kx - 1))
    return dw


def conv_db(g):
    return g.sum((0, 2, 3))


def conv_dx(g, w):
    """dx[n,ci,y,x] = sum_{co,ky,kx} g[n,co,y-ky+1,x-kx+1] w[co,ci,ky,kx]"""
    return sum(torch.einsum("nohw,oc->nchw", shifted(g, 1 - ky, 1 - kx), w[:, :, ky, kx]) for ky, kx in TAPS)


def partial_factors(mask, cin):
    """(ratio, um, r = ratio * um), each [N,1,H,W]."""
    box = sum(shifted(mask, ky - 1, kx - 1) for ky, kx in TAPS) * cin
    um = box.clamp(0, 1)
    ratio = (9.0 * cin) / (box + 1e-8) * um
    return ratio, um, ratio * um


def pconv(xm, mask, w, b):
    """(out, update_mask)"""
    ratio, um, _ = partial_factors(mask, xm.shape[1])
    return (conv(xm, w) * ratio + b.view(1, -1, 1, 1)) * um, um


def pconv_grads(xm, mask, w, g):
    """(dxm, dW, db) for the gradient g at out."""
    _, um, r = partial_factors(mask, xm.shape[1])
    gr = g * r
    return conv_dx(gr, w), conv_dw(xm, gr), conv_db(g * um)


def E(got, ref):
    """The project's error measure: max|got - ref| / max|ref|, in float64."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max())


def holed_mask(N, H, W, seed):
    """[N,1,H,W] of 0 / 1: scattered holes and one block of holes wide enough that whole 3x3 windows are empty (update_mask has zeros)."""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(N, 1, H, W, generator=g) > 0.2).float()
    m[:, :, H // 3:H // 3 + 6, W // 4:W // 4 + 7] = 0.0
    m[:, :, 0, :3] = 0.0                                 # (and holes on the border)
    return m
