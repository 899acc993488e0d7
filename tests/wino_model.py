"""The Winograd fp32 convolution (csrc/conv_wino.hpp: conv3x3_wino_kernel, convs="fp32-winograd") WRITTEN OUT in plain torch, and the inputs the
CPU test (tests/test_wino_model.py) and the GPU tests (tests/test_gpu_conv_wino.py) share.

F(2x2, 3x3): a 2x2 output tile from a 4x4 input patch d (first row / column one above / left of the tile, zero padded),
    Y = A^T [ sum over input channels of (G g G^T) .* (B^T d B) ] A
  * U = G g G^T is formed in float64 and rounded ONCE to the working dtype (conv_wino_weights_kernel);
  * B^T d B with the kernel's signs -- rows d0 - d2, d1 + d2, d2 - d1, d1 - d3, then the same on the columns;
  * the elementwise products are summed over the input channels in the working dtype (the kernel: fp32 matrix instructions);
  * A^T m A: rows m0 + m1 + m2, m1 - m2 - m3, then the same on the columns;
  * odd sizes are zero-padded to whole tiles and cropped.
``conv`` computes in the dtype of ``x`` (float64: equal to the plain convolution; float32: the E_wino32 of the tests -- what an fp32 Winograd
costs next to a plain fp32 convolution, E_plain32).  E is the project's error measure (conv_train_f64.E): max|got - ref| / max|ref|, no floor.

The cases.  The kernel's workgroup covers 8 x 16 outputs, a dispatch slice is 8 blocks, a chunk 16 input channels, a group 64 output channels,
so the shapes are the smallest at which each of its paths is taken:
    H x W   1x1 | 8x16 one whole block | 9x17 four ragged blocks | 17x35 9 blocks: short last slice, odd W, scalar stores | 24x48 9 blocks, even W, pair stores
    Cin     3 | 16 | 24 two chunks, half of the second padding, blockable | 40 | 64 first count with c + 3 < nchunk | 72 | 256 | 272 17 chunks, raw ABI only
    Cout    5 | 8 | 64 | 72 second group mostly padding | 136 three groups
    N       1 | 3
Every value appears, every Cin meets a ragged grid (1x1, 9x17, 17x35) and an even one (8x16, 24x48):

     #   Cin  Cout   H x W    N   grid     blockable
     0     3     5    1x1     1   ragged   -
     1     3    64   24x48    3   even     out
     2    16     8    8x16    1   even     in out
     3    16    72   17x35    3   ragged   in out
     4    24   136    9x17    1   ragged   in out
     5    24     8   24x48    1   even     in out
     6    40    64   17x35    1   ragged   in out
     7    40    72    8x16    3   even     in out
     8    64   136   24x48    1   even     in out
     9    64     5    9x17    3   ragged   in
    10    72    72   17x35    1   ragged   in out
    11    72    64    8x16    1   even     in out
    12   256     8    9x17    1   ragged   in out
    13   256   136   24x48    1   even     in out
    14   272    72   17x35    1   ragged   in out     (raw ABI: nets.Conv routes Cin > 256 to the direct kernel)
    15   272   136   24x48    1   even     in out     (raw ABI)
"""
import math

import torch
import torch.nn.functional as F

import conv_train_f64 as cf

E = cf.E

# (Cin, Cout, H, W, N)
CASES = [(3, 5, 1, 1, 1), (3, 64, 24, 48, 3), (16, 8, 8, 16, 1), (16, 72, 17, 35, 3), (24, 136, 9, 17, 1), (24, 8, 24, 48, 1),
         (40, 64, 17, 35, 1), (40, 72, 8, 16, 3), (64, 136, 24, 48, 1), (64, 5, 9, 17, 3), (72, 72, 17, 35, 1), (72, 64, 8, 16, 1),
         (256, 8, 9, 17, 1), (256, 136, 24, 48, 1), (272, 72, 17, 35, 1), (272, 136, 24, 48, 1)]
CASE_IDS = [f"{c}to{o}at{h}x{w}n{n}" for c, o, h, w, n in CASES]
RAGGED, EVEN = ((1, 1), (9, 17), (17, 35)), ((8, 16), (24, 48))
WN_MAXCIN = 256                                      # csrc/conv_wino.hpp: the prologue table; nets.Conv routes wider layers to the direct kernel


# ------------------------------------------------------------------------------------------------------------------ the model

G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def weights(w, dtype):
    """U = G g G^T [Cout,Cin,4,4]: formed in float64, rounded once to ``dtype``."""
    g = torch.tensor(G, dtype=torch.float64)
    return torch.einsum("ij,ocjk,lk->ocil", g, w.double(), g).to(dtype)


def _bt(d0, d1, d2, d3):
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def _at(m0, m1, m2, m3):
    return m0 + m1 + m2, m1 - m2 - m3


def input_transform(x):
    """V = B^T d B of every 4x4 patch: [N,C,TY,TX,4,4] in the dtype of ``x`` (additions only)."""
    H, W = x.shape[-2:]
    d = F.pad(x, (1, 1 + W % 2, 1, 1 + H % 2)).unfold(2, 4, 2).unfold(3, 4, 2)           # [N,C,TY,TX,4 rows,4 columns]
    t = torch.stack(_bt(*d.unbind(4)), 4)                                                # B^T d: on the rows
    return torch.stack(_bt(*t.unbind(5)), 5)                                             # (B^T d) B: on the columns


def conv(x, w, b=None):
    """The 3x3 / stride 1 / zero-pad 1 convolution of ``x`` [N,Cin,H,W] with ``w`` [Cout,Cin,3,3] as F(2x2, 3x3), in the dtype of ``x``."""
    N, _, H, W = x.shape
    m = torch.einsum("ocij,nctxij->notxij", weights(w, x.dtype), input_transform(x))
    t = torch.stack(_at(*m.unbind(4)), 4)                                                # A^T m: [N,O,TY,TX,2,4]
    y = torch.stack(_at(*t.unbind(5)), 5)                                                # (A^T m) A: [N,O,TY,TX,2,2]
    out = y.permute(0, 1, 2, 4, 3, 5).reshape(N, w.shape[0], y.shape[2] * 2, y.shape[3] * 2)[..., :H, :W]
    return out if b is None else out + b.view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ shared inputs

def _gen(case, salt):
    cin, cout, h, w, n = case
    return torch.Generator().manual_seed(100000 * salt + 1000 * cin + 10 * cout + h + n)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_inputs(case):
    """Integer probes: x in [-8, 8], w = 4 * [-4, 4], bias in [-8, 8], residual in [-16, 16], prologue scale in {1/2, 1, 2}, shift in [-2, 2].
    Then every fp32 operation of the algorithm is exact: U = G g G^T is an integer of at most 36 (g a multiple of 4), V = B^T d B one of at most 32
    (72, in halves, behind the prologue), a sum over 272 channels stays below 272 * 36 * 32 = 313344, the nine terms of an output below 2.9e6 (behind
    the prologue: 256 * 36 * 72 * 9 = 6.0e6 in halves, i.e. 1.2e7 units) -- all under 2^24, in ANY order of summation."""
    cin, cout, h, w, n = case
    g = _gen(case, 1)
    return {"x": _ints(g, (n, cin, h, w), -8, 8), "w": 4.0 * _ints(g, (cout, cin, 3, 3), -4, 4), "bias": _ints(g, (cout,), -8, 8),
            "res": _ints(g, (n, cout, h, w), -16, 16), "sc": 2.0 ** _ints(g, (cin,), -1, 1), "sh": _ints(g, (cin,), -2, 2)}


VARIANTS = ("randn", "randn+100", "relu(randn)")


def dense_inputs(case, variant="randn"):
    """The accuracy inputs: x ~ N(0, 1) (``variant``: + 100, or ReLU'd), w ~ N(0, 1) / (3 sqrt(Cin)), bias and residual ~ N(0, 1), prologue
    scale in [0.5, 1.5), shift ~ 0.3 N(0, 1); seeded."""
    cin, cout, h, w, n = case
    g = _gen(case, 2 + VARIANTS.index(variant))
    x = torch.randn(n, cin, h, w, generator=g)
    x = x + 100.0 if variant == "randn+100" else torch.relu(x) if variant == "relu(randn)" else x
    return {"x": x, "w": torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * math.sqrt(cin)), "bias": torch.randn(cout, generator=g),
            "res": torch.randn(n, cout, h, w, generator=g), "sc": torch.rand(cin, generator=g) + 0.5, "sh": 0.3 * torch.randn(cin, generator=g)}


def prologue(x, sc, sh):
    """relu(x * scale - shift): the BN + ReLU in front of a convolution (nets.bn_relu_mask without a mask), in the dtype of ``x``."""
    return torch.relu(x * sc.to(x.dtype).view(1, -1, 1, 1) - sh.to(x.dtype).view(1, -1, 1, 1))


def modes(case):
    return ("plain", "bias+residual") + (("prologue",) if case[0] <= WN_MAXCIN else ())


def reference(d, mode, dtype, conv_fn):
    """The ``mode`` of the convolution (plain | bias+residual | prologue: all three operands behind the prologue) on the inputs ``d`` by
    ``conv_fn`` (cf.conv: the definition; conv: this model) in ``dtype``."""
    x, w = d["x"].to(dtype), d["w"].to(dtype)
    if mode == "plain":
        return conv_fn(x, w)
    if mode == "prologue":
        x = prologue(x, d["sc"], d["sh"])
    return conv_fn(x, w, d["bias"].to(dtype)) + d["res"].to(dtype)


def one_hot_pixels(h, w):
    """Named pixels of an h x w image at which a wrong halo, tile seam or transform sign shows: the corners, both sides of the block seams
    (x = 15 | 16, y = 7 | 8) and their crossing, the last (ragged) column and row."""
    named = {"corner 0,0": (0, 0), "corner 0,W-1": (0, w - 1), "corner H-1,0": (h - 1, 0), "corner H-1,W-1": (h - 1, w - 1),
             "x=15": (3, 15), "x=16": (3, 16), "y=7": (7, 5), "y=8": (8, 5), "y=7,x=15": (7, 15), "y=7,x=16": (7, 16), "y=8,x=15": (8, 15),
             "y=8,x=16": (8, 16), "last column": (5, w - 1), "last row": (h - 1, 20), "x=31": (4, 31), "x=32": (4, 32), "y=15": (15, 9),
             "y=16": (16, 9)}
    return {k: p for k, p in named.items() if 0 <= p[0] < h and 0 <= p[1] < w}


def one_hot_inputs(cin, cout, h, w, tap=None):
    """(x [P,cin,h,w]: image p has the value 3 at the p-th named pixel in channel p mod cin (7 mod cin for odd p: both halves of a chunk), zero
    elsewhere; weights 4 * integers, with ``tap`` = (ky, kx) non-zero at that tap only; the names)."""
    px = one_hot_pixels(h, w)
    x = torch.zeros(len(px), cin, h, w)
    for p, (y, xx) in enumerate(px.values()):
        x[p, (p if p % 2 == 0 else 7 + p) % cin, y, xx] = 3.0
    g = torch.Generator().manual_seed(77 + cin + h)
    wt = 4.0 * _ints(g, (cout, cin, 3, 3), -4, 4)
    wt[wt == 0] = 4.0                                  # (every tap of every channel answers)
    if tap is not None:
        keep = torch.zeros(3, 3)
        keep[tap] = 1.0
        wt = wt * keep
    return x, wt, list(px)


ONE_HOT_SHAPES = [(24, 8, 17, 35), (3, 5, 9, 17), (16, 72, 24, 48)]          # (Cin, Cout, H, W)
