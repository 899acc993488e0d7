"""Host-side checks of the narrow end's tail route (csrc/conv.hip, ABI 27), none of which needs a GPU: the layout of the column weights
against a numpy statement of it, and header, exports and ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("slr_conv_tail_weight_bytes", "slr_conv_tail_weight_source", "slr_conv_tail_weights", "slr_pconv3x3_forward_tail", "slr_narrow_gather")


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def layout(cin):
    """The column weights as the header states them: f16 [tile of 32 input channels][operand][chunk of 16][hi | lo][lane 64][8].  Lane l is
    row l % 32 of the 32 x 32 tile; its K slots 8 g + j (g = l // 32) of chunk c hold the channels a lane of half g has in accumulator
    registers 8 c + j of the wide kernel's D layout: register r is channel (r % 4) + 8 (r // 4) + 4 g of the wave's 32.
    -> int arrays (operand, half, row, ci) over the buffer."""
    shape = (cin // 32, 2, 2, 2, 64, 8)
    tile, operand, chunk, half, lane, j = np.indices(shape)
    r = 8 * chunk + j
    ci = 32 * tile + (r % 4) + 8 * (r // 4) + 4 * (lane // 32)
    return [a.reshape(-1) for a in (operand, half, lane % 32, ci)]


@pytest.mark.parametrize("cin", (128, 32))
def test_column_weight_layout(L, cin):
    n = L.slr_conv_tail_weight_bytes(cin) // 2
    assert n == cin // 32 * 4096
    want = layout(cin)
    got = np.zeros((4, n), dtype=np.int32)
    out = [ctypes.c_int() for _ in range(4)]
    for e in range(n):
        assert L.slr_conv_tail_weight_source(cin, e, *(ctypes.byref(o) for o in out)) == 0
        got[:, e] = [o.value for o in out]
    for name, g, w in zip(("operand", "half", "row", "ci"), got, want):
        assert np.array_equal(g, w), name
    # every (operand, half, row) meets every input channel exactly once: a B fragment's 16 K slots x the chunks x the tiles
    key = ((got[0] * 2 + got[1]) * 32 + got[2]) * cin + got[3]
    assert len(np.unique(key)) == n == 2 * 2 * 32 * cin


def test_sizes_and_argument_errors(L):
    assert L.slr_conv_tail_weight_bytes(128) == 4 * 2 * 2 * 2 * 64 * 16
    assert L.slr_conv_tail_weight_bytes(48) == 0 and L.slr_conv_tail_weight_bytes(0) == 0
    o = [ctypes.c_int() for _ in range(4)]
    assert L.slr_conv_tail_weight_source(128, 4 * 4096, *(ctypes.byref(v) for v in o)) == -1
    P = 0x10000                                                      # a 16-byte aligned non-null "pointer": nothing dereferences it on these paths
    assert L.slr_pconv3x3_forward_tail(P, P, P, 1.0, 64.0, P, P, P, P, P, P, P, 1, 128, 64, 8, 32, None) == -1 and b"128" in L.slr_last_error()
    assert L.slr_pconv3x3_forward_tail(P, None, P, 1.0, 64.0, P, P, P, P, P, P, P, 1, 128, 128, 8, 32, None) == -1 and b"null" in L.slr_last_error()
    assert L.slr_pconv3x3_forward_tail(P, P, P, 1.0, 64.0, P, P + 4, P, P, P, P, P, 1, 128, 128, 8, 32, None) == -1
    assert L.slr_narrow_gather(P, P, P, P, None, None, P, P, P, 1, 128, 8, 32, 1.0, 1.0, 64.0, None) == -1 and b"next_scale" in L.slr_last_error()
    assert L.slr_narrow_gather(P, P, P, None, None, None, P, P, P, 1, 128, 8, 32, 1.0, 1.0, 3.0, None) == -1 and b"xscale" in L.slr_last_error()
    assert L.slr_conv_tail_weights(P, P, P, 48, 1.0, 1.0, None) == -1


def test_header_exports_and_abi_agree(L):
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    protos = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, protos), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert _lib.ABI_VERSION >= 27 and L.slr_abi_version() == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION


def test_the_switch_and_the_route_conditions():
    """nets.staged_narrow_end() restores on exit, and the route is refused off the device without touching it."""
    import torch
    from slr_sfs_amd import nets
    assert nets._S.narrow_tail is True
    with nets.staged_narrow_end():
        assert nets._S.narrow_tail is False
    assert nets._S.narrow_tail is True
    dec = nets.DecoderPconv2(64, 3)
    x = torch.zeros(1, 128, 8, 32)
    assert dec.blocks[6].tail_route(dec.blocks[7], x, torch.ones(1, 1, 8, 32), True) is False      # a CPU tensor
