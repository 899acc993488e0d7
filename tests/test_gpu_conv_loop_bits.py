"""Every output bit of the split-f16 3x3 convolutions equals what the kernel gave before its main loop was software-pipelined
(csrc/conv.hip: conv3x3_split_kernel -- B fragments requested one batch ahead, prologue constants two values ahead).  The loop keeps,
per accumulator, the order of the products (per chunk and tap: w_lo x_hi, w_hi x_lo, w_hi x_hi) and the staged values their arithmetic,
so nothing may move: tests/golden/conv_loop_bits.json holds sha256 digests of (output, update mask, saturation count) recorded by
tests/conv_loop_bits.py with the library of the commit before the change; the cases and why they are these are listed there."""
import json
import os

import pytest
import torch

import conv_loop_bits as clb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def digests():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return clb.records(slr_sfs_amd.nets)


@pytest.fixture(scope="module")
def expected(golden_dir):
    with open(os.path.join(golden_dir, "conv_loop_bits.json")) as f:
        return json.load(f)


def test_same_cases_as_recorded(digests, expected):
    assert sorted(digests) == sorted(expected)
    assert len(expected) == 1872             # 72 (Cin, Cout, grid, scale) x (NCHW 13 + blocked 10) + 24 (Cin, grid, scale) x 9 skip forms at Cout 128


@pytest.mark.parametrize("cin", clb.CINS)
@pytest.mark.parametrize("cout", clb.COUTS)
def test_outputs_bit_identical_to_the_loop_before(digests, expected, cin, cout):
    keys = [k for k in expected if k.startswith(f"cin{cin}/cout{cout}/")]
    assert keys
    bad = [k for k in keys if digests.get(k) != expected[k]]
    assert not bad, f"{len(bad)} of {len(keys)} launches differ from the recorded bits, e.g. {bad[:8]}"
