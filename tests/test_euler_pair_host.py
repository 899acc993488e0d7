"""Host-side checks of the two-direction Euler operator (csrc/euler.hip, ABI 28), none of which needs a GPU: the entry points and their
binding, the documented workspace size, and every refusal -- each of which must come back before anything is launched (the pointers
handed over here are not device memory: a launch on them could not go unnoticed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("slr_euler_pair_forward", "slr_euler_pair_workspace_bytes", "slr_euler_pair_backward")
FAKE = ctypes.c_void_p(1 << 20)                       # non-null, 8-byte aligned, never dereferenced by a refused call


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def workspace_bytes(B, H, W):
    """include/slr_splat.h: per sample 1280 bytes of header and partial maxima, an int64 and a class word per element of grad_motion."""
    return B * (1280 + 24 * H * W)


def test_abi_28_and_the_binding_table(L):
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    assert int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == L.slr_abi_version()
    assert _lib.ABI_VERSION >= 28
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert _lib.SIGNATURES["slr_euler_pair_forward"] == (i, [vp] * 3 + [i] * 3 + [vp] * 5)
    assert _lib.SIGNATURES["slr_euler_pair_workspace_bytes"] == (sz, [i] * 3)
    assert _lib.SIGNATURES["slr_euler_pair_backward"] == (i, [vp] * 3 + [i] * 3 + [vp] * 4 + [sz, vp])
    import slr_sfs_amd as S
    assert S.euler_integration_pair is S.euler_integration_manipulator.euler_integration_pair


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 20, 24), (1, 33, 31), (2, 256, 256), (1, 768, 1280), (65535, 2, 2)])
def test_workspace_bytes_is_the_documented_size(L, B, H, W):
    assert L.slr_euler_pair_workspace_bytes(B, H, W) == workspace_bytes(B, H, W)


def test_workspace_bytes_is_zero_for_refused_sizes(L):
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, -3), (1, 1 << 15, 1 << 15), (1, 1 << 20, 1 << 11)):
        assert L.slr_euler_pair_workspace_bytes(B, H, W) == 0, (B, H, W)
    assert L.slr_euler_pair_workspace_bytes(1, 1 << 15, (1 << 15) - 1) == workspace_bytes(1, 1 << 15, (1 << 15) - 1)


BAD_SIZES = [((0, 8, 8), b"sizes"), ((-2, 8, 8), b"sizes"), ((65536, 8, 8), b"sizes"), ((1, 0, 8), b"sizes"), ((1, 8, 0), b"sizes"),
             ((1, -8, 8), b"sizes"), ((1, 1 << 15, 1 << 15), b"too large"), ((3, 1 << 10, 1 << 20), b"too large")]


def test_forward_refusals(L):
    fwd = L.slr_euler_pair_forward
    good = [FAKE] * 3 + [1, 8, 8] + [FAKE] * 4
    for k in (0, 1, 2, 6, 7):                                             # motion, steps_f, steps_p, disp_f, disp_p (the visibility planes may be null)
        args = list(good)
        args[k] = None
        assert fwd(*args, None) == -1 and b"null" in L.slr_last_error(), k
    for (B, H, W), word in BAD_SIZES:
        rc = fwd(FAKE, FAKE, FAKE, B, H, W, FAKE, FAKE, None, None, None)
        assert rc == -1 and word in L.slr_last_error() and b"slr_euler_pair_forward" in L.slr_last_error(), (B, H, W, L.slr_last_error())


def test_backward_refusals(L):
    bwd = L.slr_euler_pair_backward
    need = workspace_bytes(2, 20, 24)
    good = [FAKE] * 3 + [2, 20, 24] + [FAKE] * 4 + [need]
    for k in (0, 1, 2, 6, 7, 8, 9):
        args = list(good)
        args[k] = None
        assert bwd(*args, None) == -1 and b"null" in L.slr_last_error(), k
    for (B, H, W), word in BAD_SIZES:
        rc = bwd(FAKE, FAKE, FAKE, B, H, W, FAKE, FAKE, FAKE, FAKE, 1 << 40, None)
        assert rc == -1 and word in L.slr_last_error() and b"slr_euler_pair_backward" in L.slr_last_error(), (B, H, W, L.slr_last_error())
    for nbytes in (0, 1280, need - 1, workspace_bytes(1, 20, 24)):
        args = list(good)
        args[10] = nbytes
        assert bwd(*args, None) == -2 and b"workspace" in L.slr_last_error(), nbytes
    args = list(good)
    args[9] = ctypes.c_void_p((1 << 20) + 4)                              # the int64 plane needs 8-byte alignment
    assert bwd(*args, None) == -2 and b"misaligned" in L.slr_last_error()


def test_python_refusals_come_before_the_device():
    import slr_sfs_amd as S
    pair = S.euler_integration_pair
    m = torch.zeros(2, 2, 8, 8)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        pair(m, [1, 2], [3, 4])
    with pytest.raises(NotImplementedError, match="no CPU path"):
        pair(m.requires_grad_(True), torch.tensor([1, 2]), torch.tensor([3, 4]))
    m = torch.zeros(2, 2, 8, 8)
    with pytest.raises(TypeError, match="tensor"):
        pair(np.zeros((2, 2, 8, 8), np.float32), [1, 2], [3, 4])
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(TypeError, match="float32"):
            pair(m.to(dtype), [1, 2], [3, 4])
    for shape in ((2, 8, 8), (2, 3, 8, 8), (2, 1, 8, 8), (0, 2, 8, 8), (2, 2, 0, 8), (1, 2, 2, 8, 8)):
        with pytest.raises(ValueError, match="motion"):
            pair(torch.zeros(shape), [1, 2], [3, 4])
    with pytest.raises(ValueError, match="not contiguous"):
        pair(torch.zeros(2, 2, 8, 16)[..., ::2], [1, 2], [3, 4])
    with pytest.raises(ValueError, match="steps_f"):
        pair(m, [1], [3, 4])
    with pytest.raises(ValueError, match="steps_p"):
        pair(m, torch.tensor([1, 2]), torch.tensor([3, 4, 5]))


def test_training_synthesis_takes_the_pair_only_when_asked(monkeypatch):
    """``euler_pair`` is a bool; off (the default) the module calls EulerIntegration twice as it always did, on it calls the pair
    operator once with the step counts of animating_softmax_splating.py:579-580 and never negates the motion."""
    import slr_sfs_amd as S
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(TypeError, match="euler_pair"):
            S.TrainingSynthesis(None, euler_pair=bad)
    assert S.TrainingSynthesis().euler_pair is False and S.TrainingSynthesis(None, True, True).euler_pair is True
    single, paired = [], []
    monkeypatch.setattr(S.training, "splat_blend", lambda *a, **k: a[0])
    monkeypatch.setattr(S.training.EulerIntegration, "forward", lambda self, m, n: single.append((m, n)) or m)
    monkeypatch.setattr(S.training, "euler_integration_pair", lambda m, nf, np_: paired.append((m, nf, np_)) or (m, m))
    x, m = torch.zeros(2, 2, 8, 8), torch.ones(2, 2, 8, 8)
    start, mid, end = torch.tensor([3.0, 0.0]), torch.tensor([10.0, 59.0]), torch.tensor([40.0, 59.0])
    S.TrainingSynthesis()(x, None, x, None, m, start, mid, end)
    assert len(single) == 2 and not paired
    assert single[0][0] is m and torch.equal(single[1][0], -m)
    assert single[0][1].tolist() == [7, 59] and single[1][1].tolist() == [31, 1]
    single.clear()
    S.TrainingSynthesis(None, euler_pair=True)(x, None, x, None, m, start, mid, end)
    assert not single and len(paired) == 1
    assert torch.equal(paired[0][0], m) and paired[0][1].tolist() == [7, 59] and paired[0][2].tolist() == [31, 1]
    assert paired[0][1].dtype == paired[0][2].dtype == torch.int64
