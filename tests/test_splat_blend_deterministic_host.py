"""Host-side checks of the deterministic ``splat_blend`` forward (no GPU): ABI 22 and its binding, the argument checks that happen
before the device is touched, and -- for every case of tests/test_gpu_splat_blend_deterministic.py -- which paths of the forward its
flows take, stated with numpy from the flows alone (tests/blend_det_cases.py) against the constants of csrc/slr_tuning.hpp."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import blend_det_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slr-sfs_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


def test_abi_22_and_the_binding_table(L):
    from slr_sfs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slr_splat.h")).read()
    assert int(re.search(r"#define\s+SLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == L.slr_abi_version()
    assert _lib.ABI_VERSION >= 22
    assert int(re.search(r"#define\s+SLR_BLEND_DETERMINISTIC\s+(\d+)", hdr).group(1)) == _lib.BLEND_DETERMINISTIC == 1
    for name in ("slr_splat_blend_forward_ex", "slr_splat_fallback_count_offset"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    # the _ex call is the plain one with `flags` in front of the scratch pointer
    plain, ex = _lib.SIGNATURES["slr_splat_blend_forward"], _lib.SIGNATURES["slr_splat_blend_forward_ex"]
    assert ex[0] is plain[0] and ex[1] == plain[1][:21] + [ctypes.c_int] + plain[1][21:]


def test_unknown_flag_bits_are_refused_before_the_device(L):
    ex = L.slr_splat_blend_forward_ex
    nulls = [None] * 9
    for flags in (2, 4, 3, -2, 1 << 30):
        rc = ex(*nulls, -20.0, 20.0, 1e-8, None, None, 1, 1, 8, 8, None, 0, 0, flags, None, 0, None)
        assert rc == -1 and b"flags" in L.slr_last_error(), (flags, rc, L.slr_last_error())
    for flags in (0, 1):                                           # known bits: the next check speaks (null pointers)
        rc = ex(*nulls, -20.0, 20.0, 1e-8, None, None, 1, 1, 8, 8, None, 0, 0, flags, None, 0, None)
        assert rc == -1 and b"null" in L.slr_last_error(), (flags, rc, L.slr_last_error())


def test_fallback_word_lies_in_the_zeroed_head_of_the_workspace(L):
    off = L.slr_splat_fallback_count_offset
    assert off(0, 8, 8) == 0 and off(1, 0, 8) == 0 and off(1, 8, -1) == 0
    for N, H, W in ((1, 8, 8), (2, 256, 256), (1, 768, 1280)):
        o = off(N, H, W)
        assert o > 0 and o % 4 == 0 and o + 4 <= L.slr_splat_workspace_bytes(N, H, W)
    # the word is one of the 64 of totals[] that no kernel touches: splat_ws.hpp names it, the kernels index totals[] below 24
    ws = open(os.path.join(CSRC, "splat_ws.hpp")).read()
    word = int(re.search(r"DET_FALLBACK_WORD\s*=\s*(\d+)", ws).group(1))
    assert 24 <= word < 64
    op = open(os.path.join(CSRC, "splat_op.hip")).read() + open(os.path.join(CSRC, "splat_clip.hip")).read()
    used = [int(v) for v in re.findall(r"totals\s*(?:\+|\[)\s*(\d+)", op)]
    assert used and max(used) < 24, sorted(set(used))
    assert "atomicAdd(f.totals + DET_FALLBACK_WORD, 1u)" in op and len(re.findall(r"DET_FALLBACK_WORD", op)) == 3      # one increment, the comment, the getter


def test_deterministic_is_a_bool_and_cpu_tensors_raise():
    import slr_sfs_amd as S
    x, f, a = torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8), torch.full((1,), 0.5)
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(TypeError, match="deterministic"):
            S.splat_blend(x, None, f, x, None, f, a, deterministic=bad)
        with pytest.raises(TypeError, match="deterministic"):
            S.TrainingSynthesis(None, deterministic=bad)
    for det in (True, False):
        with pytest.raises(NotImplementedError, match="no CPU path"):
            S.splat_blend(x, None, f, x, None, f, a, deterministic=det)
    assert S.TrainingSynthesis(None, deterministic=True).deterministic is True and S.TrainingSynthesis().deterministic is False
    with pytest.raises(NotImplementedError, match="no CPU path"):
        S.training.splat_blend_fallback_count(x)


def test_the_default_call_of_training_synthesis_is_unchanged(monkeypatch):
    """``deterministic`` travels to splat_blend only when it is set: the default module calls it as it always did."""
    import slr_sfs_amd as S
    seen = []
    monkeypatch.setattr(S.training, "splat_blend", lambda *a, **k: seen.append(k) or a[0])
    monkeypatch.setattr(S.training.EulerIntegration, "forward", lambda self, m, n: m)
    x, m, i = torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8), torch.tensor([1.0])
    S.TrainingSynthesis()(x, None, x, None, m, 0 * i, i, 2 * i)
    S.TrainingSynthesis(None, deterministic=True)(x, None, x, None, m, 0 * i, i, 2 * i)
    assert seen == [dict(clamp_z=(-20.0, 20.0), subtract_max=True), dict(clamp_z=(-20.0, 20.0), subtract_max=True, deterministic=True)]
    import inspect
    assert inspect.signature(S.TrainingModel.__init__).parameters["deterministic"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(S.training._SplatBlend.forward).parameters)[:12] == [
        "ctx", "start_fs", "z_start", "flow_f", "end_fs", "z_end", "flow_p", "alpha", "lo", "hi", "subtract_max", "eps"]
    assert "are_deterministic_algorithms_enabled" not in open(os.path.join(ROOT, "slr-sfs_amd", "training.py")).read()


def test_quoted_constants_are_the_shipped_ones():
    tuning = open(os.path.join(CSRC, "slr_tuning.hpp")).read()
    for name, value in K.TUNING.items():
        assert int(re.search(rf"#define\s+{name}\s+(-?\d+)", tuning).group(1)) == value, name
    assert K.SEG == K.TUNING["SLR_EPT_ONE"] * K.TILE_H * K.TILE_W and K.PASS_SEG == K.TUNING["SLR_EPT_DEFER"] * K.TILE_H * K.TILE_W
    tile = open(os.path.join(CSRC, "splat_tile.hpp")).read()
    assert "bal = mx > bal_s + (uint32_t)SLR_BAL_SLACK ? 1 : 2;" in tile and "bal_s = (ntot + TT - 1u) / TT;" in tile
    assert "if (total <= (uint32_t)SLR_SCAN_DEFER_AT)" in open(os.path.join(CSRC, "splat_op.hip")).read()


def test_paths_of_a_flow_by_hand():
    """``paths`` on flows whose entries and records can be counted by hand."""
    H, W = 16, 128
    p = K.paths(np.zeros((1, 2, H, W), np.float32))
    # the identity: every source has four in-image corners except on the right / bottom edge; a tile's entries are its own pixels, the
    # row above it and the column to its left
    assert p["records"][0, 0, 0] == 1 and p["records"][0, 5, 5] == 4 and p["records"][0, 0, 5] == 2
    assert p["tiles"][0].tolist() == [[8 * 64, 8 * 65], [9 * 64, 9 * 65]]
    assert p["octants"][0, 0, 0].tolist() == [64] + [72] * 7 and not p["dropped"].any()
    fl = np.zeros((1, 2, H, W), np.float32)
    fl[0, 0, 3, 7], fl[0, 1, 4, 4], fl[0, :, 9, 9] = np.nan, np.inf, 2.0 ** 31
    p = K.paths(fl)
    assert int(p["dropped"].sum()) == 3 and p["tiles"][0, 0, 0] == 8 * 64 - 2
    everything = np.zeros((1, 2, H, W), np.float32)                  # every source onto pixel (4, 70): one list of H * W records
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    everything[0, 0], everything[0, 1] = 70 - x, 4 - y
    p = K.paths(everything)
    assert p["records"][0, 4, 70] == H * W and p["tiles"][0].tolist() == [[0, H * W], [0, 0]] and p["octants"][0, 0, 1, 0] == H * W
    assert K.balanced(K.tile_lists(p["records"], 0, 0, 1)) and not K.balanced(K.tile_lists(K.paths(np.zeros_like(fl))["records"], 0, 0, 0))
    assert K.plan_pieces(2048, [256] * 8) == [(0, 3), (3, 3), (6, 2)]


CASE_IDS = [(name, None) for name in K.CASES] + [(name, 32) for name in ("plain", "row_pile", "sink")]


@pytest.mark.parametrize("name,channels", CASE_IDS, ids=lambda v: str(v))
def test_every_case_reaches_its_paths(oracle, name, channels):
    c = K.make_case(name, oracle, channels=channels)
    assert tuple(c["start_fs"].shape) == K.CASES[name]["shape"][:1] + (channels or K.CASES[name]["shape"][1],) + K.CASES[name]["shape"][2:]
    conds = K.conditions(name, c)
    assert len(conds) >= 4
    for what, ok in conds:
        print(f"  {name}: {what}: {ok}")
    assert all(ok for _, ok in conds), [what for what, ok in conds if not ok]
    # the same flows every time: a case is its seed
    again = K.make_case(name, oracle, channels=channels)
    assert np.array_equal(c["flow_f"], again["flow_f"], equal_nan=True) and np.array_equal(c["start_fs"], again["start_fs"])


def test_the_fallback_case_exceeds_the_small_entry_array():
    ws = open(os.path.join(CSRC, "splat_ws.hpp")).read()
    assert "(L.nt <= (uint32_t)SLR_SCAN_MAX_TILES ? SLR_SINK_ENT_MB : 1) << 20) / 16" in ws          # 1 MiB of 16-byte entries above the threshold
    tuning = open(os.path.join(CSRC, "slr_tuning.hpp")).read()
    assert int(re.search(r"#define\s+SLR_SCAN_MAX_TILES\s+(\d+)", tuning).group(1)) == K.SCAN_MAX_TILES
    conds = K.fallback_conditions(K.fallback_case())
    assert len(conds) == 4 and all(ok for _, ok in conds), conds
