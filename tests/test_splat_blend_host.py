"""Host-side checks of the two-direction blend (slr_sfs_amd.training, csrc/blend.hip): no GPU needed.

  1. the float64 yardstick tests/blend_f64.py agrees with splat_f64.training_step (pinned to the reference by test_splat_f64.py) when both
     directions get the same features and logits -- values and every gradient, to 1e-12 relative;
  2. splat_blend refuses CPU tensors, wrong shapes, dtypes and layouts; TrainingSynthesis maps the reference's option flags and refuses
     the paths it does not implement;
  3. the raw C ABI returns -1 with a message for NULL pointers and non-positive sizes, and its scratch size is host arithmetic."""
import argparse
import os

import numpy as np
import pytest
import torch

import blend_f64 as B64
import splat_f64 as F64


@pytest.fixture(scope="module")
def L():
    import slr_sfs_amd
    if not os.path.exists(slr_sfs_amd._lib.LIB_PATH):
        slr_sfs_amd._lib.build()
    return slr_sfs_amd._lib.lib()


@pytest.mark.parametrize("clamp_z", [(-20.0, 20.0), None, (-1.0, 0.5)])
def test_yardstick_agrees_with_training_step(clamp_z):
    rng = np.random.default_rng(5)
    N, C, H, W = 2, 5, 11, 13
    fs, Z = rng.standard_normal((N, C, H, W)), rng.standard_normal((N, 1, H, W)) * 2
    ff, fp = rng.uniform(-3, 3, (N, 2, H, W)).astype(np.float32), rng.uniform(-3, 3, (N, 2, H, W)).astype(np.float32)
    ff[0, 0, 2, 3], fp[1, 1, 4, 5], fp[0, :, 0, 0] = np.nan, np.inf, 3.0e9
    alpha = torch.tensor([0.5, 1.0 / 60.0], dtype=torch.float64)
    go = torch.from_numpy(rng.standard_normal((N, C, H, W)))

    def leaves():
        return [torch.from_numpy(a).double().requires_grad_(True) for a in (fs, Z, ff, fp)]
    a = leaves()
    ref = F64.training_step(a[0], a[1], a[2], a[3], alpha.view(N, 1, 1, 1), clamp_z=clamp_z)
    gref = torch.autograd.grad(ref, a, go)
    b = leaves()
    got = B64.blend_f64(b[0], b[1], b[2], b[0], b[1], b[3], alpha, clamp_z=clamp_z)
    ggot = torch.autograd.grad(got, b, go)
    for name, x, y in [("out", got, ref)] + [(n, g, r) for n, g, r in zip(("fs", "Z", "flow_f", "flow_p"), ggot, gref)]:
        x, y = x.detach(), y.detach()
        scale = float(y.abs().max())
        assert scale > 0 and bool(torch.isfinite(y).all()), name
        assert float((x - y).abs().max()) <= 1e-12 * scale, (name, float((x - y).abs().max()), scale)
    # a hole of the output is exactly +0.0, a dropped source has exactly no gradient
    assert bool((ggot[2][0, :, 2, 3] == 0).all()) and bool((ggot[3][1, :, 4, 5] == 0).all()) and bool((ggot[3][0, :, 0, 0] == 0).all())


def test_yardstick_options():
    """z = None weights by alpha only (= logits of zero), subtract_max=False leaves the logits alone."""
    rng = np.random.default_rng(6)
    N, C, H, W = 1, 3, 6, 7
    t = lambda *s: torch.from_numpy(rng.standard_normal(s))
    vf, vp, zf, zp, ff, fp = t(N, C, H, W), t(N, C, H, W), t(N, 1, H, W), t(N, 1, H, W), t(N, 2, H, W).float(), t(N, 2, H, W).float()
    alpha = torch.tensor([0.3], dtype=torch.float64)
    none = B64.blend_f64(vf, None, ff, vp, None, fp, alpha)
    zero = B64.blend_f64(vf, torch.zeros_like(zf), ff, vp, torch.zeros_like(zp), fp, alpha)
    assert torch.equal(none, zero)
    v1 = B64.blend_f64(vf, zf, ff, vp, zp, fp, alpha, subtract_max=False, clamp_z=None)
    shifted = B64.blend_f64(vf, zf + zf.max(), ff, vp, zp + zp.max(), fp, alpha, clamp_z=None)
    # (a common factor per direction does NOT cancel between directions: the shift must be the one of each direction's own maximum)
    full = B64.blend_f64(vf, zf, ff, vp, zp, fp, alpha, clamp_z=None)
    assert float((shifted - full).abs().max()) <= 1e-12 * float(full.abs().max())
    assert float((v1 - full).abs().max()) > 1e-6


def _cpu_case(N=1, C=2, H=4, W=5):
    z = lambda *s: torch.zeros(*s)
    return dict(start_fs=z(N, C, H, W), z_start=z(N, 1, H, W), flow_f=z(N, 2, H, W), end_fs=z(N, C, H, W), z_end=z(N, 1, H, W),
                flow_p=z(N, 2, H, W), alpha=z(N))


def test_splat_blend_refuses_cpu_tensors():
    import slr_sfs_amd as S
    with pytest.raises(NotImplementedError):
        S.splat_blend(**_cpu_case())
    with pytest.raises(NotImplementedError):
        S.training.splat_blend(**dict(_cpu_case(), z_start=None, z_end=None))


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the device: the argument checks run in front of every device call, so they can be reached
    without one."""
    @property
    def is_cuda(self):
        return True


def _fake(t):
    return None if t is None else t.as_subclass(_FakeCuda)


@pytest.mark.parametrize("change,exc", [
    (dict(end_fs=torch.zeros(1, 3, 4, 5)), ValueError),
    (dict(flow_f=torch.zeros(1, 3, 4, 5)), ValueError),
    (dict(flow_p=torch.zeros(1, 2, 5, 4)), ValueError),
    (dict(z_start=torch.zeros(1, 2, 4, 5)), ValueError),
    (dict(z_end=torch.zeros(1, 4, 5)), ValueError),
    (dict(alpha=torch.zeros(2)), ValueError),
    (dict(start_fs=torch.zeros(2, 4, 5)), ValueError),
    (dict(start_fs=torch.zeros(1, 2, 4, 5, dtype=torch.float64)), TypeError),
    (dict(alpha=torch.zeros(1, dtype=torch.float16)), TypeError),
    (dict(flow_f=torch.zeros(1, 2, 5, 4).transpose(2, 3)), ValueError),
    (dict(start_fs=torch.zeros(1, 4, 4, 5)[:, ::2]), ValueError),
    (dict(z_end=torch.zeros(1, 1, 4, 10)[..., ::2]), ValueError),
])
def test_splat_blend_refuses_bad_arguments_before_the_device(change, exc, monkeypatch):
    import slr_sfs_amd as S

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(S.training, "call", no_device)
    monkeypatch.setattr(S.training, "workspace", no_device)
    case = {k: _fake(v) for k, v in dict(_cpu_case(), **change).items()}
    with pytest.raises(exc):
        S.splat_blend(**case)
    with pytest.raises(ValueError):
        S.splat_blend(**{k: _fake(v) for k, v in _cpu_case().items()}, clamp_z=(1.0, -1.0))
    with pytest.raises(ValueError):
        S.splat_blend(**{k: _fake(v) for k, v in _cpu_case().items()}, eps=0.0)


def test_training_synthesis_reads_the_reference_flags():
    import slr_sfs_amd as S
    ns = argparse.Namespace
    assert S.TrainingSynthesis().options == dict(train_z=False, subtract_max=True, clamp_z=(-20.0, 20.0))
    assert S.TrainingSynthesis(ns(train_Z=True)).options == dict(train_z=True, subtract_max=True, clamp_z=(-20.0, 20.0))
    assert S.TrainingSynthesis(ns(train_Z=True, use_softmax_splatter_v1=True)).options["subtract_max"] is False
    assert S.TrainingSynthesis(dict(train_Z=True, use_softmax_splatter_v1=False)).options["subtract_max"] is True
    # "no_clamp_Z" in self.opt: the attribute's EXISTENCE switches the clamp off, whatever its value
    assert S.TrainingSynthesis(ns(train_Z=True, no_clamp_Z=False)).options["clamp_z"] is None
    assert S.TrainingSynthesis(ns(train_Z=True, no_clamp_Z=True)).options["clamp_z"] is None
    assert S.TrainingSynthesis({"no_clamp_Z": False}).options["clamp_z"] is None
    assert S.TrainingSynthesis(ns(train_Z=False)).options["train_z"] is False
    for flag in ("use_softmax_splatter_v2", "use_softmax_splatter_v3", "use_3d_splatter", "use_mesh_splatter", "random_ff_mask"):
        with pytest.raises(NotImplementedError, match=flag):
            S.TrainingSynthesis(ns(train_Z=True, **{flag: True}))
        S.TrainingSynthesis(ns(train_Z=True, **{flag: False}))                  # present and off: fine
    assert isinstance(S.TrainingSynthesis().euler_integration, S.EulerIntegration)


def test_blend_abi_refuses_bad_arguments(L):
    inf = float("inf")
    p = 256                                              # a non-null, aligned address: the argument checks never dereference it
    fwd = lambda **k: L.slr_splat_blend_forward(*[k.get(n, p) for n in ("vf", "zf", "df", "vp", "zp", "dp", "alpha", "mf", "mp")],
                                                k.get("lo", -20.0), k.get("hi", 20.0), k.get("eps", 1e-8), k.get("out", p), k.get("norm", p),
                                                k.get("N", 1), k.get("C", 4), k.get("H", 8), k.get("W", 8), k.get("ws", p), k.get("wsb", 1 << 40),
                                                k.get("flags", 0), k.get("scratch", p), k.get("sb", 1 << 40), None)
    bwd = lambda **k: L.slr_splat_blend_backward(*[k.get(n, p) for n in ("vf", "zf", "df", "vp", "zp", "dp", "alpha", "mf", "mp")],
                                                 k.get("lo", -20.0), k.get("hi", 20.0), k.get("eps", 1e-8), k.get("out", p), k.get("norm", p),
                                                 k.get("gout", p), *[k.get(n, p) for n in ("gvf", "gzf", "gdf", "gvp", "gzp", "gdp")],
                                                 k.get("N", 1), k.get("C", 4), k.get("H", 8), k.get("W", 8), k.get("scratch", p), k.get("sb", 1 << 40), None)
    for name in ("vf", "df", "vp", "dp", "alpha", "out", "norm"):
        assert fwd(**{name: None}) == -1 and b"null" in L.slr_last_error(), name
    for name in ("vf", "df", "vp", "dp", "alpha", "out", "norm", "gout"):
        assert bwd(**{name: None}) == -1 and b"null" in L.slr_last_error(), name
    for f in (fwd, bwd):
        for dim in ("N", "C", "H", "W"):
            for bad in (0, -3):
                assert f(**{dim: bad}) == -1 and b"sizes" in L.slr_last_error(), (dim, bad)
        assert f(lo=1.0, hi=-1.0) == -1 and b"clamp" in L.slr_last_error()
        assert f(eps=0.0) == -1
        assert f(scratch=None) == -1 and b"scratch" in L.slr_last_error()
        assert f(sb=16) == -1 and b"scratch" in L.slr_last_error()
        assert f(scratch=p + 4) == -1
    assert fwd(ws=None) == -1 and b"workspace" in L.slr_last_error()
    assert fwd(wsb=16) == -1
    assert fwd(ws=p + 8) == -1 and b"workspace" in L.slr_last_error()       # (misaligned: refused before the first launch)
    assert fwd(N=40000, H=1, W=1) == -1 and b"sizes" in L.slr_last_error()   # (the batch is a grid dimension)
    assert fwd(flags=1) == -1 and b"prebinned" in L.slr_last_error()
    assert bwd(zf=None) == -1 and b"logits" in L.slr_last_error()          # a gradient of logits that were not given
    assert bwd(zp=None) == -1
    assert fwd(lo=-inf, hi=inf, N=0) == -1                                   # (the infinite range itself is accepted: "sizes" is what fails)
    assert b"sizes" in L.slr_last_error()


def test_blend_scratch_size_is_host_arithmetic(L):
    f = L.slr_splat_blend_ws_bytes
    for shape in ((0, 64, 256, 256), (2, 0, 256, 256), (2, 64, 0, 256), (2, 64, 256, 0), (-1, 64, 256, 256)):
        assert f(*shape) == 0, shape
    # the forward's raw sums of the two directions ([N,C,H,W] + a normaliser plane each) set the size; nothing else grows with C
    assert f(2, 64, 256, 256) == 2 * 2 * 65 * 256 * 256 * 4
    assert f(1, 64, 768, 1280) == 2 * 65 * 768 * 1280 * 4
    assert f(1, 1, 1, 1) >= 4 * 256
    # one channel: the backward's partial sums (2 aux planes + 2 directions x 3 planes per sample) are the larger part
    assert f(2, 1, 256, 256) >= (2 + 6) * 2 * 256 * 256 * 4
