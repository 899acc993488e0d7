"""The kernels of csrc/metrics.hip one by one against float64 definitions (tests/metrics_fixture.py), on the frames clips really contain
(flat, saturated, posterised), in every SSIM window instantiation, at the tile edges, with every mask form, and at the shape the
evaluation runs at (batches of four 720 x 1280 pairs); evaluate_clip across chunk boundaries.  tests/test_gpu_metrics.py holds the
comparison with the reference's own outputs on textured frames.

Where a bound has the form 6 E_ref + 1e-6, E_ref is the error of the SAME definition evaluated by torch in float32 on the CPU (the
reference's formulation at the reference's precision) against float64, computed in the test from the test's inputs and never from the
kernel; the form and the factor are those of test_decoder_on_the_fp32_rung_vs_fp64.  Every such test prints its figures (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import metrics_fixture as MF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import slr_sfs_amd
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd.metrics


@pytest.fixture(scope="module")
def vgg(M):
    return M.load_vgg16_state_dict(M.PerceptualVGG16(), MF.vgg16_state_dict()).cuda()


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------ A. SSIM / MSE

N_NOISY = 2


@functools.lru_cache(maxsize=2)
def _hard(form, H, W):
    """(names, device inputs x / y, CPU float [n,3,H,W] a / b) of the hard family followed by N_NOISY textured pairs."""
    pa, pb = MF.image_pair(H, W, n=N_NOISY, tag="hard_noisy")
    if form == "uint8":
        fam = MF.hard_pairs(H, W)
        a = np.stack([v[0] for v in fam.values()] + list(pa))
        b = np.stack([v[1] for v in fam.values()] + list(pb))
        x, y, a, b = _t(a), _t(b), MF.to_tensor(a), MF.to_tensor(b)
    else:
        fam = MF.hard_pairs_float(H, W)
        a = torch.cat([torch.stack([_t(v[0]) for v in fam.values()]), MF.to_tensor(pa)])
        b = torch.cat([torch.stack([_t(v[1]) for v in fam.values()]), MF.to_tensor(pb)])
        x, y = a, b
    return list(fam) + [f"noisy{i}" for i in range(N_NOISY)], x, y, a, b


@pytest.mark.parametrize("form", ["uint8", "float"])
@pytest.mark.parametrize("ws", [11, 7])
@pytest.mark.parametrize("hw", [(48, 80), (720, 1280)])
def test_ssim_hard_frames_vs_fp64(M, hw, ws, form):
    """slr_ssim_mse on flat, saturated and posterised frames (metrics_fixture.hard_pairs / hard_pairs_float), with and without a mask,
    against ssim_f64 / psnr_f64.  sigma = E[x^2] - mu^2 is formed in fp32 here as in the reference; on a flat frame every pixel carries
    the same rounding error and nothing averages out, so the 1e-5 of the textured frames does not hold for either implementation.
    Per window, with E_ref = max over the hard family of |ssim_f32_reference - float64| (required < 2e-3, so a broken yardstick cannot
    widen the bound): every case within 6 E_ref + 1e-6 of float64; identical frames: MSE exactly 0, PSNR inf, |SSIM - 1| <= 2 * 2^-23;
    |dPSNR| <= 1e-4 dB wherever MSE > 0; the textured pairs of the same batch within 1e-5 as in tests/test_gpu_metrics.py.

    Measured on an MI355X (max e_gpu over the hard family | E_ref | ratio), masked and unmasked together:
      48 x 80    window 11  uint8 3.75e-4 | 1.24e-3 | 0.30    float 1.09e-4 | 4.57e-4 | 0.24
      48 x 80    window 7   uint8 1.51e-4 | 7.52e-4 | 0.20    float 1.25e-4 | 1.79e-4 | 0.70
      720 x 1280 window 11  uint8 5.19e-4 | 1.69e-3 | 0.31    float 2.16e-4 | 9.53e-4 | 0.23
      720 x 1280 window 7   uint8 1.94e-4 | 9.15e-4 | 0.21    float 1.09e-4 | 6.10e-4 | 0.18
    Per case the ratio goes both ways: 1.00 on flat 253 vs 252 (5.19e-4 both), 5.6 on the half-saturated frame at window 7 (1.94e-4
    against 3.46e-5).  Textured pairs: 2.4e-6; identical frames: SSIM 1 and MSE 0 exactly; |dPSNR| <= 6.5e-6 dB."""
    H, W = hw
    names, x, y, a, b = _hard(form, H, W)
    n = len(names)
    mask = _t(MF.mask_for(H, W, n=n, tag="hard_mask"))
    xd, yd = x.cuda(), y.cuda()
    got = {}
    for key, m in (("plain", None), ("mask", mask)):
        sm = M.ssim_mse(xd, yd, ws, None if m is None else m.cuda())
        got[key] = (sm[:, 0].cpu().double(), sm[:, 1].cpu(), M.psnr_from_mse(sm[:, 1]).cpu().double())
    rows = []
    for i, name in enumerate(names):
        ai, bi = a[i:i + 1], b[i:i + 1]
        m64 = MF.ssim_map(ai, bi, ws, torch.float64, separable=H >= 256)
        m32 = MF.ssim_map(ai, bi, ws, torch.float32)
        if i == 0 and H < 256:                                           # the separable float64 form is the 2-D one
            assert float((MF.ssim_map(ai, bi, ws, torch.float64, separable=True) - m64).abs().max()) < 1e-10
        for key, m in (("plain", None), ("mask", mask[i:i + 1])):
            f64, f32 = float(MF.ssim_reduce(m64, m, False)), float(MF.ssim_reduce(m32, m, False))
            rows.append((name, key, float(got[key][0][i]), f64, abs(f32 - f64), float(got[key][1][i]), float(got[key][2][i]),
                         float(MF.psnr_f64(ai, bi, m))))
    hard = [r for r in rows if not r[0].startswith("noisy")]
    E_ref = max(r[4] for r in hard)
    bound = 6 * E_ref + 1e-6
    bad = []
    for name, key, s, f64, e_ref, mse, psnr, psnr64 in rows:
        e_gpu = abs(s - f64)
        print(f"[hard {H}x{W} w{ws} {form} {key:5s}] {name:24s} ssim {f64:.7f} e_gpu {e_gpu:.2e} e_ref {e_ref:.2e} "
              f"ratio {e_gpu / e_ref if e_ref else float('nan'):.2f} psnr {psnr64:.4f} dpsnr {abs(psnr - psnr64):.1e}")
        if name.startswith("noisy"):
            if e_gpu > 1e-5:
                bad.append((name, key, "textured frames: 1e-5", e_gpu))
        elif e_gpu > bound:
            bad.append((name, key, "6 E_ref + 1e-6", e_gpu, bound))
        if name == "self":
            if mse != 0.0 or psnr != float("inf") or psnr64 != float("inf") or abs(s - 1.0) > 2 * 2.0 ** -23:
                bad.append((name, key, "identical frames", mse, psnr, s - 1.0))
        elif not (mse > 0 and abs(psnr - psnr64) <= 1e-4):
            bad.append((name, key, "psnr", mse, psnr, psnr64))
    e_max = max(abs(r[2] - r[3]) for r in hard)
    print(f"[hard {H}x{W} w{ws} {form}] max e_gpu {e_max:.2e}  E_ref {E_ref:.2e}  ratio {e_max / E_ref:.3f}  bound {bound:.2e}")
    assert E_ref < 2e-3, E_ref
    assert not bad, bad


SIZES_EDGE = ((15, 63), (16, 64), (17, 65), (1, 1), (1, 200), (200, 1), (3, 130))       # one below / at / one above the 16 x 64 tile, lines
CHANNELS = (1, 2, 3, 4, 64)


@pytest.mark.parametrize("ws", [1, 3, 5, 7, 9, 11, 13, 15])
def test_ssim_every_window_and_channel_count(M, ws):
    """Every instantiation of ssim_tile_kernel (R = 0 .. 7; R = 7 fills the LDS patch exactly), float input with 1, 2, 3, 4 and 64
    channels (uint8 as well at 3), at the tile edges and on single rows / columns / pixels, masked and not, against ssim_f64 / psnr_f64
    on textured frames: |dSSIM| <= 1e-5, |dPSNR| <= 1e-4 dB as in tests/test_gpu_metrics.py.  For a (window, size) at which the fp32
    restatement of the reference is itself more than 5e-6 from float64 (E_ref, computed here, over the channel counts and masks), the bound
    is 6 E_ref + 1e-6 instead.  On the CPU this was written on that is: window 3 at 15 x 63, 16 x 64, 17 x 65 (6.5e-6, 6.8e-6, 7.1e-6), window 11 at 17 x 65
    (5.3e-6), window 13 at 17 x 65 (5.1e-6); every other (window, size) keeps 1e-5.
    The masked MSE divides by 3 * (mask sum) whatever C is, as metrics.py:16-17 of the reference does; psnr_f64 has the same literal 3,
    so changing that is a decision and not an accident."""
    bad = []
    for H, W in SIZES_EDGE:
        rows = []
        for C in CHANNELS:
            a_u8, b_u8 = MF.image_pair(H, W, n=2, tag="edge", C=C)
            a, b = _t(a_u8).permute(0, 3, 1, 2).float().div(255.0).contiguous(), _t(b_u8).permute(0, 3, 1, 2).float().div(255.0).contiguous()
            mask = _t(MF.mask_for(H, W, n=2, tag=f"edge{C}"))
            m64, m32 = MF.ssim_map(a, b, ws, torch.float64), MF.ssim_map(a, b, ws, torch.float32)
            forms = [("float", a.cuda(), b.cuda())] + ([("uint8", _t(a_u8).cuda(), _t(b_u8).cuda())] if C == 3 else [])
            for key, m in (("plain", None), ("mask", mask)):
                f64, f32 = MF.ssim_reduce(m64, m, False), MF.ssim_reduce(m32, m, False)
                p64 = MF.psnr_f64(a, b, m)
                for form, x, y in forms:
                    sm = M.ssim_mse(x, y, ws, None if m is None else m.cuda())
                    rows.append((C, key, form, sm[:, 0].cpu().double(), f64, float((f32 - f64).abs().max()),
                                 M.psnr_from_mse(sm[:, 1]).cpu().double(), p64))
        E_ref = max(r[5] for r in rows)
        tol = 1e-5 if E_ref <= 5e-6 else 6 * E_ref + 1e-6
        e_max = max(float((r[3] - r[4]).abs().max()) for r in rows)
        print(f"[edge w{ws} {H}x{W}] max e_gpu {e_max:.2e}  E_ref {E_ref:.2e}  tol {tol:.2e}")
        for C, key, form, s, f64, _, p, p64 in rows:
            if float((s - f64).abs().max()) > tol:
                bad.append((H, W, C, key, form, "ssim", s.tolist(), f64.tolist(), tol))
            if not np.allclose(p.numpy(), p64.numpy(), rtol=0, atol=1e-4):
                bad.append((H, W, C, key, form, "psnr", p.tolist(), p64.tolist()))
    assert not bad, bad


def test_ssim_mask_forms(M):
    """A [1,1,H,W] mask is the same mask repeated over the batch (bit-exact); an all-zero mask gives SSIM 0 and MSE 0 (the divisor is
    clamped to 1); an all-one mask and a mask that is one on the single last pixel of a partial tile (37 x 61: row 36, column 60) against
    float64.  One pixel averages nothing, so its bound is 6 E_ref + 1e-6 with E_ref the largest per-pixel error of the fp32 restatement
    over the image (channel mean of the map, as the masked form takes it)."""
    H, W, n = 37, 61, 3
    a_u8, b_u8 = MF.image_pair(H, W, n=n, tag="maskforms")
    a, b = MF.to_tensor(a_u8), MF.to_tensor(b_u8)
    one = _t(MF.mask_for(H, W, n=1, tag="maskforms"))
    for x, y in ((a.cuda(), b.cuda()), (_t(a_u8).cuda(), _t(b_u8).cuda())):
        assert torch.equal(M.ssim_mse(x, y, 11, one.cuda()), M.ssim_mse(x, y, 11, one.expand(n, 1, H, W).contiguous().cuda()))
        np.testing.assert_allclose(M.ssim_mse(x, y, 11, one.cuda())[:, 0].cpu().numpy(), MF.ssim_f64(a, b, 11, one).numpy(), rtol=0, atol=1e-5)
        zero = M.ssim_mse(x, y, 11, torch.zeros(n, 1, H, W, device="cuda"))
        assert torch.equal(zero, torch.zeros(n, 2, device="cuda")), zero
        ones = torch.ones(n, 1, H, W)
        sm = M.ssim_mse(x, y, 11, ones.cuda())
        np.testing.assert_allclose(sm[:, 0].cpu().numpy(), MF.ssim_f64(a, b, 11, ones).numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(sm[:, 0].cpu().numpy(), M.ssim_mse(x, y, 11)[:, 0].cpu().numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(M.psnr_from_mse(sm[:, 1]).cpu().numpy(), MF.psnr_f64(a, b, ones).numpy(), rtol=0, atol=1e-4)
        np.testing.assert_allclose(M.psnr(x, y, ones.cuda()).cpu().numpy(), M.psnr(x, y).cpu().numpy(), rtol=0, atol=1e-4)
        for py, px in ((H - 1, W - 1), (0, 0), (16, 0), (35, 17), (H - 1, 0)):                # (35: the fourth row of a thread's four)
            pix = torch.zeros(n, 1, H, W)
            pix[:, :, py, px] = 1.0
            m64, m32 = MF.ssim_map(a, b, 11, torch.float64), MF.ssim_map(a, b, 11, torch.float32)
            E_ref = float((m32.double().mean(1) - m64.mean(1)).abs().max())
            sm = M.ssim_mse(x, y, 11, pix.cuda())
            want = m64.mean(1)[:, py, px]
            err = float((sm[:, 0].cpu().double() - want).abs().max())
            print(f"[mask pixel ({py},{px})] e_gpu {err:.2e}  E_ref (per pixel) {E_ref:.2e}")
            assert err <= 6 * E_ref + 1e-6, (py, px, err, E_ref)
            np.testing.assert_allclose(M.psnr_from_mse(sm[:, 1]).cpu().numpy(), MF.psnr_f64(a, b, pix).numpy(), rtol=0, atol=1e-4)


def test_ssim_hard_frames_720p_deterministic_and_batch_independent(M):
    """Five frames of the hard family at 720 x 1280: two calls are bit-identical, and frame 3 alone equals frame 3 inside the batch."""
    fam = MF.hard_pairs(720, 1280)
    pick = ("half_saturated", "flat255-1", "posterised+1", "flat199-3", "shift1")
    x = _t(np.stack([fam[k][0] for k in pick])).cuda()
    y = _t(np.stack([fam[k][1] for k in pick])).cuda()
    mask = _t(MF.mask_for(720, 1280, n=5, tag="hard_det")).cuda()
    for ws in (11, 7):
        for m in (None, mask):
            sm = M.ssim_mse(x, y, ws, m)
            assert torch.equal(sm, M.ssim_mse(x, y, ws, m))
            assert torch.equal(sm[3:4], M.ssim_mse(x[3:4], y[3:4], ws, None if m is None else m[3:4]))
    f = MF.to_tensor(np.stack([fam[k][0] for k in pick])).cuda(), MF.to_tensor(np.stack([fam[k][1] for k in pick])).cuda()
    np.testing.assert_allclose(M.ssim_mse(*f).cpu().numpy(), M.ssim_mse(x, y).cpu().numpy(), rtol=0, atol=1e-7)    # v / 255 as floats: same values in


# ------------------------------------------------------------------ B. feature distance, input scaling, pooling

FD_SHAPES = ((1, 1), (3, 85), (16, 16), (1, 257), (45, 80), (90, 160))         # 255 / 256 / 257 pixels: one below / at / above a workgroup


@pytest.mark.parametrize("C", [8, 64, 128, 256, 512])
def test_feature_distance_vs_fp64(M, C):
    """slr_feature_cos_distance on constructed channel-blocked features against its float64 definition (perceptual_f64's norm and
    1 - mean on relu(f)): signs (the kernel's own ReLU), pixels whose ReLU'd vector is all zero in one map or in both (the + 1e-10 of
    normalize_tensor: their term is exactly 0), f1 = f0, f1 = 3 f0, magnitudes 1e-3 and 1e3, permuted channels; 1 to 14400 pixels
    (one workgroup, exactly one, one pixel into the second, 57 partial sums), three images and one alone (bit-exact).
    Bound: 6 E_ref + 1e-6, E_ref = the same definition in torch float32 on the CPU against float64, over the family of this C.  One missed
    pixel at 45 x 80 moves the result by up to 2.8e-4.

    Measured on an MI355X (max e_gpu | E_ref | ratio): C = 8: 1.19e-7 | 1.19e-7 | 1.0, 64: 2.38e-7 | 1.79e-7 | 1.3, 128: 1.79e-7 | 6.31e-8 | 2.8,
    256: 1.79e-7 | 1.19e-7 | 1.5, 512: 5.96e-7 | 1.19e-7 | 5.0 (one pixel, f1 = 3 f0: within the bound through its 1e-6 term)."""
    rows = []
    for H, W in FD_SHAPES:
        fam, band = MF.feature_pairs(3, C, H, W)
        for name, (f0, f1) in fam.items():
            b0, b1 = MF.to_blocked(f0).cuda(), MF.to_blocked(f1).cuda()
            got = M.feature_distance(b0, b1)
            assert torch.equal(got, M.feature_distance(b0, b1)), (name, H, W)
            assert torch.equal(got[1:2], M.feature_distance(b0[1:2].contiguous(), b1[1:2].contiguous())), (name, H, W)
            f64, f32 = MF.feature_distance_def(f0, f1, torch.float64), MF.feature_distance_def(f0, f1, torch.float32)
            rows.append((H, W, name, float((got.cpu().double() - f64).abs().max()), float((f32 - f64).abs().max())))
            if name == "dead_in_both":                                   # f0 = f1 > 0 outside the band: the distance is the band's share
                pos = torch.where(band, f0, f0.abs() + 0.1)
                d = M.feature_distance(MF.to_blocked(pos).cuda(), MF.to_blocked(pos).cuda()).cpu().double()
                share = float(band.sum()) / (H * W)
                assert float((d - share).abs().max()) <= 1e-6, (H, W, d.tolist(), share)      # cos = s / (sqrt(s) + eps)^2: a few roundings from 1
    E_ref = max(r[4] for r in rows)
    e_max = max(r[3] for r in rows)
    for H, W, name, e_gpu, e_ref in rows:
        print(f"[fd C={C} {H}x{W}] {name:18s} e_gpu {e_gpu:.2e} e_ref {e_ref:.2e}")
    print(f"[fd C={C}] max e_gpu {e_max:.2e}  E_ref {E_ref:.2e}  ratio {e_max / E_ref:.3f}")
    assert E_ref < 1e-5, E_ref                                           # (a broken yardstick must not widen the bound)
    bad = [r for r in rows if not r[3] <= 6 * E_ref + 1e-6]
    assert not bad, bad


@pytest.mark.parametrize("hw", [(1, 1), (3, 85), (1, 257), (64, 96)])
@pytest.mark.parametrize("n", [1, 3])
def test_vgg_prep_vs_fp64(hw, n):
    """slr_vgg_prep as PerceptualVGG16.score calls it: uint8 [N,H,W,3] frames holding every level in every channel (where the size
    allows), floats in [0, 1] with from01 and in [-1, 1] without, against ((x * 2 - 1) - shift) / scale in float64.  Bound 1e-6 absolute:
    at most four fp32 roundings of magnitudes <= 1.2 divided by a scale >= 0.448 (4 * 2^-24 * 1.2 / 0.448 = 6.4e-7), plus the rounding of
    the constants; not a bound in ulps of the result, which passes through zero.  uint8 frames and the float tensor v / 255 give the same bits;
    the channels hold different values, so a wrong output layout cannot pass."""
    from slr_sfs_amd import _lib
    H, W = hw
    idx = np.arange(n * H * W).reshape(n, H, W, 1)
    u8 = ((idx * 7 + np.array([0, 85, 171]).reshape(1, 1, 1, 3) + 255 * (H * W == 1)) % 256).astype(np.uint8)
    if H * W >= 256:
        assert all(len(np.unique(u8[i, :, :, c])) == 256 for i in range(n) for c in range(3))

    def prep(t, is_u8, from01):
        out = torch.full((n, 3, H, W), float("nan"), device="cuda")
        _lib.call("slr_vgg_prep", out.device, t.cuda(), is_u8, from01, out, n, H, W)
        return out.cpu()

    got_u8 = prep(_t(u8), 1, 1)
    x64 = _t(u8).permute(0, 3, 1, 2).double() / 255.0
    assert float((got_u8.double() - MF.vgg_prep_f64(x64, True)).abs().max()) <= 1e-6
    f = MF.to_tensor(u8)
    assert torch.equal(prep(f, 0, 1), got_u8)
    r = np.random.default_rng(n * 1000 + H * W)
    f01 = _t(r.uniform(0, 1, (n, 3, H, W)).astype(np.float32))
    f01.view(-1)[:2] = torch.tensor([0.0, 1.0])[: f01.numel()]
    assert float((prep(f01, 0, 1).double() - MF.vgg_prep_f64(f01, True)).abs().max()) <= 1e-6
    f11 = f01 * 2 - 1
    assert float((prep(f11, 0, 0).double() - MF.vgg_prep_f64(f11, False)).abs().max()) <= 1e-6


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("hw", [(2, 2), (2, 3), (3, 2), (45, 81), (90, 160), (720, 1280)])
def test_relu_maxpool_vs_torch(M, hw, n, C):
    """slr_relu_maxpool2x2_b8 equals F.max_pool2d(F.relu(x), 2, 2) bit for bit (neither rounds): odd sizes (floor mode), the smallest
    ones, the 720 x 1280 of conv1_2's output, windows that are all negative (-> 0)."""
    H, W = hw
    r = np.random.default_rng(C * 100000 + H * W + n)
    x = _t(r.standard_normal((n, C, H, W)).astype(np.float32))
    x[:, :, : max(2, H // 3), : max(2, W // 2)] = -x[:, :, : max(2, H // 3), : max(2, W // 2)].abs() - 0.25     # whole windows negative
    out = M.relu_maxpool2x2(MF.to_blocked(x).cuda())
    want = torch.nn.functional.max_pool2d(torch.relu(x), 2, 2)
    assert out.shape == want.shape == (n, C, H // 2, W // 2)
    assert bool((want[:, :, 0, 0] == 0).all())
    assert torch.equal(MF.from_blocked(out.cpu()), want)


# ------------------------------------------------------------------ C. the Perceptual metric at the evaluation shape

def test_perceptual_720p_batch_of_four(M, vgg):
    """Four 720 x 1280 pairs in one batch, the shape evaluate_clip runs at (perceptual_batch: 8 images x 64 channels x 720 x 1280 x 4 B =
    1.76 GiB per activation tensor): every pair's total and five per-slice scores equal the pair run alone bit for bit, and pairs 0
    (textured) and 2 (half saturated) are within 1e-4 relative of the float64 VGG16, slice by slice and in total.
    Measured on an MI355X, worst slice | total: pair 0: 2.4e-7 (relu4_3) | 5.5e-8; pair 2: 6.6e-5 (relu5_3), 2.1e-5 (relu4_3) | 3.2e-7."""
    H, W = 720, 1280
    assert M.perceptual_batch(H, W) == 4
    a_u8, b_u8 = MF.image_pair(H, W, n=4, tag="p720")
    a_u8[2], b_u8[2] = MF.hard_pairs(H, W)["half_saturated"]
    x, y = _t(a_u8).cuda(), _t(b_u8).cuda()
    total, per = vgg.score(x, y, True, retPerLayer=True)
    total, per = total.cpu(), torch.stack(per).cpu()                      # [4], [5, 4]
    assert bool(torch.isfinite(per).all())
    for i in range(4):
        t1, p1 = vgg.score(x[i:i + 1], y[i:i + 1], True, retPerLayer=True)
        assert torch.equal(t1.cpu(), total[i:i + 1]), i
        assert torch.equal(torch.stack(p1).cpu(), per[:, i:i + 1]), i
    del x, y
    torch.cuda.empty_cache()
    feats = MF.vgg16_features(dtype=torch.float64)
    for i in (0, 2):
        want, want_per = MF.perceptual_f64(MF.to_tensor(a_u8[i:i + 1]), MF.to_tensor(b_u8[i:i + 1]), per_layer=True, features=feats)
        want_per = torch.stack(want_per)[:, 0]
        rel = ((per[:, i].double() - want_per) / want_per).abs()
        print(f"[perceptual 720p pair {i}] per slice {want_per.tolist()} rel err {rel.tolist()} total rel "
              f"{abs(float(total[i]) - float(want)) / float(want):.2e}")
        np.testing.assert_allclose(per[:, i].numpy(), want_per.numpy(), rtol=1e-4)
        np.testing.assert_allclose(total[i].numpy(), want[0].numpy(), rtol=1e-4)


# ------------------------------------------------------------------ D. evaluate_clip across chunk boundaries

@pytest.mark.parametrize("form", ["uint8", "float"])
def test_evaluate_clip_chunks_and_masks(M, vgg, form):
    """A 7-frame 48 x 64 clip in Perceptual chunks of 3 + 3 + 1, of 1 and in one piece: the same bits, equal to the per-frame calls;
    with a [1,1,h,w] and a [7,1,h,w] mask PSNR / SSIM are the masked functions and Perceptual does not change."""
    n, H, W = 7, 48, 64
    a_u8, b_u8 = MF.image_pair(H, W, n=n, tag="clip7")
    pred, gt = (_t(a_u8).cuda(), _t(b_u8).cuda()) if form == "uint8" else (MF.to_tensor(a_u8).cuda(), MF.to_tensor(b_u8).cuda())
    assert M.perceptual_batch(H, W) > n
    res = {b: M.evaluate_clip(pred, gt, vgg, batch=b) for b in (3, 1, None)}
    for b in (1, None):
        assert list(res[b]) == ["PSNR", "SSIM", "Perceptual"]
        for k in res[3]:
            assert res[b][k].shape == (n,) and torch.equal(res[b][k], res[3][k]), (b, k)
    for i in range(n):
        sm = M.ssim_mse(pred[i:i + 1], gt[i:i + 1])
        assert torch.equal(sm[:, 0], res[3]["SSIM"][i:i + 1]) and torch.equal(M.psnr_from_mse(sm[:, 1]), res[3]["PSNR"][i:i + 1]), i
        assert torch.equal(M.perceptual_sim(pred[i:i + 1], gt[i:i + 1], vgg), res[3]["Perceptual"][i:i + 1]), i
    x, y = MF.to_tensor(a_u8), MF.to_tensor(b_u8)
    np.testing.assert_allclose(res[3]["SSIM"].cpu().numpy(), MF.ssim_f64(x, y, 11, None, False).numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(res[3]["PSNR"].cpu().numpy(), MF.psnr_f64(x, y).numpy(), rtol=0, atol=1e-4)
    for mn in (1, n):
        mask = _t(MF.mask_for(H, W, n=mn, tag="clip7")).cuda()
        r = M.evaluate_clip(pred, gt, vgg, mask=mask, batch=3)
        assert torch.equal(r["PSNR"], M.psnr(pred, gt, mask)) and torch.equal(r["SSIM"], M.ssim_metric(pred, gt, mask))
        assert torch.equal(r["Perceptual"], res[3]["Perceptual"])
        np.testing.assert_allclose(r["SSIM"].cpu().numpy(), MF.ssim_f64(x, y, 11, mask.cpu()).numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(r["PSNR"].cpu().numpy(), MF.psnr_f64(x, y, mask.cpu()).numpy(), rtol=0, atol=1e-4)
        assert not torch.equal(r["SSIM"], res[3]["SSIM"])
    assert list(M.evaluate_clip(pred, gt)) == ["PSNR", "SSIM"]
