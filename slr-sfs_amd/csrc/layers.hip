// layers.hip -- the head of the two-layer model (models/animating_softmax_splating_2layers_alpha_seperate.py), ABI 24: what lies between
// the networks' raw outputs and the loss dictionary.
//   * the composite of the fluid and the background layer under their alphas (:372, :598, :608, :616-617, :652, :775-789) and its backward,
//   * the alpha losses (:420-421, :619-621, :658-666, :694-699, :727-729, :757-765): the (reweighted) alpha MSE against the rock mask, the
//     alpha total variation, the two alpha-decoder consistency losses, and their backward -- the TV as a five-point stencil,
//   * (ABI 25) the alpha-0 blending weight of train_alpha_finetuneBG_finetuneFluid_v1.sh: c0 with a gradient, and the two region losses
//     on it (:741-755), and their backward.
// All planes contiguous NCHW fp32.  Nothing here synchronises; there are no atomics: sums are per-workgroup partial sums in double
// (slr_reduce.hpp), added by a second launch in a fixed order, so every result has the same bits from run to run.  Every operation on an
// element is the fp32 one torch would do, products with masks included (0 * NaN = NaN); sign(0) = sign(NaN) = 0 (torch.sign).
// A thread owns four consecutive pixels of the flattened [N, H W] index: 16-byte accesses where four pixels never straddle a plane or a
// row and the planes start aligned (H W % 4 == 0 for the composite and the blending weight, W % 4 == 0 for the losses), scalar accesses elsewhere.
#include "slr_common.hpp"
#include "slr_reduce.hpp"

namespace slr {

constexpr int LY_THREADS = 128;                          // 512 pixels a workgroup: [2,.,256,256] is 256 workgroups, one per CU
constexpr int LY_PER_BLOCK = LY_THREADS * 4;
constexpr int LY_SUMS = 11;                              // partial sums of alpha_losses_forward_kernel
constexpr float LY_EPS = 1e-8f;

__device__ __forceinline__ float ly_sign(float d) { return (float)(d > 0.0f) - (float)(d < 0.0f); }     // torch.sign: 0 at 0 and at NaN
__device__ __forceinline__ float ly_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float ly_clamp_eps(float s) { return s < LY_EPS ? LY_EPS : s; }               // torch.clamp(min=1e-8): a NaN stays

// Elements off[0] .. off[0] + 3 in one 16-byte access when vec, else the first cnt of off[e] one by one (the others read as 0).
__device__ __forceinline__ void ld4(const float *__restrict__ p, const long long (&off)[4], bool vec, int cnt, float (&o)[4]) {
    if (vec) {
        const float4 v = *(const float4 *)(p + off[0]);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = e < cnt ? p[off[e]] : 0.0f;
    }
}

__device__ __forceinline__ void st4(float *__restrict__ p, const long long (&off)[4], bool vec, int cnt, const float (&o)[4]) {
    if (vec) *(float4 *)(p + off[0]) = make_float4(o[0], o[1], o[2], o[3]);
    else
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) p[off[e]] = o[e];
}

// The thread's four pixels: pix[e] = e0 + e of the flattened [N, HW] index (pixels past the end repeat e0), n[e] its sample.
struct Quad {
    long long pix[4], n[4];
    int cnt;
};

__device__ __forceinline__ bool ly_quad(Quad &q, long long total, long long HW) {
    const long long e0 = ((long long)blockIdx.x * LY_THREADS + threadIdx.x) * 4;
    const long long left = total - e0;
    q.cnt = left >= 4 ? 4 : left > 0 ? (int)left : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        q.pix[e] = e < q.cnt ? e0 + e : (q.cnt ? e0 : 0);
        q.n[e] = q.pix[e] / HW;
    }
    return q.cnt > 0;
}

// ------------------------------------------------------------------ the composite
// F = tanh(fr), B = tanh(br), af = sigmoid(fa), ab = sigmoid(ba), n = max(af + ab, 1e-8):  pred = (af F + ab B) / n,  ca = af / n.
__global__ __launch_bounds__(LY_THREADS) void layer_composite_forward_kernel(const float *__restrict__ fr, const float *__restrict__ br,
                                                                             const float *__restrict__ fa, const float *__restrict__ ba,
                                                                             float *__restrict__ pred, float *__restrict__ fl,
                                                                             float *__restrict__ bg, float *__restrict__ ca,
                                                                             long long total, long long HW, int vec_ok) {
    Quad q;
    if (!ly_quad(q, total, HW)) return;
    const bool vec = vec_ok && q.cnt == 4;
    long long o1[4], o3[4];                              // offsets in a one-channel plane and of channel 0 in a three-channel tensor
#pragma unroll
    for (int e = 0; e < 4; ++e) { o1[e] = q.pix[e]; o3[e] = q.pix[e] + 2 * q.n[e] * HW; }
    float xa[4], xb[4], af[4], ab[4], nn[4], o[4];
    ld4(fa, o1, vec, q.cnt, xa);
    ld4(ba, o1, vec, q.cnt, xb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        af[e] = ly_sigmoid(xa[e]);
        ab[e] = ly_sigmoid(xb[e]);
        nn[e] = ly_clamp_eps(af[e] + ab[e]);
        o[e] = af[e] / nn[e];
    }
    st4(ca, o1, vec, q.cnt, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float F[4], B[4];
        ld4(fr, o3, vec, q.cnt, F);
        ld4(br, o3, vec, q.cnt, B);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            F[e] = tanhf(F[e]);
            B[e] = tanhf(B[e]);
            o[e] = (af[e] * F[e] + ab[e] * B[e]) / nn[e];
        }
        st4(fl, o3, vec, q.cnt, F);
        st4(bg, o3, vec, q.cnt, B);
        st4(pred, o3, vec, q.cnt, o);
#pragma unroll
        for (int e = 0; e < 4; ++e) o3[e] += HW;
    }
}

// From gp = d pred, gf = d F, gb = d B (each may be NULL: absent), the chain as autograd walks it:
//   g_num = gp / n;  g_n = sum_c -gp (af F + ab B) / n^2, passed on to af + ab only where af + ab >= 1e-8 (the clamp's backward)
//   d fr = (g_num af + gf) (1 - F^2);  d br = (g_num ab + gb) (1 - B^2);  d fa = (sum_c g_num F + g_s) (1 - af) af;  d ba likewise.
// Outputs may be NULL (not wanted).
__global__ __launch_bounds__(LY_THREADS) void layer_composite_backward_kernel(const float *__restrict__ fr, const float *__restrict__ br,
                                                                              const float *__restrict__ fa, const float *__restrict__ ba,
                                                                              const float *__restrict__ gp, const float *__restrict__ gf,
                                                                              const float *__restrict__ gb, float *__restrict__ dfr,
                                                                              float *__restrict__ dbr, float *__restrict__ dfa,
                                                                              float *__restrict__ dba, long long total, long long HW,
                                                                              int vec_ok) {
    Quad q;
    if (!ly_quad(q, total, HW)) return;
    const bool vec = vec_ok && q.cnt == 4;
    long long o1[4], o3[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { o1[e] = q.pix[e]; o3[e] = q.pix[e] + 2 * q.n[e] * HW; }
    float xa[4], xb[4], af[4], ab[4], s[4], nn[4], gaf[4], gab[4], gn[4];
    ld4(fa, o1, vec, q.cnt, xa);
    ld4(ba, o1, vec, q.cnt, xb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        af[e] = ly_sigmoid(xa[e]);
        ab[e] = ly_sigmoid(xb[e]);
        s[e] = af[e] + ab[e];
        nn[e] = ly_clamp_eps(s[e]);
        gaf[e] = gab[e] = gn[e] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float F[4], B[4], P[4] = {0.0f, 0.0f, 0.0f, 0.0f}, GF[4] = {0.0f, 0.0f, 0.0f, 0.0f}, GB[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        ld4(fr, o3, vec, q.cnt, F);
        ld4(br, o3, vec, q.cnt, B);
        if (gp) ld4(gp, o3, vec, q.cnt, P);
        if (gf) ld4(gf, o3, vec, q.cnt, GF);
        if (gb) ld4(gb, o3, vec, q.cnt, GB);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            F[e] = tanhf(F[e]);
            B[e] = tanhf(B[e]);
            if (gp) {
                const float num = af[e] * F[e] + ab[e] * B[e];
                const float gnum = P[e] / nn[e];
                gn[e] += -P[e] * num / (nn[e] * nn[e]);
                gaf[e] += gnum * F[e];
                gab[e] += gnum * B[e];
                GF[e] += gnum * af[e];
                GB[e] += gnum * ab[e];
            }
            F[e] = GF[e] * (1.0f - F[e] * F[e]);
            B[e] = GB[e] * (1.0f - B[e] * B[e]);
        }
        if (dfr) st4(dfr, o3, vec, q.cnt, F);
        if (dbr) st4(dbr, o3, vec, q.cnt, B);
#pragma unroll
        for (int e = 0; e < 4; ++e) o3[e] += HW;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gs = s[e] >= LY_EPS ? gn[e] : 0.0f;
        xa[e] = (gaf[e] + gs) * (1.0f - af[e]) * af[e];
        xb[e] = (gab[e] + gs) * (1.0f - ab[e]) * ab[e];
    }
    if (dfa) st4(dfa, o1, vec, q.cnt, xa);
    if (dba) st4(dba, o1, vec, q.cnt, xb);
}

// ------------------------------------------------------------------ the alpha losses
// What both passes need of a pixel: its coordinates and its offsets in a one-channel plane and in a_start [N,2,H,W] (channel 0).
struct AlphaPix {
    long long o1, o2;
    int y, x;
};

__device__ __forceinline__ AlphaPix alpha_pix(long long pix, long long n, long long HW, int W) {
    AlphaPix p;
    const long long r = pix - n * HW;
    p.o1 = pix;
    p.o2 = pix + n * HW;
    p.y = (int)(r / W);
    p.x = (int)(r - (long long)p.y * W);
    return p;
}

// The file's SmoothL1Loss (:63-65) of d = input - target: |d| + 0.1 (2 sigmoid(5 |d|) - 1).
__device__ __forceinline__ float ly_smooth_l1(float d) {
    const float t = fabsf(d);
    return t + 0.1f * (2.0f * ly_sigmoid(5.0f * t) - 1.0f);
}

// Partial sums, part[block * LY_SUMS + k]:  0 sum r m err, 1 sum r m, 2 sum (1 - r) m err, 3 sum (1 - r) m, 4 sum err,
//   5 / 6 the TV sums of a1 along x / y, 7 / 8 those of sigmoid(a0), 9 sum S, 10 sum S m.
__global__ __launch_bounds__(LY_THREADS) void alpha_losses_forward_kernel(const float *__restrict__ a, const float *__restrict__ rock,
                                                                          const float *__restrict__ sma, const float *__restrict__ warped,
                                                                          const float *__restrict__ norm, const float *__restrict__ far,
                                                                          float *__restrict__ gt_out, float *__restrict__ c0_out,
                                                                          double *__restrict__ part, long long total, long long HW, int H,
                                                                          int W, int vec_ok) {
    __shared__ double red[LY_SUMS][LY_THREADS / 64];
    double v[LY_SUMS];
#pragma unroll
    for (int k = 0; k < LY_SUMS; ++k) v[k] = 0.0;
    Quad q;
    if (ly_quad(q, total, HW)) {
        const bool vec = vec_ok && q.cnt == 4;           // (W % 4 == 0: the four pixels lie in one row)
        AlphaPix p[4];
        long long o1[4], o2[4], o2b[4], od[4], odb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            p[e] = alpha_pix(q.pix[e], q.n[e], HW, W);
            o1[e] = p[e].o1; o2[e] = p[e].o2; o2b[e] = p[e].o2 + HW;
            const bool below = p[e].y + 1 < H;           // (no row below: re-read the pixel itself, a difference of 0 that is not counted)
            od[e] = below ? o2[e] + W : o2[e];
            odb[e] = od[e] + HW;
        }
        float a0[4], a1[4], d0[4], d1[4], r[4], sm[4], wa[4], nm[4], f[4], gt[4], c0[4];
        ld4(a, o2, vec, q.cnt, a0);
        ld4(a, o2b, vec, q.cnt, a1);
        ld4(a, od, vec, q.cnt, d0);
        ld4(a, odb, vec, q.cnt, d1);
        ld4(rock, o1, vec, q.cnt, r);
        ld4(sma, o1, vec, q.cnt, sm);
        ld4(warped, o1, vec, q.cnt, wa);
        ld4(norm, o1, vec, q.cnt, nm);
        ld4(far, o1, vec, q.cnt, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool live = e < q.cnt, right = p[e].x + 1 < W, below = p[e].y + 1 < H;
            const float m = 1.0f - sm[e];
            const float sf = ly_sigmoid(a1[e]), sb = ly_sigmoid(a0[e]);
            const float nn = ly_clamp_eps(sf + sb);
            c0[e] = sf / nn;
            gt[e] = r[e] * m * 0.25f + (1.0f - r[e]) * m + sm[e] * 0.5f;
            const float ee = c0[e] * m - gt[e] * m, err = ee * ee;
            const float pos = r[e] * m, neg = (1.0f - r[e]) * m;
            float r0 = 0.0f, r1 = 0.0f;                  // the right neighbour: the next element of the vector, else a load
            if (vec && e < 3) { r0 = a0[e < 3 ? e + 1 : 3]; r1 = a1[e < 3 ? e + 1 : 3]; }
            else if (live && right) { r0 = a[o2[e] + 1]; r1 = a[o2b[e] + 1]; }
            const float k = nm[e] > LY_EPS ? 1.0f : 0.0f;
            const float S = ly_smooth_l1(wa[e] * k - f[e] * k);
            if (live) {
                v[0] += (double)(pos * err); v[1] += (double)pos; v[2] += (double)(neg * err); v[3] += (double)neg; v[4] += (double)err;
                if (right) { v[5] += (double)fabsf(a1[e] - r1); v[7] += (double)fabsf(sb - ly_sigmoid(r0)); }
                if (below) { v[6] += (double)fabsf(a1[e] - d1[e]); v[8] += (double)fabsf(sb - ly_sigmoid(d0[e])); }
                v[9] += (double)S; v[10] += (double)(S * m);
            }
        }
        st4(gt_out, o1, vec, q.cnt, gt);
        st4(c0_out, o1, vec, q.cnt, c0);
    }
    block_sum<LY_SUMS, LY_THREADS / 64>(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < LY_SUMS; ++k) part[(long long)blockIdx.x * LY_SUMS + k] = v[k];
}

// The workgroups' partial sums in a fixed order -> out[8]: 0 AlphaMSEloss, 1 AlphaTV, 2 Alpha Decoder Consistency Loss, 3 its moving-region
// form, 4 / 5 the factors 0.5 / (1 + sum r m) and 0.5 / (1 + sum (1 - r) m) the backward multiplies with, 6 / 7 zero.
__global__ __launch_bounds__(256) void alpha_losses_finish_kernel(const double *__restrict__ part, float *__restrict__ out, int blocks,
                                                                  int reweight, double cnt, double cnt_x, double cnt_y) {
    __shared__ double red[LY_SUMS][4];
    double v[LY_SUMS];
#pragma unroll
    for (int k = 0; k < LY_SUMS; ++k) v[k] = 0.0;
    for (int t = threadIdx.x; t < blocks; t += 256)
#pragma unroll
        for (int k = 0; k < LY_SUMS; ++k) v[k] += part[(long long)t * LY_SUMS + k];
    block_sum<LY_SUMS, 4>(v, red);
    if (threadIdx.x == 0) {
        const double kpos = 0.5 / (1.0 + v[1]), kneg = 0.5 / (1.0 + v[3]);
        out[0] = (float)(reweight ? v[0] * kpos + v[2] * kneg : v[4] / cnt);
        out[1] = (float)((v[5] / cnt_x + v[6] / cnt_y) + (v[7] / cnt_x + v[8] / cnt_y));
        out[2] = (float)(v[9] / cnt);
        out[3] = (float)(v[10] / cnt);
        out[4] = (float)kpos;
        out[5] = (float)kneg;
        out[6] = out[7] = 0.0f;
    }
}

// The TV gradient at a pixel of value c with neighbours l, r (along x) and u, d (along y), those that exist:
//   kx (sign(c - r) - sign(l - c)) + ky (sign(c - d) - sign(u - c)).
__device__ __forceinline__ float tv_grad(float c, float l, float r, float u, float d, bool hl, bool hr, bool hu, bool hd, float kx, float ky) {
    const float gx = (hr ? ly_sign(c - r) : 0.0f) - (hl ? ly_sign(l - c) : 0.0f);
    const float gy = (hd ? ly_sign(c - d) : 0.0f) - (hu ? ly_sign(u - c) : 0.0f);
    return gx * kx + gy * ky;
}

// d a_start [N,2,H,W] and d fluid_alpha_raw [N,1,H,W] from g[4], the gradients reaching the four loss values (device), and `losses`, the
// forward's vector (its factors 4 / 5).  Either output may be NULL.
__global__ __launch_bounds__(LY_THREADS) void alpha_losses_backward_kernel(const float *__restrict__ a, const float *__restrict__ rock,
                                                                           const float *__restrict__ sma, const float *__restrict__ warped,
                                                                           const float *__restrict__ norm, const float *__restrict__ far,
                                                                           const float *__restrict__ losses, const float *__restrict__ g,
                                                                           float *__restrict__ da, float *__restrict__ dfar,
                                                                           long long total, long long HW, int H, int W, int reweight,
                                                                           float inv_cnt, float inv_x, float inv_y, int vec_ok) {
    Quad q;
    if (!ly_quad(q, total, HW)) return;
    const bool vec = vec_ok && q.cnt == 4;
    const float g_mse = g[0], g_tv = g[1], g_adc = g[2], g_mr = g[3];
    const float kpos = g_mse * losses[4], kneg = g_mse * losses[5], kplain = g_mse * inv_cnt;
    const float kx = g_tv * inv_x, ky = g_tv * inv_y, k_adc = g_adc * inv_cnt, k_mr = g_mr * inv_cnt;
    AlphaPix p[4];
    long long o1[4], o2[4], o2b[4], ou[4], oub[4], od[4], odb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        p[e] = alpha_pix(q.pix[e], q.n[e], HW, W);
        o1[e] = p[e].o1; o2[e] = p[e].o2; o2b[e] = p[e].o2 + HW;
        ou[e] = p[e].y > 0 ? o2[e] - W : o2[e];          // (no such row: the pixel itself, not used)
        od[e] = p[e].y + 1 < H ? o2[e] + W : o2[e];
        oub[e] = ou[e] + HW; odb[e] = od[e] + HW;
    }
    float a0[4], a1[4], u0[4], u1[4], d0[4], d1[4], r[4], sm[4], o0[4], ob[4];
    ld4(a, o2, vec, q.cnt, a0);
    ld4(a, o2b, vec, q.cnt, a1);
    if (da) {
        ld4(a, ou, vec, q.cnt, u0);
        ld4(a, oub, vec, q.cnt, u1);
        ld4(a, od, vec, q.cnt, d0);
        ld4(a, odb, vec, q.cnt, d1);
        ld4(rock, o1, vec, q.cnt, r);
    }
    ld4(sma, o1, vec, q.cnt, sm);
    if (da) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool live = e < q.cnt, hl = p[e].x > 0, hr = p[e].x + 1 < W, hu = p[e].y > 0, hd = p[e].y + 1 < H;
            const float m = 1.0f - sm[e];
            const float sf = ly_sigmoid(a1[e]), sb = ly_sigmoid(a0[e]);
            const float s = sf + sb, nn = ly_clamp_eps(s);
            const float c0 = sf / nn;
            const float gt = r[e] * m * 0.25f + (1.0f - r[e]) * m + sm[e] * 0.5f;
            const float ee = c0 * m - gt * m;
            const float gerr = reweight ? kpos * (r[e] * m) + kneg * ((1.0f - r[e]) * m) : kplain;
            const float gc0 = gerr * (2.0f * ee) * m;
            const float gnn = -gc0 * sf / (nn * nn);
            const float gs = s >= LY_EPS ? gnn : 0.0f;
            const float gsf = gc0 / nn + gs, gsb = gs;
            float l0 = 0.0f, l1 = 0.0f, r0 = 0.0f, r1 = 0.0f;
            if (vec && e > 0) { l0 = a0[e > 0 ? e - 1 : 0]; l1 = a1[e > 0 ? e - 1 : 0]; }
            else if (live && hl) { l0 = a[o2[e] - 1]; l1 = a[o2b[e] - 1]; }
            if (vec && e < 3) { r0 = a0[e < 3 ? e + 1 : 3]; r1 = a1[e < 3 ? e + 1 : 3]; }
            else if (live && hr) { r0 = a[o2[e] + 1]; r1 = a[o2b[e] + 1]; }
            const float tv1 = tv_grad(a1[e], l1, r1, u1[e], d1[e], hl, hr, hu, hd, kx, ky);
            const float tvb = tv_grad(sb, ly_sigmoid(l0), ly_sigmoid(r0), ly_sigmoid(u0[e]), ly_sigmoid(d0[e]), hl, hr, hu, hd, kx, ky);
            ob[e] = gsf * (1.0f - sf) * sf + tv1;
            o0[e] = (gsb + tvb) * (1.0f - sb) * sb;
        }
        st4(da, o2, vec, q.cnt, o0);
        st4(da, o2b, vec, q.cnt, ob);
    }
    if (dfar) {
        float wa[4], nm[4], f[4];
        ld4(warped, o1, vec, q.cnt, wa);
        ld4(norm, o1, vec, q.cnt, nm);
        ld4(far, o1, vec, q.cnt, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float m = 1.0f - sm[e];
            const float k = nm[e] > LY_EPS ? 1.0f : 0.0f;
            const float d = wa[e] * k - f[e] * k, t = fabsf(d);
            const float sg = ly_sigmoid(5.0f * t);
            const float gS = k_adc + k_mr * m;           // d S = gS;  d t = gS + gS 0.1 * 2 * 5 sg (1 - sg);  d d = d t sign(d);  d f = -d d k
            const float gt_ = gS + gS * 0.2f * (1.0f - sg) * sg * 5.0f;
            f[e] = -(gt_ * ly_sign(d)) * k;
        }
        st4(dfar, o1, vec, q.cnt, f);
    }
}

// ------------------------------------------------------------------ the alpha-0 blending weight (ABI 25)
// c0 = sf / max(sf + sb, 1e-8) of the START image (:420-421) as the plane train_alpha_finetuneBG_finetuneFluid_v1.sh splats the alpha logit
// with (:483-484, :538-539), and the two region losses on it (:741-755), S the file's SmoothL1Loss:
//   Fluid = mean S(c0 (1 - r) m - (1 - r) m),   Rock = mean S(c0 r m - target r m),   m = 1 - small_motion_alpha.
// Products in torch's order, left to right.  Partial sums, part[block * 2 + k]: 0 the fluid term, 1 the rock term.
constexpr int B0_SUMS = 2;

__global__ __launch_bounds__(LY_THREADS) void blend_alpha0_forward_kernel(const float *__restrict__ a, const float *__restrict__ rock,
                                                                          const float *__restrict__ sma, float *__restrict__ c0_out,
                                                                          double *__restrict__ part, float target, long long total,
                                                                          long long HW, int vec_ok) {
    __shared__ double red[B0_SUMS][LY_THREADS / 64];
    double v[B0_SUMS] = {0.0, 0.0};
    Quad q;
    if (ly_quad(q, total, HW)) {
        const bool vec = vec_ok && q.cnt == 4;           // (H W % 4 == 0: the four pixels lie in one sample)
        long long o1[4], o2[4], o2b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { o1[e] = q.pix[e]; o2[e] = q.pix[e] + q.n[e] * HW; o2b[e] = o2[e] + HW; }
        float a0[4], a1[4], r[4], sm[4], c0[4];
        ld4(a, o2, vec, q.cnt, a0);
        ld4(a, o2b, vec, q.cnt, a1);
        ld4(rock, o1, vec, q.cnt, r);
        ld4(sma, o1, vec, q.cnt, sm);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float m = 1.0f - sm[e], nr = 1.0f - r[e];
            const float sf = ly_sigmoid(a1[e]), sb = ly_sigmoid(a0[e]);
            c0[e] = sf / ly_clamp_eps(sf + sb);
            const float SF = ly_smooth_l1(c0[e] * nr * m - nr * m);
            const float SR = ly_smooth_l1(c0[e] * r[e] * m - target * r[e] * m);
            if (e < q.cnt) { v[0] += (double)SF; v[1] += (double)SR; }
        }
        st4(c0_out, o1, vec, q.cnt, c0);
    }
    block_sum<B0_SUMS, LY_THREADS / 64>(v, red);
    if (threadIdx.x == 0) {
        part[(long long)blockIdx.x * B0_SUMS] = v[0];
        part[(long long)blockIdx.x * B0_SUMS + 1] = v[1];
    }
}

// The workgroups' partial sums in a fixed order -> out[2]: 0 FluidRegionLoss, 1 RockRegionLoss.
__global__ __launch_bounds__(256) void blend_alpha0_finish_kernel(const double *__restrict__ part, float *__restrict__ out, int blocks,
                                                                  double cnt) {
    __shared__ double red[B0_SUMS][4];
    double v[B0_SUMS] = {0.0, 0.0};
    for (int t = threadIdx.x; t < blocks; t += 256) {
        v[0] += part[(long long)t * B0_SUMS];
        v[1] += part[(long long)t * B0_SUMS + 1];
    }
    block_sum<B0_SUMS, 4>(v, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(v[0] / cnt);
        out[1] = (float)(v[1] / cnt);
    }
}

// d S(d) / d d times g: g (1 + sigmoid(5 t) (1 - sigmoid(5 t))) sign(d), t = |d|, in the operations of alpha_losses_backward_kernel.
__device__ __forceinline__ float ly_smooth_l1_grad(float d, float g) {
    const float sg = ly_sigmoid(5.0f * fabsf(d));
    return (g + g * 0.2f * (1.0f - sg) * sg * 5.0f) * ly_sign(d);
}

// d a_start [N,2,H,W] from gc0 [N,1,H,W], the gradient reaching c0, and g[2], those reaching the two losses (device); either may be NULL
// (absent).  The chain is autograd's: what reaches max(sf + sb, 1e-8) passes on only where sf + sb >= 1e-8.
__global__ __launch_bounds__(LY_THREADS) void blend_alpha0_backward_kernel(const float *__restrict__ a, const float *__restrict__ rock,
                                                                           const float *__restrict__ sma, const float *__restrict__ gc0,
                                                                           const float *__restrict__ g, float *__restrict__ da,
                                                                           float target, float inv_cnt, long long total, long long HW,
                                                                           int vec_ok) {
    Quad q;
    if (!ly_quad(q, total, HW)) return;
    const bool vec = vec_ok && q.cnt == 4;
    const float kf = g ? g[0] * inv_cnt : 0.0f, kr = g ? g[1] * inv_cnt : 0.0f;
    long long o1[4], o2[4], o2b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { o1[e] = q.pix[e]; o2[e] = q.pix[e] + q.n[e] * HW; o2b[e] = o2[e] + HW; }
    float a0[4], a1[4], r[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sm[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    ld4(a, o2, vec, q.cnt, a0);
    ld4(a, o2b, vec, q.cnt, a1);
    if (g) {
        ld4(rock, o1, vec, q.cnt, r);
        ld4(sma, o1, vec, q.cnt, sm);
    }
    if (gc0) ld4(gc0, o1, vec, q.cnt, gc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float sf = ly_sigmoid(a1[e]), sb = ly_sigmoid(a0[e]);
        const float s = sf + sb, nn = ly_clamp_eps(s);
        float dc0 = gc[e];
        if (g) {
            const float m = 1.0f - sm[e], nr = 1.0f - r[e];
            const float c0 = sf / nn;
            dc0 += ly_smooth_l1_grad(c0 * nr * m - nr * m, kf) * m * nr;
            dc0 += ly_smooth_l1_grad(c0 * r[e] * m - target * r[e] * m, kr) * m * r[e];
        }
        const float gnn = -dc0 * sf / (nn * nn);
        const float gs = s >= LY_EPS ? gnn : 0.0f;
        a1[e] = (dc0 / nn + gs) * (1.0f - sf) * sf;
        a0[e] = gs * (1.0f - sb) * sb;
    }
    st4(da, o2, vec, q.cnt, a0);
    st4(da, o2b, vec, q.cnt, a1);
}

static long long ly_blocks(long long total) { return (total + LY_PER_BLOCK - 1) / LY_PER_BLOCK; }
static bool ly_sizes(int N, int H, int W, int min_hw) {
    return N > 0 && H >= min_hw && W >= min_hw && (long long)N * H * W < (1LL << 36);
}

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT int slr_layer_composite_forward(const float *fluid_raw, const float *bg_raw, const float *fluid_alpha_raw,
                                           const float *bg_alpha_raw, float *pred, float *fluid, float *bg, float *composite_alpha, int N,
                                           int H, int W, void *stream) {
    SLR_CHECK_ARG(fluid_raw && bg_raw && fluid_alpha_raw && bg_alpha_raw && pred && fluid && bg && composite_alpha, "null pointer");
    SLR_CHECK_ARG(ly_sizes(N, H, W, 1), "sizes");
    const long long HW = (long long)H * W, total = (long long)N * HW;
    const int vec = HW % 4 == 0 && !(((uintptr_t)fluid_raw | (uintptr_t)bg_raw | (uintptr_t)fluid_alpha_raw | (uintptr_t)bg_alpha_raw |
                                      (uintptr_t)pred | (uintptr_t)fluid | (uintptr_t)bg | (uintptr_t)composite_alpha) & 15);
    hipLaunchKernelGGL(layer_composite_forward_kernel, dim3((unsigned)ly_blocks(total)), dim3(LY_THREADS), 0, (hipStream_t)stream,
                       fluid_raw, bg_raw, fluid_alpha_raw, bg_alpha_raw, pred, fluid, bg, composite_alpha, total, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_layer_composite_backward(const float *fluid_raw, const float *bg_raw, const float *fluid_alpha_raw,
                                            const float *bg_alpha_raw, const float *g_pred, const float *g_fluid, const float *g_bg,
                                            float *d_fluid_raw, float *d_bg_raw, float *d_fluid_alpha_raw, float *d_bg_alpha_raw, int N,
                                            int H, int W, void *stream) {
    SLR_CHECK_ARG(fluid_raw && bg_raw && fluid_alpha_raw && bg_alpha_raw, "null pointer");
    SLR_CHECK_ARG(d_fluid_raw || d_bg_raw || d_fluid_alpha_raw || d_bg_alpha_raw, "null pointer: no gradient is wanted");
    SLR_CHECK_ARG(ly_sizes(N, H, W, 1), "sizes");
    const long long HW = (long long)H * W, total = (long long)N * HW;
    const int vec = HW % 4 == 0 && !(((uintptr_t)fluid_raw | (uintptr_t)bg_raw | (uintptr_t)fluid_alpha_raw | (uintptr_t)bg_alpha_raw |
                                      (uintptr_t)g_pred | (uintptr_t)g_fluid | (uintptr_t)g_bg | (uintptr_t)d_fluid_raw |
                                      (uintptr_t)d_bg_raw | (uintptr_t)d_fluid_alpha_raw | (uintptr_t)d_bg_alpha_raw) & 15);
    hipLaunchKernelGGL(layer_composite_backward_kernel, dim3((unsigned)ly_blocks(total)), dim3(LY_THREADS), 0, (hipStream_t)stream,
                       fluid_raw, bg_raw, fluid_alpha_raw, bg_alpha_raw, g_pred, g_fluid, g_bg, d_fluid_raw, d_bg_raw, d_fluid_alpha_raw,
                       d_bg_alpha_raw, total, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_alpha_losses_ws_bytes(int N, int H, int W) {
    if (!ly_sizes(N, H, W, 2)) return 0;
    return al256((size_t)ly_blocks((long long)N * H * W) * LY_SUMS * sizeof(double));
}

SLR_EXPORT int slr_alpha_losses_forward(const float *a_start, const float *mask_rock, const float *small_motion_alpha,
                                        const float *warped_alpha, const float *norm, const float *fluid_alpha_raw, float *losses,
                                        float *gt_alpha, float *c0, int reweight, int N, int H, int W, void *ws, size_t ws_bytes,
                                        void *stream) {
    SLR_CHECK_ARG(a_start && mask_rock && small_motion_alpha && warped_alpha && norm && fluid_alpha_raw && losses && gt_alpha && c0,
                  "null pointer");
    SLR_CHECK_ARG(ly_sizes(N, H, W, 2), "sizes (H, W >= 2: the total variation is a mean over nothing below)");
    if (!ws || ws_bytes < slr_alpha_losses_ws_bytes(N, H, W) || ((uintptr_t)ws & 7)) {
        slr::set_error("%s: workspace: slr_alpha_losses_ws_bytes(N, H, W) bytes, 8-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    const long long HW = (long long)H * W, total = (long long)N * HW, blocks = ly_blocks(total);
    const int vec = W % 4 == 0 && !(((uintptr_t)a_start | (uintptr_t)mask_rock | (uintptr_t)small_motion_alpha | (uintptr_t)warped_alpha |
                                     (uintptr_t)norm | (uintptr_t)fluid_alpha_raw | (uintptr_t)gt_alpha | (uintptr_t)c0) & 15);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(alpha_losses_forward_kernel, dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, a_start, mask_rock, small_motion_alpha,
                       warped_alpha, norm, fluid_alpha_raw, gt_alpha, c0, (double *)ws, total, HW, H, W, vec);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(alpha_losses_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)ws, losses, (int)blocks, reweight,
                       (double)total, (double)N * H * (W - 1), (double)N * (H - 1) * W);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_alpha_losses_backward(const float *a_start, const float *mask_rock, const float *small_motion_alpha,
                                         const float *warped_alpha, const float *norm, const float *fluid_alpha_raw, const float *losses,
                                         const float *g_losses, float *d_a_start, float *d_fluid_alpha_raw, int reweight, int N, int H,
                                         int W, void *stream) {
    SLR_CHECK_ARG(a_start && mask_rock && small_motion_alpha && warped_alpha && norm && fluid_alpha_raw && losses && g_losses,
                  "null pointer");
    SLR_CHECK_ARG(d_a_start || d_fluid_alpha_raw, "null pointer: no gradient is wanted");
    SLR_CHECK_ARG(ly_sizes(N, H, W, 2), "sizes (H, W >= 2)");
    const long long HW = (long long)H * W, total = (long long)N * HW;
    const int vec = W % 4 == 0 && !(((uintptr_t)a_start | (uintptr_t)mask_rock | (uintptr_t)small_motion_alpha | (uintptr_t)warped_alpha |
                                     (uintptr_t)norm | (uintptr_t)fluid_alpha_raw | (uintptr_t)d_a_start | (uintptr_t)d_fluid_alpha_raw) & 15);
    hipLaunchKernelGGL(alpha_losses_backward_kernel, dim3((unsigned)ly_blocks(total)), dim3(LY_THREADS), 0, (hipStream_t)stream, a_start,
                       mask_rock, small_motion_alpha, warped_alpha, norm, fluid_alpha_raw, losses, g_losses, d_a_start, d_fluid_alpha_raw,
                       total, HW, H, W, reweight, (float)(1.0 / (double)total), (float)(1.0 / ((double)N * H * (W - 1))),
                       (float)(1.0 / ((double)N * (H - 1) * W)), vec);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_blend_alpha0_ws_bytes(int N, int H, int W) {
    if (!ly_sizes(N, H, W, 1)) return 0;
    return al256((size_t)ly_blocks((long long)N * H * W) * B0_SUMS * sizeof(double));
}

SLR_EXPORT int slr_blend_alpha0_forward(const float *a_start, const float *mask_rock, const float *small_motion_alpha, float *c0,
                                        float *values, float rock_target, int N, int H, int W, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(a_start && mask_rock && small_motion_alpha && c0 && values, "null pointer");
    SLR_CHECK_ARG(ly_sizes(N, H, W, 1), "sizes");
    if (!ws || ws_bytes < slr_blend_alpha0_ws_bytes(N, H, W) || ((uintptr_t)ws & 7)) {
        slr::set_error("%s: workspace: slr_blend_alpha0_ws_bytes(N, H, W) bytes, 8-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    const long long HW = (long long)H * W, total = (long long)N * HW, blocks = ly_blocks(total);
    const int vec = HW % 4 == 0 && !(((uintptr_t)a_start | (uintptr_t)mask_rock | (uintptr_t)small_motion_alpha | (uintptr_t)c0) & 15);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(blend_alpha0_forward_kernel, dim3((unsigned)blocks), dim3(LY_THREADS), 0, st, a_start, mask_rock,
                       small_motion_alpha, c0, (double *)ws, rock_target, total, HW, vec);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(blend_alpha0_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)ws, values, (int)blocks, (double)total);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_blend_alpha0_backward(const float *a_start, const float *mask_rock, const float *small_motion_alpha, const float *g_c0,
                                         const float *g_values, float *d_a_start, float rock_target, int N, int H, int W, void *stream) {
    SLR_CHECK_ARG(a_start && mask_rock && small_motion_alpha && d_a_start, "null pointer");
    SLR_CHECK_ARG(g_c0 || g_values, "null pointer: no gradient arrives");
    SLR_CHECK_ARG(ly_sizes(N, H, W, 1), "sizes");
    const long long HW = (long long)H * W, total = (long long)N * HW;
    const int vec = HW % 4 == 0 && !(((uintptr_t)a_start | (uintptr_t)mask_rock | (uintptr_t)small_motion_alpha | (uintptr_t)g_c0 |
                                      (uintptr_t)d_a_start) & 15);
    hipLaunchKernelGGL(blend_alpha0_backward_kernel, dim3((unsigned)ly_blocks(total)), dim3(LY_THREADS), 0, (hipStream_t)stream, a_start,
                       mask_rock, small_motion_alpha, g_c0, g_values, d_a_start, rock_target, (float)(1.0 / (double)total), total, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}
