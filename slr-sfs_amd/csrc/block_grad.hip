// block_grad.hip -- what the decoder block needs to learn beyond its 3x3 convolutions (ABI 16): ResNet_Block_Pconv2 in training mode
// (models/layers/blocks.py:218-248) with the noise-conditioned partial batch-norm of models/layers/normalization.py:19-52, 256-354.
// The batch-norm kernels are one family for both mask kinds: the channel-uniform plane mask of every block (or none) and the per-element
// mask x != 0 of the decoder's first block (ABI 17, architectures.py:369; the rest of that block: csrc/decoder_grad.hip).
//   * batch statistics: per channel the sums of x and x^2 over ALL elements (normalization.py:325-329) in double, the count N H W,
//     sum(mask) + eps or, per channel, the integer number of nonzero elements + eps (normalization.py:319-335 with a [N,C,H,W] mask); mean
//     and var = m2 - m^2 formed in double and rounded once.
//   * training BN + ReLU + mask: a = relu(x * scale[n,c] - shift[n,c]) * mask with per-sample tables (gain and bias come from the noise).
//   * its backward: one reduction pass (s0 = sum gy, s1 = sum gy x per (n, c), gy = ga * mask * [y > 0], the gate recomputed from x),
//     a finalize kernel (dgain, dbias, the per-channel coefficients of the statistics' gradient) and one elementwise pass
//     dx = gy * scale + A + B * (x - mean) (+ addend).
//   * weight gradient of the 1x1 skip convolution: dW[co][ci] = sum_{n,p} G[n,co,p] X[n,ci,p] on v_mfma_f32_32x32x2_f32, the pixels cut
//     into slabs whose partial sums a second launch adds in double in slab order (the scheme of conv_grad.hip).
//   * the adjoints of slr_avgpool3x3s2 and slr_upsample_bilinear2x in gather form.
// Every tensor-sized kernel reads NCHW or channel-blocked ([N,C/8,H,W,8]) tensors; no atomics, every sum in a fixed order: the same inputs
// give the same bits.  Nothing here synchronises.
#include "slr_common.hpp"
#include "slr_reduce.hpp"
#include "block_items.hpp"

namespace slr {

// ------------------------------------------------------------------ the two mask kinds
// NZ = false: the channel-uniform plane `mask` [N,1,H,W], or none (NULL).  One count for all channels: N H W or sum(mask) + eps.
// NZ = true:  k = [x != 0] per element, recomputed from x by every kernel as the ReLU gate is.  One count per channel: nnz + eps, an integer
//             summed as one.  `mask` is NULL.
// The two reduction kernels give a thread the PPT items of their mask kind before the one workgroup sum, so that the float64 wave
// reductions are paid once per PPT items.
constexpr int BN_PPT_PLANE = 1, BN_PPT_NONZERO = 8;
constexpr int bn_ppt(bool nz) { return nz ? BN_PPT_NONZERO : BN_PPT_PLANE; }

// ------------------------------------------------------------------ 1. batch statistics
// part[(plane * GX + bx) * 2 KS + ...]: the workgroup's sums of x and x^2 per channel (KS = 8 channels blocked, 1 NCHW) in double -- over all
// elements, which with NZ is over the kept ones: the others are exact zeros.  What the count is made of goes to `cnt`:
//   plane:   mpart[n * GX + bx], the workgroup's sum of the mask in double, written by the workgroups of the first plane of every image;
//   nonzero: cpart[(plane * GX + bx) * KS + ...], its number of nonzero elements per channel.
template <bool B8, bool NZ, int PPT>
__global__ __launch_bounds__(BG_THREADS) void bn_stats_kernel(const float *__restrict__ x, const float *__restrict__ mask,
                                                             double *__restrict__ part, void *__restrict__ cnt, int planes, int HW,
                                                             int vec) {
    constexpr int K = BgItem<B8>::K, KS = B8 ? 8 : 1, NV = 2 * KS + (NZ ? 0 : 1);
    __shared__ double red[NV][BG_THREADS / 64];
    const int plane = blockIdx.y, n = plane / planes;    // (bg_item's own division)
    const bool msum = !NZ && mask && plane == n * planes;            // (uniform over the workgroup)
    double v[NV];
    unsigned c[KS];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
#pragma unroll
    for (int j = 0; j < KS; ++j) c[j] = 0;
    auto item = [&](int j) {
        const BgItem<B8> it = bg_item<B8, PPT>(planes, HW, vec, j);
        if (PPT > 1 && it.cnt == 0) return false;        // (a thread's only item stays: it reads as zeros, as it always did)
        float e[K];
        bg_load<B8>(it, x, e);                           // (elements past the plane read as 0: no sum and no count sees them)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double d = (double)e[k];
            v[B8 ? 2 * k : 0] += d;
            v[B8 ? 2 * k + 1 : 1] += d * d;
            if (NZ) c[B8 ? k : 0] += e[k] != 0.0f ? 1u : 0u;
        }
        if (msum) {
            float m[K];
            bg_mask<B8>(it, mask, m);
            if (B8) v[NV - 1] = j == 0 ? (double)m[0] : v[NV - 1] + (double)m[0];       // (the first item starts the sum: a -0.0 stays one)
            else
#pragma unroll
                for (int k = 0; k < K; ++k) v[NV - 1] += (double)m[k];
        }
        return true;
    };
    bg_items<PPT>(item);
    block_sum<NV, BG_THREADS / 64>(v, red);
    if constexpr (NZ) {
        __shared__ unsigned cred[KS][BG_THREADS / 64];
        block_count<KS, BG_THREADS / 64>(c, cred);
    }
    if (threadIdx.x == 0) {
        const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        double *p = part + wg * (2 * KS);
#pragma unroll
        for (int j = 0; j < 2 * KS; ++j) p[j] = v[j];
        if constexpr (NZ)
#pragma unroll
            for (int j = 0; j < KS; ++j) ((unsigned *)cnt)[wg * KS + j] = c[j];
        else if (msum) ((double *)cnt)[(size_t)n * gridDim.x + blockIdx.x] = v[NV - 1];
    }
}

// One workgroup per channel: the partial sums in the order (n, bx); mean, var and the count: nnz + eps of the channel (cpart; integers
// below 2^31, every sum of them exact in double), sum(mask) + eps (mpart) or N H W (neither), the last two written by channel 0 alone.
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const double *__restrict__ part, const double *__restrict__ mpart,
                                                             const unsigned *__restrict__ cpart, float *__restrict__ mean,
                                                             float *__restrict__ var, float *__restrict__ count, int N, int C, int GX,
                                                             int b8, float eps, int HW) {
    __shared__ double red[3][4];
    const int c = blockIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    unsigned long long nz = 0;
    for (int i = threadIdx.x; i < N * GX; i += 256) {
        const int n = i / GX, bx = i - n * GX;
        const double *q = bg_part(part, n, c, bx, C, GX, b8);
        v[0] += q[0];
        v[1] += q[1];
        if (cpart) nz += bg_cpart(cpart, n, c, bx, C, GX, b8);
        else if (mpart) v[2] += mpart[i];
    }
    if (cpart) v[2] = (double)nz;
    block_sum<3, 4>(v, red);
    if (threadIdx.x == 0) {
        const double cnt = cpart || mpart ? v[2] + (double)eps : (double)N * (double)HW;       // normalization.py:325 / torch.mean
        const double m = v[0] / cnt;
        mean[c] = (float)m;
        var[c] = (float)(v[1] / cnt - m * m);
        if (cpart) count[c] = (float)cnt;
        else if (c == 0) count[0] = (float)cnt;
    }
}

// ------------------------------------------------------------------ 2. training BN + ReLU + mask
// scale[n,c] = rsqrt(var[c] + eps) * gain[n,c], shift[n,c] = mean[c] * scale[n,c] - bias[n,c] (normalization.py:342-354), in fp32 with
// one rounding per operation.
__global__ __launch_bounds__(256) void bn_tables_kernel(const float *__restrict__ mean, const float *__restrict__ var,
                                                        const float *__restrict__ gain, const float *__restrict__ bias, float eps,
                                                        float *__restrict__ scale, float *__restrict__ shift, int NC, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    const int c = i % C;
    const float rs = 1.0f / sqrtf(var[c] + eps);
    const float sc = gain ? rs * gain[i] : rs;
    scale[i] = sc;
    const float sh = mean[c] * sc;
    shift[i] = bias ? sh - bias[i] : sh;
}

template <bool B8, bool NZ>
__global__ __launch_bounds__(BG_THREADS) void bn_train_forward_kernel(const float *__restrict__ x, const float *__restrict__ scale,
                                                                     const float *__restrict__ shift, const float *__restrict__ mask,
                                                                     float *__restrict__ a, int planes, int HW, int vec) {
    constexpr int K = BgItem<B8>::K;
    const BgItem<B8> it = bg_item<B8>(planes, HW, vec);
    if (it.cnt == 0) return;
    const int C = B8 ? planes * 8 : planes;
    float e[K], sc[K], sh[K], m[K];
    bg_load<B8>(it, x, e);
    bg_table<B8>(it, scale, it.n, C, sc);
    bg_table<B8>(it, shift, it.n, C, sh);
    if (!NZ) bg_mask<B8>(it, mask, m);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (NZ) m[k] = e[k] != 0.0f ? 1.0f : 0.0f;
        const float r = relu_nan(e[k] * sc[k] - sh[k]);  // (a NaN pre-activation stays one, as torch.relu's)
        e[k] = NZ || mask ? r * m[k] : r;
    }
    bg_store<B8>(it, a, e);
}

// ------------------------------------------------------------------ 3. its backward
// gy = ga * mask * [not x * scale - shift <= 0] at the item's elements (the forward's own fp32 expression decides the gate; a NaN
// pre-activation leaves it open, as torch's ReLU backward does).  Elements past the plane get 0: ga and x read as 0 there.
template <bool B8, bool NZ>
__device__ __forceinline__ void bg_gate(const BgItem<B8> &it, const float *__restrict__ ga, const float *__restrict__ mask,
                                        const float *__restrict__ scale, const float *__restrict__ shift, int C,
                                        const float (&e)[BgItem<B8>::K], float (&sc)[BgItem<B8>::K], float (&gy)[BgItem<B8>::K]) {
    constexpr int K = BgItem<B8>::K;
    float sh[K], m[K], g[K];
    bg_load<B8>(it, ga, g);
    bg_table<B8>(it, scale, it.n, C, sc);
    bg_table<B8>(it, shift, it.n, C, sh);
    if (!NZ) bg_mask<B8>(it, mask, m);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float y = e[k] * sc[k] - sh[k];
        // torch's ReLU backward closes on `<= 0` only: a NaN pre-activation passes the gradient.  The plane mask is a factor (a NaN
        // gradient under a zero mask stays NaN, as autograd's product); the nonzero mask is a second gate.
        if (NZ) gy[k] = (y <= 0.0f || e[k] == 0.0f) ? 0.0f : g[k];
        else gy[k] = y <= 0.0f ? 0.0f : mask ? g[k] * m[k] : g[k];
    }
}

// part[(plane * GX + bx) * 2 KS + ...] = the workgroup's s0 = sum gy and s1 = sum gy * x per channel, in double
template <bool B8, bool NZ, int PPT>
__global__ __launch_bounds__(BG_THREADS) void bn_backward_reduce_kernel(const float *__restrict__ x, const float *__restrict__ ga,
                                                                       const float *__restrict__ mask, const float *__restrict__ scale,
                                                                       const float *__restrict__ shift, double *__restrict__ part,
                                                                       int planes, int HW, int vec) {
    constexpr int K = BgItem<B8>::K, KS = B8 ? 8 : 1, NV = 2 * KS;
    __shared__ double red[NV][BG_THREADS / 64];
    const int C = B8 ? planes * 8 : planes;
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
    auto item = [&](int j) {
        const BgItem<B8> it = bg_item<B8, PPT>(planes, HW, vec, j);
        float e[K], sc[K], gy[K];
        bg_load<B8>(it, x, e);
        if (it.cnt) {
            bg_gate<B8, NZ>(it, ga, mask, scale, shift, C, e, sc, gy);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double d = B8 || k < it.cnt ? (double)gy[k] : 0.0;   // (gy past the plane is 0 as it is)
                v[B8 ? 2 * k : 0] += d;
                v[B8 ? 2 * k + 1 : 1] += d * (double)e[k];
            }
        }
        return it.cnt != 0;
    };
    bg_items<PPT>(item);
    block_sum<NV, BG_THREADS / 64>(v, red);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NV;
#pragma unroll
        for (int j = 0; j < NV; ++j) p[j] = v[j];
    }
}

// One workgroup per channel, the images in order: (s0, s1)[n] = the partial sums in bx order; dbias[n,c] = s0, dgain[n,c] = rs (s1 - m s0);
// P = sum_n gain s0, Q = sum_n gain s1, dv = -rs^3 (Q - m P) / 2 and, with the count cnt[c * cstride] (one for all channels: stride 0),
//     ab[c] = A = -rs P / cnt,  ab[C + c] = B = 2 dv / cnt     (dx = gy * scale + A + B (x - m); stored statistics: A = B = 0).
__global__ __launch_bounds__(256) void bn_backward_final_kernel(const double *__restrict__ part, const float *__restrict__ mean,
                                                                const float *__restrict__ var, const float *__restrict__ gain,
                                                                const float *__restrict__ cnt, int cstride, float eps,
                                                                float *__restrict__ dgain, float *__restrict__ dbias,
                                                                float *__restrict__ ab, int N, int C, int GX, int b8, int stored) {
    __shared__ double red[2][4];
    const int c = blockIdx.x;
    const double m = (double)mean[c], rs = 1.0 / sqrt((double)var[c] + (double)eps);
    double P = 0.0, Q = 0.0;
    for (int n = 0; n < N; ++n) {
        double v[2] = {0.0, 0.0};
        for (int bx = threadIdx.x; bx < GX; bx += 256) {
            const double *q = bg_part(part, n, c, bx, C, GX, b8);
            v[0] += q[0];
            v[1] += q[1];
        }
        block_sum<2, 4>(v, red);
        if (threadIdx.x == 0) {
            const double g = gain ? (double)gain[(size_t)n * C + c] : 1.0;
            if (dbias) dbias[(size_t)n * C + c] = (float)v[0];
            if (dgain) dgain[(size_t)n * C + c] = (float)(rs * (v[1] - m * v[0]));
            P += g * v[0];
            Q += g * v[1];
        }
        __syncthreads();                                 // (red is free again)
    }
    if (threadIdx.x == 0 && ab) {
        const double n_el = stored ? 1.0 : (double)cnt[(size_t)c * cstride];       // (stored statistics come without a count)
        const double dv = -0.5 * rs * rs * rs * (Q - m * P);
        ab[c] = stored ? 0.0f : (float)(-rs * P / n_el);
        ab[C + c] = stored ? 0.0f : (float)(2.0 * dv / n_el);
    }
}

// dx = gy * scale + (A + B * (x - mean)) (+ addend) at EVERY element, those the mask drops included: the statistics' gradient reaches them
// as the reference's autograd does.  ab = NULL: stored statistics, dx = gy * scale (+ addend)
template <bool B8, bool NZ>
__global__ __launch_bounds__(BG_THREADS) void bn_backward_dx_kernel(const float *__restrict__ x, const float *__restrict__ ga,
                                                                   const float *__restrict__ mask, const float *__restrict__ scale,
                                                                   const float *__restrict__ shift, const float *__restrict__ mean,
                                                                   const float *__restrict__ ab, const float *__restrict__ addend,
                                                                   float *__restrict__ dx, int planes, int HW, int vec) {
    constexpr int K = BgItem<B8>::K;
    const BgItem<B8> it = bg_item<B8>(planes, HW, vec);
    if (it.cnt == 0) return;
    const int C = B8 ? planes * 8 : planes;
    float e[K], sc[K], gy[K], o[K];
    bg_load<B8>(it, x, e);
    bg_gate<B8, NZ>(it, ga, mask, scale, shift, C, e, sc, gy);
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = gy[k] * sc[k];
    if (ab) {
        float A[K], B[K], mu[K];
        bg_table<B8>(it, ab, 0, C, A);
        bg_table<B8>(it, ab + C, 0, C, B);
        bg_table<B8>(it, mean, 0, C, mu);
#pragma unroll
        for (int k = 0; k < K; ++k) o[k] = o[k] + (A[k] + B[k] * (e[k] - mu[k]));
    }
    if (addend) {
        float ad[K];
        bg_load<B8>(it, addend, ad);
#pragma unroll
        for (int k = 0; k < K; ++k) o[k] = o[k] + ad[k];
    }
    bg_store<B8>(it, dx, o);
}

// ------------------------------------------------------------------ 4. weight gradient of the 1x1 convolution
// An implicit GEMM with M = Cout, N = Cin, K = N H W.  A workgroup of four waves owns 128 co x 64 ci (a wave: 32 co x 64 ci = two
// 32 x 32 accumulators) over a slab of the pixels, in chunks of 32 consecutive pixels of one image: at 64 -> 128 channels one workgroup
// column covers the whole weight, so X and G are read from HBM exactly once.  Staged tiles are [32-channel tile][pixel][channel] as in
// conv_grad.hip (pixel stride 32 blocked / 33 NCHW); the next chunk's loads are in flight while the matrix pipe works on this one.
constexpr int W1_P = 32, W1_CO = 128, W1_CI = 64;
constexpr int w1_stride(bool b8) { return b8 ? 32 : 33; }

// A thread's items are threadIdx.x + k * 256: the 8 channels of a pixel (blocked) or 4 consecutive pixels of a channel (NCHW).
template <bool B8, int TC> struct W1Regs {
    static constexpr int ITEMS = TC * W1_P / (B8 ? 8 : 4) / BG_THREADS;
    float4 v[B8 ? ITEMS * 2 : ITEMS];
};

template <bool B8, int TC>
__device__ __forceinline__ void w1_load(W1Regs<B8, TC> &rg, const float *__restrict__ src, int n, int C, int c0, int HW, int p0, int vec) {
    constexpr int ITEMS = W1Regs<B8, TC>::ITEMS;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int item = threadIdx.x + k * BG_THREADS;
        if constexpr (B8) {
            const int cg = item / W1_P, p = p0 + (item - cg * W1_P), G8 = C >> 3, g = (c0 >> 3) + cg;
            float4 a = zero, b = zero;
            if (p < HW && g < G8) {
                const float4 *q = (const float4 *)(src + (((size_t)n * G8 + g) * HW + p) * 8);
                a = q[0]; b = q[1];
            }
            rg.v[2 * k] = a; rg.v[2 * k + 1] = b;
        } else {
            const int c = item / (W1_P / 4), p = p0 + (item - c * (W1_P / 4)) * 4, ch = c0 + c;
            float4 a = zero;
            if (ch < C && p < HW) {
                const float *s = src + ((size_t)n * C + ch) * HW + p;
                if (vec) a = *(const float4 *)s;          // (HW % 4 == 0: the four pixels are inside)
                else {
                    a.x = s[0];
                    if (p + 1 < HW) a.y = s[1];
                    if (p + 2 < HW) a.z = s[2];
                    if (p + 3 < HW) a.w = s[3];
                }
            }
            rg.v[k] = a;
        }
    }
}

template <bool B8, int TC>
__device__ __forceinline__ void w1_store(float *__restrict__ t, const W1Regs<B8, TC> &rg) {
    constexpr int PS = w1_stride(B8), ITEMS = W1Regs<B8, TC>::ITEMS;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int item = threadIdx.x + k * BG_THREADS;
        if constexpr (B8) {
            const int cg = item / W1_P, pix = item - cg * W1_P;
            float4 *d = (float4 *)(t + ((cg >> 2) * W1_P + pix) * PS + (cg & 3) * 8);
            d[0] = rg.v[2 * k]; d[1] = rg.v[2 * k + 1];
        } else {
            const int c = item / (W1_P / 4), pix = (item - c * (W1_P / 4)) * 4;
            float *d = t + ((c >> 5) * W1_P + pix) * PS + (c & 31);
            d[0] = rg.v[k].x; d[PS] = rg.v[k].y; d[2 * PS] = rg.v[k].z; d[3 * PS] = rg.v[k].w;
        }
    }
}

// grid (ci tiles * co tiles, splits): the channel tiles of one slab are neighbours in launch order (they read the same pixels).  Slab s
// takes the chunks [s T / S, (s + 1) T / S) of the T = N * ceil(HW / 32) chunks and writes part[s][co][ci].
template <bool XB8, bool GB8>
__global__ __launch_bounds__(BG_THREADS) void conv1x1_wgrad_kernel(const float *__restrict__ X, const float *__restrict__ G,
                                                                  float *__restrict__ part, int Cin, int Cout, int HW, int chunks, int CPI,
                                                                  int TCI, int xvec, int gvec) {
    constexpr int PSX = w1_stride(XB8), PSG = w1_stride(GB8);
    __shared__ __attribute__((aligned(16))) float gs[(W1_CO / 32) * W1_P * PSG];
    __shared__ __attribute__((aligned(16))) float xs[(W1_CI / 32) * W1_P * PSX];
    const int tco = blockIdx.x / TCI, tci = blockIdx.x - tco * TCI, ci0 = tci * W1_CI, co0 = tco * W1_CO;
    const int s = blockIdx.y, S = gridDim.y;
    const int first = (int)((long long)s * chunks / S), last = (int)((long long)(s + 1) * chunks / S);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const float *ga = gs + (wave * W1_P + h) * PSG + c;
    const float *xa = xs + h * PSX + c;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    W1Regs<GB8, W1_CO> rg_g;
    W1Regs<XB8, W1_CI> rg_x;
    auto load_chunk = [&](int ch) {
        const int n = ch / CPI, p0 = (ch - n * CPI) * W1_P;
        w1_load<GB8, W1_CO>(rg_g, G, n, Cout, co0, HW, p0, gvec);
        w1_load<XB8, W1_CI>(rg_x, X, n, Cin, ci0, HW, p0, xvec);
    };
    load_chunk(first);                                   // (host: at most one slab per chunk, so first < last)
    for (int ch = first; ch < last; ++ch) {
        __syncthreads();                                 // (the previous chunk's reads are done)
        w1_store<GB8, W1_CO>(gs, rg_g);
        w1_store<XB8, W1_CI>(xs, rg_x);
        __syncthreads();
        if (ch + 1 < last) load_chunk(ch + 1);           // in flight during the MFMAs below
#pragma unroll
        for (int kp = 0; kp < W1_P / 2; ++kp) {          // a k step = the pixel pair (2 kp, 2 kp + 1)
            const float a = ga[2 * kp * PSG];
            const float b0 = xa[2 * kp * PSX], b1 = xa[(W1_P + 2 * kp) * PSX];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
        }
    }
    // D[row = co][column = ci]: the column on the lane, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in register r
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ci = ci0 + j * 32 + c;
        if (ci < Cin)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wave * 32 + mfma32_row(r, h);
                if (co < Cout) part[((size_t)s * Cout + co) * Cin + ci] = acc[j][r];
            }
    }
}

// dW[e] = sum_s part[s][e]: 64 elements x 4 ranges of slabs per workgroup, each range in slab order, the four in order (the scheme of
// conv3x3_wgrad_sum_kernel without its tap transposition).
__global__ __launch_bounds__(256) void conv1x1_wgrad_sum_kernel(const float *__restrict__ part, float *__restrict__ dw, int S, int total) {
    __shared__ double red[4][64];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    double v = 0.0;
    if (e < total)
        for (int s = q * S / 4; s < (q + 1) * S / 4; ++s) v += (double)part[(size_t)s * total + e];
    red[q][threadIdx.x & 63] = v;
    __syncthreads();
    if (q == 0 && e < total) dw[e] = (float)(((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]);
}

// ------------------------------------------------------------------ 5. adjoints of the resampling stages (gather form)
__device__ __forceinline__ void bg_ld8(const float *p, float (&v)[8]) {
    const float4 *q = (const float4 *)p;
    const float4 a = q[0], b = q[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void bg_st8(float *p, const float (&v)[8]) {
    float4 *q = (float4 *)p;
    q[0] = make_float4(v[0], v[1], v[2], v[3]);
    q[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// Average pool 3x3 / stride 2 / pad 1, padding counted: input row y lies in the windows of output row y / 2 and, for odd y, y / 2 + 1.
// gin[y][x] = (1/9) * sum of g over those (at most 2 x 2) outputs.  One work-item = 4 consecutive input pixels of a row.
template <bool VEC>
__global__ __launch_bounds__(256) void avgpool3x3s2_backward_kernel(const float *__restrict__ g, float *__restrict__ gin, int H, int W,
                                                                   int OH, int OW) {
    const int W4 = (W + 3) / 4;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W4) return;
    const int y = idx / W4, x0 = (idx - y * W4) * 4;
    const size_t plane = blockIdx.y;
    const float *gp = g + plane * (size_t)OH * OW;
    const int oy0 = y >> 1, ox0 = x0 >> 1;
    const bool two = (y & 1) && oy0 + 1 < OH;
    float c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int ox = ox0 + j;
        const bool ok = ox < OW;
        const float t0 = gp[(size_t)oy0 * OW + (ok ? ox : 0)];
        const float t1 = gp[(size_t)(two ? oy0 + 1 : oy0) * OW + (ok ? ox : 0)];
        c[j] = ok ? (two ? t0 + t1 : t0) : 0.0f;
    }
    const float k9 = 1.0f / 9.0f;
    const float o[4] = {c[0] * k9, (c[0] + c[1]) * k9, c[1] * k9, (c[1] + c[2]) * k9};
    float *op = gin + (plane * H + y) * (size_t)W + x0;
    if (VEC) *(float4 *)op = make_float4(o[0], o[1], o[2], o[3]);
    else
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < W) op[k] = o[k];
}

__global__ __launch_bounds__(256) void avgpool3x3s2_backward_b8_kernel(const float *__restrict__ g, float *__restrict__ gin, int H, int W,
                                                                      int OH, int OW) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int y = idx / W, x = idx - y * W;
    const size_t plane = blockIdx.y;
    const float *gp = g + plane * (size_t)OH * OW * 8;
    const int oy0 = y >> 1, ox0 = x >> 1;
    const bool twoy = (y & 1) && oy0 + 1 < OH, twox = (x & 1) && ox0 + 1 < OW;
    float s[8], t[8];
    bg_ld8(gp + ((size_t)oy0 * OW + ox0) * 8, s);
    if (twoy) {
        bg_ld8(gp + ((size_t)(oy0 + 1) * OW + ox0) * 8, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += t[k];
    }
    if (twox) {                                          // the same order as the NCHW kernel: rows first, then the two columns
        float u[8];
        bg_ld8(gp + ((size_t)oy0 * OW + ox0 + 1) * 8, u);
        if (twoy) {
            bg_ld8(gp + ((size_t)(oy0 + 1) * OW + ox0 + 1) * 8, t);
#pragma unroll
            for (int k = 0; k < 8; ++k) u[k] += t[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += u[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] *= 1.0f / 9.0f;
    bg_st8(gin + (plane * (size_t)H * W + idx) * 8, s);
}

// x2 bilinear, align_corners = False: the weight input position i has in output position o, by the forward's own arithmetic
// (src = max((o + 0.5) / 2 - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, size - 1), l1 = src - i0): the border clamping folds the
// weight of a clamped neighbour onto the border position.  Outputs 2 i - 1 .. 2 i + 2 are the only ones that can reach i.
__device__ __forceinline__ float up_weight(int o, int i, int size) {
    if (o < 0 || o >= 2 * size) return 0.0f;
    const float s = fmaxf((o + 0.5f) * 0.5f - 0.5f, 0.0f);
    const int i0 = (int)s, i1 = min(i0 + 1, size - 1);
    const float l1 = s - (float)i0;
    return (i0 == i ? 1.0f - l1 : 0.0f) + (i1 == i ? l1 : 0.0f);
}

// gin[y][x] = sum_a wy[a] * (sum_b wx[b] * g[2 y - 1 + a][2 x - 1 + b]).  One work-item = the input pixels (y, x0), (y, x0 + 1), x0 even:
// output columns 2 x0 - 1 .. 2 x0 + 4 of four rows, the middle four as one 16-byte load with VEC.
template <bool VEC>
__global__ __launch_bounds__(256) void upsample2x_backward_kernel(const float *__restrict__ g, float *__restrict__ gin, int H, int W) {
    const int W2 = (W + 1) / 2, OW = 2 * W, OH = 2 * H;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W2) return;
    const int y = idx / W2, x0 = (idx - y * W2) * 2;
    const size_t plane = blockIdx.y;
    const float *gp = g + plane * (size_t)OH * OW;
    const bool second = x0 + 1 < W;
    float wa[4], wb[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        wa[b] = up_weight(2 * x0 - 1 + b, x0, W);
        wb[b] = second ? up_weight(2 * x0 + 1 + b, x0 + 1, W) : 0.0f;
    }
    // t0, t1 = the column sums of one output row for the two pixels.  torch's forward gives output 0 the taps (1, 0) on inputs 0 and 1 --
    // l1 = 0 at the clamped source position -- so its backward sends 0 x g[0] to input 1: nothing for a finite g, a NaN for a NaN (or
    // an infinite) one.  The term is kept as a select, which leaves the bits of every finite result alone.
    auto row_sums = [&](const float *row, float &t0, float &t1) {
        float v[6];
        const int xl = 2 * x0 - 1, xr = 2 * x0 + 4;
        v[0] = row[xl >= 0 ? xl : 0];
        if (VEC) {                                       // OW % 4 == 0: 2 x0 is a multiple of 4 and 2 x0 + 3 < OW
            const float4 q = *(const float4 *)(row + 2 * x0);
            v[1] = q.x; v[2] = q.y; v[3] = q.z; v[4] = q.w;
        } else {
#pragma unroll
            for (int k = 1; k < 5; ++k) v[k] = row[min(xl + k, OW - 1)];
        }
        v[5] = row[xr < OW ? xr : OW - 1];               // (a clamped address only ever meets weight 0)
        t0 = ((wa[0] * v[0] + wa[1] * v[1]) + wa[2] * v[2]) + wa[3] * v[3];
        t1 = ((wb[0] * v[2] + wb[1] * v[3]) + wb[2] * v[4]) + wb[3] * v[5];
        const float z = 0.0f * v[1];                     // output column 0 onto input column 1
        if (x0 == 0 && z != z) t1 = z;
    };
    float r0 = 0.0f, r1 = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int oy = 2 * y - 1 + a;
        const float wy = up_weight(oy, y, H);
        float t0, t1;
        row_sums(gp + (size_t)min(max(oy, 0), OH - 1) * OW, t0, t1);
        r0 += wy * t0;
        r1 += wy * t1;
    }
    if (y == 1) {                                        // output row 0 onto input row 1, the same zero-weight term
        float t0, t1;
        row_sums(gp, t0, t1);
        const float z0 = 0.0f * t0, z1 = 0.0f * t1;
        if (z0 != z0) r0 = z0;
        if (z1 != z1) r1 = z1;
    }
    float *op = gin + (plane * H + y) * (size_t)W + x0;
    op[0] = r0;
    if (second) op[1] = r1;
}

__global__ __launch_bounds__(256) void upsample2x_backward_b8_kernel(const float *__restrict__ g, float *__restrict__ gin, int H, int W) {
    const int OW = 2 * W, OH = 2 * H;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int y = idx / W, x = idx - y * W;
    const size_t plane = blockIdx.y;
    const float *gp = g + plane * (size_t)OH * OW * 8;
    float wx[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) wx[b] = up_weight(2 * x - 1 + b, x, W);
    // (the zero-weight terms of output row / column 0 onto input row / column 1: see the NCHW kernel)
    auto row_sums = [&](const float *row, float (&t)[8]) {
        float v[4][8];
#pragma unroll
        for (int b = 0; b < 4; ++b) bg_ld8(row + (size_t)min(max(2 * x - 1 + b, 0), OW - 1) * 8, v[b]);
#pragma unroll
        for (int k = 0; k < 8; ++k)                      // the NCHW kernel's order per channel
            t[k] = ((wx[0] * v[0][k] + wx[1] * v[1][k]) + wx[2] * v[2][k]) + wx[3] * v[3][k];
        if (x == 1) {
            float c0[8];
            bg_ld8(row, c0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float z = 0.0f * c0[k];
                if (z != z) t[k] = z;
            }
        }
    };
    float r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int oy = 2 * y - 1 + a;
        const float wy = up_weight(oy, y, H);
        float t[8];
        row_sums(gp + (size_t)min(max(oy, 0), OH - 1) * OW * 8, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += wy * t[k];
    }
    if (y == 1) {
        float t[8];
        row_sums(gp, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float z = 0.0f * t[k];
            if (z != z) r[k] = z;
        }
    }
    bg_st8(gin + (plane * (size_t)H * W + idx) * 8, r);
}

// ------------------------------------------------------------------ host side
// The workspace of a mask kind: part | mpart or cpart | ab -- the partial sums (the blocked form's count; the NCHW form needs no more),
// the mask's partial sums [N][GX] in double or the nonzero counts [N][C][GX], the statistics' coefficients.
static size_t bn_part_bytes(int N, int C, int HW, bool nz) { return al256((size_t)N * C * bg_gx(HW, true, bn_ppt(nz)) * 2 * sizeof(double)); }
static size_t bn_cnt_bytes(int N, int C, int HW, bool nz) {
    return nz ? al256((size_t)N * C * bg_gx(HW, true, bn_ppt(nz)) * sizeof(unsigned)) : al256((size_t)N * bg_gx(HW, true, bn_ppt(nz)) * sizeof(double));
}
static size_t bn_ws_bytes(int N, int C, int HW, bool nz) {
    return bn_part_bytes(N, C, HW, nz) + bn_cnt_bytes(N, C, HW, nz) + al256((size_t)2 * C * sizeof(float));
}

// An export of the family: its name and its workspace function's (for the error texts), its mask kind
struct BnExport {
    const char *fn, *ws_fn;
    bool nz;
};
static int bn_ws_check(const BnExport &ex, const void *ws, size_t ws_bytes, int N, int C, int HW) {
    if (ws && !((uintptr_t)ws & 255) && ws_bytes >= bn_ws_bytes(N, C, HW, ex.nz)) return 0;
    set_error("%s: ws: %s(N, C, H, W) bytes, 256-byte aligned", ex.fn, ex.ws_fn);
    return SLR_E_WORKSPACE;
}

// Launches the instantiation of a family kernel for (b8, ex.nz); KERNEL: one of the BN_* macros below, which add the PPT of the mask kind
#define BN_LAUNCH(KERNEL, grid, ...)                                                                                    \
    do {                                                                                                                \
        if (b8 && ex.nz) hipLaunchKernelGGL((KERNEL(true, true)), grid, dim3(BG_THREADS), 0, st, __VA_ARGS__);          \
        else if (b8) hipLaunchKernelGGL((KERNEL(true, false)), grid, dim3(BG_THREADS), 0, st, __VA_ARGS__);             \
        else if (ex.nz) hipLaunchKernelGGL((KERNEL(false, true)), grid, dim3(BG_THREADS), 0, st, __VA_ARGS__);          \
        else hipLaunchKernelGGL((KERNEL(false, false)), grid, dim3(BG_THREADS), 0, st, __VA_ARGS__);                    \
        SLR_CHECK_HIP_FN(ex.fn, hipGetLastError());                                                                     \
    } while (0)
#define BN_STATS(B8, NZ) bn_stats_kernel<B8, NZ, bn_ppt(NZ)>
#define BN_FORWARD(B8, NZ) bn_train_forward_kernel<B8, NZ>
#define BN_REDUCE(B8, NZ) bn_backward_reduce_kernel<B8, NZ, bn_ppt(NZ)>
#define BN_DX(B8, NZ) bn_backward_dx_kernel<B8, NZ>

static int bn_stats(const BnExport &ex, const float *x, const float *mask, float eps, float *mean, float *var, float *count, int N, int C,
                    int H, int W, int b8, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG_FN(ex.fn, x && mean && var && count, "null pointer");
    BG_CHECK_PLANES(ex.fn, C);
    SLR_CHECK_ARG_FN(ex.fn, eps >= 0.0f, "eps");
    SLR_CHECK_ARG_FN(ex.fn, !(((uintptr_t)x | (uintptr_t)mask | (uintptr_t)mean | (uintptr_t)var | (uintptr_t)count) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG_FN(ex.fn, !(b8 && ((uintptr_t)x & 15)), "16-byte aligned channel-blocked tensors");
    const int HW = H * W;
    if (const int e = bn_ws_check(ex, ws, ws_bytes, N, C, HW)) return e;
    hipStream_t st = (hipStream_t)stream;
    const int vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)mask) & 15);
    double *part = (double *)ws;
    void *cnt = (char *)ws + bn_part_bytes(N, C, HW, ex.nz);
    const dim3 grid = bg_grid(N, C, HW, b8, bn_ppt(ex.nz));
    BN_LAUNCH(BN_STATS, grid, x, mask, part, cnt, b8 ? C / 8 : C, HW, vec);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C), dim3(256), 0, st, (const double *)part, (const double *)(!ex.nz && mask ? cnt : nullptr),
                       (const unsigned *)(ex.nz ? cnt : nullptr), mean, var, count, N, C, (int)grid.x, b8, eps, HW);
    SLR_CHECK_HIP_FN(ex.fn, hipGetLastError());
    return 0;
}

static int bn_forward(const BnExport &ex, const float *x, const float *scale, const float *shift, const float *mask, float *a, int N, int C,
                      int H, int W, int b8, void *stream) {
    SLR_CHECK_ARG_FN(ex.fn, x && scale && shift && a, "null pointer");
    BG_CHECK_PLANES(ex.fn, C);
    SLR_CHECK_ARG_FN(ex.fn, !(((uintptr_t)x | (uintptr_t)mask | (uintptr_t)a | (uintptr_t)scale | (uintptr_t)shift) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG_FN(ex.fn, !(b8 && (((uintptr_t)x | (uintptr_t)a) & 15)), "16-byte aligned channel-blocked tensors");
    const int HW = H * W, vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)mask | (uintptr_t)a) & 15);
    hipStream_t st = (hipStream_t)stream;
    BN_LAUNCH(BN_FORWARD, bg_grid(N, C, HW, b8), x, scale, shift, mask, a, b8 ? C / 8 : C, HW, vec);
    return 0;
}

static int bn_backward(const BnExport &ex, const float *x, const float *ga, const float *mask, const float *scale, const float *shift,
                       const float *mean, const float *var, const float *gain, const float *count, float eps, const float *addend, float *dx,
                       float *dgain, float *dbias, int stored, int N, int C, int H, int W, int b8, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG_FN(ex.fn, x && ga && scale && shift && mean && var, "null pointer");
    SLR_CHECK_ARG_FN(ex.fn, dx || dgain || dbias, "null pointer: nothing to compute");
    SLR_CHECK_ARG_FN(ex.fn, stored == 0 || stored == 1, "stored");
    SLR_CHECK_ARG_FN(ex.fn, stored || count, ex.nz ? "null pointer: batch statistics need their counts" : "null pointer: batch statistics need their count");
    SLR_CHECK_ARG_FN(ex.fn, !addend || dx, "addend goes with dx");
    BG_CHECK_PLANES(ex.fn, C);
    SLR_CHECK_ARG_FN(ex.fn, eps >= 0.0f, "eps");
    SLR_CHECK_ARG_FN(ex.fn, !(((uintptr_t)x | (uintptr_t)ga | (uintptr_t)mask | (uintptr_t)addend | (uintptr_t)dx | (uintptr_t)dgain | (uintptr_t)dbias) & 3),
                     "4-byte aligned tensors");
    SLR_CHECK_ARG_FN(ex.fn, !(b8 && (((uintptr_t)x | (uintptr_t)ga | (uintptr_t)addend | (uintptr_t)dx) & 15)), "16-byte aligned channel-blocked tensors");
    const int HW = H * W;
    const bool reduce = dgain || dbias || !stored;
    if (reduce)
        if (const int e = bn_ws_check(ex, ws, ws_bytes, N, C, HW)) return e;
    hipStream_t st = (hipStream_t)stream;
    const int vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)ga | (uintptr_t)mask | (uintptr_t)addend | (uintptr_t)dx) & 15);
    const int planes = b8 ? C / 8 : C;
    float *ab = nullptr;
    if (reduce) {
        double *part = (double *)ws;
        if (dx && !stored) ab = (float *)((char *)ws + bn_part_bytes(N, C, HW, ex.nz) + bn_cnt_bytes(N, C, HW, ex.nz));
        const dim3 grid = bg_grid(N, C, HW, b8, bn_ppt(ex.nz));
        BN_LAUNCH(BN_REDUCE, grid, x, ga, mask, scale, shift, part, planes, HW, vec);
        hipLaunchKernelGGL(bn_backward_final_kernel, dim3(C), dim3(256), 0, st, (const double *)part, mean, var, gain, count, ex.nz ? 1 : 0, eps,
                           dgain, dbias, ab, N, C, (int)grid.x, b8, stored);
        SLR_CHECK_HIP_FN(ex.fn, hipGetLastError());
    }
    if (dx) BN_LAUNCH(BN_DX, bg_grid(N, C, HW, b8), x, ga, mask, scale, shift, mean, (const float *)ab, addend, dx, planes, HW, vec);
    return 0;
}

static long long w1_chunks(int N, int HW) { return (long long)N * ((HW + W1_P - 1) / W1_P); }
static int w1_tiles(int Cin, int Cout) { return ((Cin + W1_CI - 1) / W1_CI) * ((Cout + W1_CO - 1) / W1_CO); }
static bool w1_sizes_ok(int N, int Cin, int Cout, int H, int W) {
    return N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && (long long)N * (Cin > Cout ? Cin : Cout) * H * W < (1LL << 31) - 1024 &&
           (long long)Cin * Cout < (1LL << 28) && w1_tiles(Cin, Cout) <= (1 << 20);
}
static int w1_splits(int N, int Cin, int Cout, int H, int W, int splits) {
    const long long chunks = w1_chunks(N, H * W);
    long long S = splits > 0 ? splits : slr_wgrad1x1_auto_splits(chunks, w1_tiles(Cin, Cout), (long long)Cout * Cin * 4);
    if (S > 65535) S = 65535;
    return (int)(S < chunks ? S : chunks);
}

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI
// The batch-norm family's exports, plane mask (ABI 16) and nonzero mask (ABI 17): the arguments of the launchers above.
static const BnExport BN_PLANE_STATS = {"slr_bn_batch_stats", "slr_bn_train_ws_bytes", false}, BN_PLANE_FORWARD = {"slr_bn_relu_mask_train", "slr_bn_train_ws_bytes", false},
                      BN_PLANE_BACKWARD = {"slr_bn_relu_mask_backward", "slr_bn_train_ws_bytes", false},
                      BN_NZ_STATS = {"slr_bn_nonzero_stats", "slr_bn_nonzero_ws_bytes", true}, BN_NZ_FORWARD = {"slr_bn_relu_nonzero_train", "slr_bn_nonzero_ws_bytes", true},
                      BN_NZ_BACKWARD = {"slr_bn_relu_nonzero_backward", "slr_bn_nonzero_ws_bytes", true};

SLR_EXPORT size_t slr_bn_train_ws_bytes(int N, int C, int H, int W) { return bg_sizes_ok(N, C, H, W) ? bn_ws_bytes(N, C, H * W, false) : 0; }
SLR_EXPORT size_t slr_bn_nonzero_ws_bytes(int N, int C, int H, int W) { return bg_sizes_ok(N, C, H, W) ? bn_ws_bytes(N, C, H * W, true) : 0; }

SLR_EXPORT int slr_bn_batch_stats(const float *x, const float *mask, float eps, float *mean, float *var, float *count, int N, int C, int H,
                                  int W, int b8, void *ws, size_t ws_bytes, void *stream) {
    return bn_stats(BN_PLANE_STATS, x, mask, eps, mean, var, count, N, C, H, W, b8, ws, ws_bytes, stream);
}
SLR_EXPORT int slr_bn_nonzero_stats(const float *x, float eps, float *mean, float *var, float *count, int N, int C, int H, int W, int b8,
                                    void *ws, size_t ws_bytes, void *stream) {
    return bn_stats(BN_NZ_STATS, x, nullptr, eps, mean, var, count, N, C, H, W, b8, ws, ws_bytes, stream);
}

SLR_EXPORT int slr_bn_train_tables(const float *mean, const float *var, const float *gain, const float *bias, float eps, float *scale,
                                   float *shift, int N, int C, void *stream) {
    SLR_CHECK_ARG(mean && var && scale && shift, "null pointer");
    SLR_CHECK_ARG(N > 0 && C > 0 && (long long)N * C <= 65535, "sizes (N * C <= 65535)");
    SLR_CHECK_ARG(eps >= 0.0f, "eps");
    hipLaunchKernelGGL(bn_tables_kernel, dim3((N * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean, var, gain, bias, eps, scale,
                       shift, N * C, C);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_bn_relu_mask_train(const float *x, const float *scale, const float *shift, const float *mask, float *a, int N, int C,
                                      int H, int W, int b8, void *stream) {
    return bn_forward(BN_PLANE_FORWARD, x, scale, shift, mask, a, N, C, H, W, b8, stream);
}
SLR_EXPORT int slr_bn_relu_nonzero_train(const float *x, const float *scale, const float *shift, float *a, int N, int C, int H, int W,
                                         int b8, void *stream) {
    return bn_forward(BN_NZ_FORWARD, x, scale, shift, nullptr, a, N, C, H, W, b8, stream);
}

SLR_EXPORT int slr_bn_relu_mask_backward(const float *x, const float *ga, const float *mask, const float *scale, const float *shift,
                                         const float *mean, const float *var, const float *gain, const float *count, float eps,
                                         const float *addend, float *dx, float *dgain, float *dbias, int stored, int N, int C, int H, int W,
                                         int b8, void *ws, size_t ws_bytes, void *stream) {
    return bn_backward(BN_PLANE_BACKWARD, x, ga, mask, scale, shift, mean, var, gain, count, eps, addend, dx, dgain, dbias, stored, N, C, H, W, b8,
                       ws, ws_bytes, stream);
}
SLR_EXPORT int slr_bn_relu_nonzero_backward(const float *x, const float *ga, const float *scale, const float *shift, const float *mean,
                                            const float *var, const float *gain, const float *count, float eps, const float *addend,
                                            float *dx, float *dgain, float *dbias, int stored, int N, int C, int H, int W, int b8, void *ws,
                                            size_t ws_bytes, void *stream) {
    return bn_backward(BN_NZ_BACKWARD, x, ga, nullptr, scale, shift, mean, var, gain, count, eps, addend, dx, dgain, dbias, stored, N, C, H, W, b8,
                       ws, ws_bytes, stream);
}

SLR_EXPORT size_t slr_conv1x1_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int splits) {
    if (!w1_sizes_ok(N, Cin, Cout, H, W) || splits < 0) return 0;
    return al256((size_t)w1_splits(N, Cin, Cout, H, W, splits) * Cout * Cin * sizeof(float));
}

SLR_EXPORT int slr_conv1x1_weight_grad(const float *x, const float *g, float *dw, int N, int Cin, int Cout, int H, int W, int splits,
                                       int layout, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(x && g && dw, "null pointer");
    SLR_CHECK_ARG(w1_sizes_ok(N, Cin, Cout, H, W), "sizes (N * max(Cin, Cout) * H * W < 2^31 - 1024, Cin * Cout < 2^28)");
    SLR_CHECK_ARG(splits >= 0, "splits (0 = chosen by the library)");
    SLR_CHECK_ARG(!(layout & ~(SLR_GRAD_X_B8 | SLR_GRAD_G_B8)), "layout");
    const bool xb8 = layout & SLR_GRAD_X_B8, gb8 = layout & SLR_GRAD_G_B8;
    SLR_CHECK_ARG(!xb8 || Cin % 8 == 0, "SLR_GRAD_X_B8 needs Cin % 8 == 0");
    SLR_CHECK_ARG(!gb8 || Cout % 8 == 0, "SLR_GRAD_G_B8 needs Cout % 8 == 0");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)g | (uintptr_t)dw) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(!(xb8 && ((uintptr_t)x & 15)) && !(gb8 && ((uintptr_t)g & 15)), "16-byte aligned channel-blocked tensors");
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < slr_conv1x1_grad_ws_bytes(N, Cin, Cout, H, W, splits)) {
        set_error("%s: ws: slr_conv1x1_grad_ws_bytes(N, Cin, Cout, H, W, splits) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, S = w1_splits(N, Cin, Cout, H, W, splits);
    const int chunks = (int)w1_chunks(N, HW), CPI = (HW + W1_P - 1) / W1_P, TCI = (Cin + W1_CI - 1) / W1_CI;
    const int xvec = HW % 4 == 0 && !((uintptr_t)x & 15), gvec = HW % 4 == 0 && !((uintptr_t)g & 15);
    float *part = (float *)ws;
    const dim3 grid(w1_tiles(Cin, Cout), S);
#define SLR_W1_LAUNCH(XB, GB) \
    hipLaunchKernelGGL((conv1x1_wgrad_kernel<XB, GB>), grid, dim3(BG_THREADS), 0, st, x, g, part, Cin, Cout, HW, chunks, CPI, TCI, xvec, gvec)
    if (xb8 && gb8) SLR_W1_LAUNCH(true, true);
    else if (xb8) SLR_W1_LAUNCH(true, false);
    else if (gb8) SLR_W1_LAUNCH(false, true);
    else SLR_W1_LAUNCH(false, false);
#undef SLR_W1_LAUNCH
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(conv1x1_wgrad_sum_kernel, dim3((Cout * Cin + 63) / 64), dim3(256), 0, st, (const float *)part, dw, S, Cout * Cin);
    SLR_CHECK_LAUNCH();
    return 0;
}

// H, W: the size of the pooled / up-sampled tensor's INPUT, i.e. of gin
SLR_EXPORT int slr_avgpool3x3s2_backward(const float *g, float *gin, int N, int C, int H, int W, int b8, void *stream) {
    SLR_CHECK_ARG(g && gin, "null pointer");
    SLR_CHECK_ARG(b8 == 0 || b8 == 1, "b8");
    SLR_CHECK_ARG(!b8 || (C % 8 == 0 && !(((uintptr_t)g | (uintptr_t)gin) & 15)), "channel-blocked layout needs C % 8 == 0 and 16-byte aligned tensors");
    SLR_CHECK_ARG(!(((uintptr_t)g | (uintptr_t)gin) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C < 65536 && (long long)H * W < (1LL << 30), "sizes");
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    hipStream_t st = (hipStream_t)stream;
    if (b8) {
        hipLaunchKernelGGL(avgpool3x3s2_backward_b8_kernel, dim3((H * W + 255) / 256, N * C / 8), dim3(256), 0, st, g, gin, H, W, OH, OW);
        SLR_CHECK_LAUNCH();
        return 0;
    }
    const dim3 grid((H * ((W + 3) / 4) + 255) / 256, N * C);
    if (W % 4 == 0 && !((uintptr_t)gin & 15)) hipLaunchKernelGGL(avgpool3x3s2_backward_kernel<true>, grid, dim3(256), 0, st, g, gin, H, W, OH, OW);
    else hipLaunchKernelGGL(avgpool3x3s2_backward_kernel<false>, grid, dim3(256), 0, st, g, gin, H, W, OH, OW);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_upsample_bilinear2x_backward(const float *g, float *gin, int N, int C, int H, int W, int b8, void *stream) {
    SLR_CHECK_ARG(g && gin, "null pointer");
    SLR_CHECK_ARG(b8 == 0 || b8 == 1, "b8");
    SLR_CHECK_ARG(!b8 || (C % 8 == 0 && !(((uintptr_t)g | (uintptr_t)gin) & 15)), "channel-blocked layout needs C % 8 == 0 and 16-byte aligned tensors");
    SLR_CHECK_ARG(!(((uintptr_t)g | (uintptr_t)gin) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C < 65536 && (long long)H * W < (1LL << 28), "sizes");
    hipStream_t st = (hipStream_t)stream;
    if (b8) {
        hipLaunchKernelGGL(upsample2x_backward_b8_kernel, dim3((H * W + 255) / 256, N * C / 8), dim3(256), 0, st, g, gin, H, W);
        SLR_CHECK_LAUNCH();
        return 0;
    }
    const dim3 grid((H * ((W + 1) / 2) + 255) / 256, N * C);
    if (W % 2 == 0 && !((uintptr_t)g & 15)) hipLaunchKernelGGL(upsample2x_backward_kernel<true>, grid, dim3(256), 0, st, g, gin, H, W);
    else hipLaunchKernelGGL(upsample2x_backward_kernel<false>, grid, dim3(256), 0, st, g, gin, H, W);
    SLR_CHECK_LAUNCH();
    return 0;
}
