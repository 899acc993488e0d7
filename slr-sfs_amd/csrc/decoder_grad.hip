// decoder_grad.hip -- what the decoder's FIRST block needs to learn beyond csrc/block_grad.hip (ABI 17): ResNet_Block_Pconv2 called with the
// per-element mask (x != 0) of models/networks/architectures.py:369.  The mask k = [x != 0] is never a tensor: every kernel recomputes it
// from x, as the ReLU gate already is.
//   * batch statistics (models/layers/normalization.py:319-335 with a [N,C,H,W] mask): per channel the sums of x and x^2 in double and the
//     INTEGER number of nonzero elements; count[c] = nnz + eps, mean = sum x / count, var = sum x^2 / count - mean^2, rounded once.
//   * msum[n,1,h,w] = sum_c k: what the partial convolution behind the BN needs of the mask (partialconv2d.py:61-72), exact integers.
//   * a = relu(x * scale[n,c] - shift[n,c]) * k, and its backward: gy = ga * k * [y > 0]; reduce, finalize, dx = gy * scale + A + B (x - m)
//     (+ addend) with the per-channel count -- the A + B (x - m) term reaches the zero elements as well, as the reference's autograd does.
//   * the partial convolution's epilogue with given factor planes: out = (raw * ratio + bias) * um (+ residual).
// The two reductions take several items per thread (DG_PPT) before the one workgroup sum: the float64 wave reductions that bound
// block_grad.hip's passes are paid once per 8 items.  Both layouts, no atomics, every sum in double in a fixed order: the same
// inputs give the same bits.  Nothing here synchronises.
#include "slr_common.hpp"
#include "slr_reduce.hpp"
#include "block_items.hpp"

namespace slr {

constexpr int DG_PPT = 8;                                // items of a thread in the two reduction kernels

// The thread's j-th item in a reduction kernel: workgroup bx owns the items [bx * DG_PPT * 256, (bx + 1) * DG_PPT * 256) of its plane,
// item (j * 256 + thread) of them; consecutive threads stay on consecutive addresses.  Items past the plane have cnt = 0.
template <bool B8> __device__ __forceinline__ BgItem<B8> dg_item(int planes, int HW, int vec, int j) {
    BgItem<B8> it;
    const int plane = blockIdx.y;
    it.n = plane / planes;
    const int cp = plane - it.n * planes;
    const long long p = ((long long)(blockIdx.x * DG_PPT + j) * BG_THREADS + threadIdx.x) * (B8 ? 1 : 4);
    const long long left = (long long)HW - p;
    it.c0 = B8 ? cp * 8 : cp;
    it.cnt = B8 ? (left > 0 ? 8 : 0) : (left >= 4 ? 4 : left > 0 ? (int)left : 0);
    it.v4 = !B8 && vec && it.cnt == 4;
    it.off = it.cnt ? (B8 ? ((size_t)plane * HW + (size_t)p) * 8 : (size_t)plane * HW + (size_t)p) : 0;
    it.moff = it.cnt ? (size_t)it.n * HW + (size_t)p : 0;
    return it;
}

// Sum of K counters per thread over a workgroup of NW waves; thread 0 returns the sums.  Every thread calls it.
template <int K, int NW>
__device__ __forceinline__ void block_count(unsigned (&c)[K], unsigned (*red)[NW]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[k] += (unsigned)__shfl_xor((int)c[k], o, 64);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[k][wave] = c[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) s += red[k][w];
            c[k] = s;
        }
}

// The workgroup's count of channel c, image n, workgroup bx (the layout of bg_part with one value per channel)
__device__ __forceinline__ unsigned dg_cpart(const unsigned *cpart, int n, int c, int bx, int C, int GX, int b8) {
    return b8 ? cpart[(((size_t)n * (C >> 3) + (c >> 3)) * GX + bx) * 8 + (c & 7)] : cpart[((size_t)n * C + c) * GX + bx];
}

// ------------------------------------------------------------------ 1. batch statistics with the per-element mask
// part[(plane * GX + bx) * 2 KS + ...]: the workgroup's sums of x and x^2 per channel (KS = 8 channels blocked, 1 NCHW) in double -- over all
// elements, which is over the kept ones: the others are exact zeros; cpart[(plane * GX + bx) * KS + ...]: its number of nonzero elements.
template <bool B8>
__global__ __launch_bounds__(BG_THREADS) void nz_stats_kernel(const float *__restrict__ x, double *__restrict__ part,
                                                             unsigned *__restrict__ cpart, int planes, int HW, int vec) {
    constexpr int K = BgItem<B8>::K, KS = B8 ? 8 : 1, NV = 2 * KS;
    __shared__ double red[NV][BG_THREADS / 64];
    __shared__ unsigned cred[KS][BG_THREADS / 64];
    double v[NV];
    unsigned c[KS];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
#pragma unroll
    for (int j = 0; j < KS; ++j) c[j] = 0;
#pragma unroll 2
    for (int j = 0; j < DG_PPT; ++j) {
        const BgItem<B8> it = dg_item<B8>(planes, HW, vec, j);
        if (it.cnt == 0) break;                          // (the items of a thread go up the plane: nothing follows)
        float e[K];
        bg_load<B8>(it, x, e);                           // (elements past the plane read as 0: no sum and no count sees them)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double d = (double)e[k];
            v[B8 ? 2 * k : 0] += d;
            v[B8 ? 2 * k + 1 : 1] += d * d;
            c[B8 ? k : 0] += e[k] != 0.0f ? 1u : 0u;
        }
    }
    block_sum<NV, BG_THREADS / 64>(v, red);
    block_count<KS, BG_THREADS / 64>(c, cred);
    if (threadIdx.x == 0) {
        const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
        for (int j = 0; j < NV; ++j) part[wg * NV + j] = v[j];
#pragma unroll
        for (int j = 0; j < KS; ++j) cpart[wg * KS + j] = c[j];
    }
}

// One workgroup per channel: the partial sums in the order (n, bx); count = nnz + eps (normalization.py:325), mean, var.
__global__ __launch_bounds__(256) void nz_stats_final_kernel(const double *__restrict__ part, const unsigned *__restrict__ cpart,
                                                             float *__restrict__ mean, float *__restrict__ var, float *__restrict__ count,
                                                             int N, int C, int GX, int b8, float eps) {
    __shared__ double red[3][4];
    const int c = blockIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    unsigned long long nz = 0;
    for (int i = threadIdx.x; i < N * GX; i += 256) {
        const int n = i / GX, bx = i - n * GX;
        const double *q = bg_part(part, n, c, bx, C, GX, b8);
        v[0] += q[0];
        v[1] += q[1];
        nz += dg_cpart(cpart, n, c, bx, C, GX, b8);
    }
    v[2] = (double)nz;                                   // (integers below 2^31: every sum of them is exact in double)
    block_sum<3, 4>(v, red);
    if (threadIdx.x == 0) {
        const double cnt = v[2] + (double)eps;
        const double m = v[0] / cnt;
        mean[c] = (float)m;
        var[c] = (float)(v[1] / cnt - m * m);
        count[c] = (float)cnt;
    }
}

// ------------------------------------------------------------------ 2. the mask as the partial convolution sees it
// msum[n,0,p] = sum_c [x[n,c,p] != 0].  In the blocked layout a pixel's channels lie in C / 8 planes: a thread walks them for its pixel;
// NCHW: a thread walks the C planes for its four pixels.  grid (ceil(HW / 256) | ceil(HW / 1024), N).
template <bool B8>
__global__ __launch_bounds__(BG_THREADS) void nz_count_plane_kernel(const float *__restrict__ x, float *__restrict__ msum, int C, int HW,
                                                                   int vec) {
    const int n = blockIdx.y;
    const int p = (blockIdx.x * BG_THREADS + threadIdx.x) * (B8 ? 1 : 4);
    if (p >= HW) return;
    if constexpr (B8) {
        const int G8 = C >> 3;
        const float4 *q = (const float4 *)(x + ((size_t)n * G8 * HW + p) * 8);
        int s = 0;
#pragma unroll 4
        for (int g = 0; g < G8; ++g) {
            const float4 a = q[(size_t)g * HW * 2], b = q[(size_t)g * HW * 2 + 1];
            s += (a.x != 0.0f) + (a.y != 0.0f) + (a.z != 0.0f) + (a.w != 0.0f) + (b.x != 0.0f) + (b.y != 0.0f) + (b.z != 0.0f) + (b.w != 0.0f);
        }
        msum[(size_t)n * HW + p] = (float)s;
    } else {
        const int cnt = HW - p >= 4 ? 4 : HW - p;
        const float *q = x + (size_t)n * C * HW + p;
        int s[4] = {0, 0, 0, 0};
        if (vec && cnt == 4) {
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const float4 a = *(const float4 *)(q + (size_t)c * HW);
                s[0] += a.x != 0.0f; s[1] += a.y != 0.0f; s[2] += a.z != 0.0f; s[3] += a.w != 0.0f;
            }
            *(float4 *)(msum + (size_t)n * HW + p) = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
        } else {
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) s[k] += q[(size_t)c * HW + k] != 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) msum[(size_t)n * HW + p + k] = (float)s[k];
        }
    }
}

// ------------------------------------------------------------------ 3. training BN + ReLU + per-element mask
template <bool B8>
__global__ __launch_bounds__(BG_THREADS) void nz_forward_kernel(const float *__restrict__ x, const float *__restrict__ scale,
                                                               const float *__restrict__ shift, float *__restrict__ a, int planes, int HW,
                                                               int vec) {
    constexpr int K = BgItem<B8>::K;
    const BgItem<B8> it = bg_item<B8>(planes, HW, vec);
    if (it.cnt == 0) return;
    const int C = B8 ? planes * 8 : planes;
    float e[K], sc[K], sh[K];
    bg_load<B8>(it, x, e);
    bg_table<B8>(it, scale, it.n, C, sc);
    bg_table<B8>(it, shift, it.n, C, sh);
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = relu_nan(e[k] * sc[k] - sh[k]) * (e[k] != 0.0f ? 1.0f : 0.0f);      // (NaN stays NaN)
    bg_store<B8>(it, a, e);
}

// ------------------------------------------------------------------ 4. its backward
// gy = ga * k * [x * scale - shift > 0] at the item's elements (the forward's own fp32 expression decides the gate)
template <bool B8>
__device__ __forceinline__ void nz_gate(const BgItem<B8> &it, const float *__restrict__ ga, const float *__restrict__ scale,
                                        const float *__restrict__ shift, int C, const float (&e)[BgItem<B8>::K], float (&sc)[BgItem<B8>::K],
                                        float (&gy)[BgItem<B8>::K]) {
    constexpr int K = BgItem<B8>::K;
    float sh[K], g[K];
    bg_load<B8>(it, ga, g);
    bg_table<B8>(it, scale, it.n, C, sc);
    bg_table<B8>(it, shift, it.n, C, sh);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float y = e[k] * sc[k] - sh[k];
        gy[k] = (y <= 0.0f || e[k] == 0.0f) ? 0.0f : g[k];      // (closed on `<= 0` only, as torch's ReLU backward: open for a NaN)
    }
}

// part[(plane * GX + bx) * 2 KS + ...] = the workgroup's s0 = sum gy and s1 = sum gy * x per channel, in double
template <bool B8>
__global__ __launch_bounds__(BG_THREADS) void nz_backward_reduce_kernel(const float *__restrict__ x, const float *__restrict__ ga,
                                                                       const float *__restrict__ scale, const float *__restrict__ shift,
                                                                       double *__restrict__ part, int planes, int HW, int vec) {
    constexpr int K = BgItem<B8>::K, KS = B8 ? 8 : 1, NV = 2 * KS;
    __shared__ double red[NV][BG_THREADS / 64];
    const int C = B8 ? planes * 8 : planes;
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
#pragma unroll 2
    for (int j = 0; j < DG_PPT; ++j) {
        const BgItem<B8> it = dg_item<B8>(planes, HW, vec, j);
        if (it.cnt == 0) break;
        float e[K], sc[K], gy[K];
        bg_load<B8>(it, x, e);
        nz_gate<B8>(it, ga, scale, shift, C, e, sc, gy);  // (elements past the plane: x reads as 0, so k = 0 and gy = 0)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double d = (double)gy[k];
            v[B8 ? 2 * k : 0] += d;
            v[B8 ? 2 * k + 1 : 1] += d * (double)e[k];
        }
    }
    block_sum<NV, BG_THREADS / 64>(v, red);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NV;
#pragma unroll
        for (int j = 0; j < NV; ++j) p[j] = v[j];
    }
}

// bn_backward_final_kernel of block_grad.hip with the count of the channel: ab[c] = A = -rs P / cnt[c], ab[C + c] = B = 2 dv / cnt[c].
__global__ __launch_bounds__(256) void nz_backward_final_kernel(const double *__restrict__ part, const float *__restrict__ mean,
                                                                const float *__restrict__ var, const float *__restrict__ gain,
                                                                const float *__restrict__ cnt, float eps, float *__restrict__ dgain,
                                                                float *__restrict__ dbias, float *__restrict__ ab, int N, int C, int GX,
                                                                int b8, int stored) {
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
        const double n_el = stored ? 1.0 : (double)cnt[c];
        const double dv = -0.5 * rs * rs * rs * (Q - m * P);
        ab[c] = stored ? 0.0f : (float)(-rs * P / n_el);
        ab[C + c] = stored ? 0.0f : (float)(2.0 * dv / n_el);
    }
}

// dx = gy * scale + (A + B * (x - mean)) (+ addend) at EVERY element, the zeros included;  ab = NULL: stored statistics
template <bool B8>
__global__ __launch_bounds__(BG_THREADS) void nz_backward_dx_kernel(const float *__restrict__ x, const float *__restrict__ ga,
                                                                   const float *__restrict__ scale, const float *__restrict__ shift,
                                                                   const float *__restrict__ mean, const float *__restrict__ ab,
                                                                   const float *__restrict__ addend, float *__restrict__ dx, int planes,
                                                                   int HW, int vec) {
    constexpr int K = BgItem<B8>::K;
    const BgItem<B8> it = bg_item<B8>(planes, HW, vec);
    if (it.cnt == 0) return;
    const int C = B8 ? planes * 8 : planes;
    float e[K], sc[K], gy[K], o[K];
    bg_load<B8>(it, x, e);
    nz_gate<B8>(it, ga, scale, shift, C, e, sc, gy);
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

// ------------------------------------------------------------------ 5. the partial convolution's epilogue with given factor planes
// out = (raw * ratio + bias[c]) * um (+ residual), fp32 in that order (partialconv2d.py:72-74, blocks.py:248).  out may be raw: a thread
// reads its own elements before it writes them, and neither pointer is declared restrict.
template <bool B8>
__global__ __launch_bounds__(BG_THREADS) void pconv_train_epilogue_kernel(const float *raw, const float *__restrict__ ratio,
                                                                         const float *__restrict__ um, const float *__restrict__ bias,
                                                                         const float *__restrict__ residual, float *out,
                                                                         int planes, int HW, int vec) {
    constexpr int K = BgItem<B8>::K;
    const BgItem<B8> it = bg_item<B8>(planes, HW, vec);
    if (it.cnt == 0) return;
    const int C = B8 ? planes * 8 : planes;
    float e[K], r[K], u[K], b[K];
    bg_load<B8>(it, raw, e);
    bg_mask<B8>(it, ratio, r);
    bg_mask<B8>(it, um, u);
    bg_table<B8>(it, bias, 0, C, b);
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = (e[k] * r[k] + b[k]) * u[k];
    if (residual) {
        float s[K];
        bg_load<B8>(it, residual, s);
#pragma unroll
        for (int k = 0; k < K; ++k) e[k] = e[k] + s[k];
    }
    bg_store<B8>(it, out, e);
}

// ------------------------------------------------------------------ host side
static bool dg_sizes_ok(int N, int C, int H, int W) {
    return N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C * H * W < (1LL << 31) - 4 * BG_THREADS && (long long)N * C <= 65535;
}
static int dg_gx1(int HW, bool b8) { return b8 ? (HW + BG_THREADS - 1) / BG_THREADS : (HW + 4 * BG_THREADS - 1) / (4 * BG_THREADS); }
// workgroups per plane of a reduction kernel (DG_PPT items per thread)
static int dg_gx(int HW, bool b8) { return (dg_gx1(HW, b8) + DG_PPT - 1) / DG_PPT; }
// the partial sums (the blocked form's count; the NCHW form needs no more), the counts, the statistics' coefficients
static size_t dg_part_bytes(int N, int C, int H, int W) { return al256((size_t)N * C * dg_gx(H * W, true) * 2 * sizeof(double)); }
static size_t dg_cpart_bytes(int N, int C, int H, int W) { return al256((size_t)N * C * dg_gx(H * W, true) * sizeof(unsigned)); }
static size_t dg_ws_bytes(int N, int C, int H, int W) {
    return dg_part_bytes(N, C, H, W) + dg_cpart_bytes(N, C, H, W) + al256((size_t)2 * C * sizeof(float));
}
static bool dg_ws_ok(const void *ws, size_t ws_bytes, int N, int C, int H, int W) {
    return ws && !((uintptr_t)ws & 255) && ws_bytes >= dg_ws_bytes(N, C, H, W);
}
static dim3 dg_grid1(int N, int C, int HW, bool b8) { return dim3(dg_gx1(HW, b8), b8 ? N * (C / 8) : N * C); }
static dim3 dg_grid(int N, int C, int HW, bool b8) { return dim3(dg_gx(HW, b8), b8 ? N * (C / 8) : N * C); }

}  // namespace slr

using namespace slr;

#define DG_CHECK_PLANES(C)                                                                                              \
    SLR_CHECK_ARG(dg_sizes_ok(N, C, H, W), "sizes (N * C * H * W < 2^31 - 1024, N * C <= 65535)");                      \
    SLR_CHECK_ARG(b8 == 0 || b8 == 1, "b8");                                                                            \
    SLR_CHECK_ARG(!b8 || C % 8 == 0, "a channel-blocked layout needs C % 8 == 0")

// ------------------------------------------------------------------ C ABI

SLR_EXPORT size_t slr_bn_nonzero_ws_bytes(int N, int C, int H, int W) {
    if (!dg_sizes_ok(N, C, H, W)) return 0;
    return dg_ws_bytes(N, C, H, W);
}

SLR_EXPORT int slr_bn_nonzero_stats(const float *x, float eps, float *mean, float *var, float *count, int N, int C, int H, int W, int b8,
                                    void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(x && mean && var && count, "null pointer");
    DG_CHECK_PLANES(C);
    SLR_CHECK_ARG(eps >= 0.0f, "eps");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)mean | (uintptr_t)var | (uintptr_t)count) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && ((uintptr_t)x & 15)), "16-byte aligned channel-blocked tensors");
    if (!dg_ws_ok(ws, ws_bytes, N, C, H, W)) {
        set_error("%s: ws: slr_bn_nonzero_ws_bytes(N, C, H, W) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, vec = HW % 4 == 0 && !((uintptr_t)x & 15);
    double *part = (double *)ws;
    unsigned *cpart = (unsigned *)((char *)ws + dg_part_bytes(N, C, H, W));
    const dim3 grid = dg_grid(N, C, HW, b8);
    if (b8) hipLaunchKernelGGL(nz_stats_kernel<true>, grid, dim3(BG_THREADS), 0, st, x, part, cpart, C / 8, HW, vec);
    else hipLaunchKernelGGL(nz_stats_kernel<false>, grid, dim3(BG_THREADS), 0, st, x, part, cpart, C, HW, vec);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(nz_stats_final_kernel, dim3(C), dim3(256), 0, st, (const double *)part, (const unsigned *)cpart, mean, var, count, N, C,
                       (int)grid.x, b8, eps);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_nonzero_count_plane(const float *x, float *msum, int N, int C, int H, int W, int b8, void *stream) {
    SLR_CHECK_ARG(x && msum, "null pointer");
    DG_CHECK_PLANES(C);
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)msum) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && ((uintptr_t)x & 15)), "16-byte aligned channel-blocked tensors");
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)msum) & 15);
    const dim3 grid(dg_gx1(HW, b8), N);
    if (b8) hipLaunchKernelGGL(nz_count_plane_kernel<true>, grid, dim3(BG_THREADS), 0, st, x, msum, C, HW, vec);
    else hipLaunchKernelGGL(nz_count_plane_kernel<false>, grid, dim3(BG_THREADS), 0, st, x, msum, C, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_bn_relu_nonzero_train(const float *x, const float *scale, const float *shift, float *a, int N, int C, int H, int W,
                                         int b8, void *stream) {
    SLR_CHECK_ARG(x && scale && shift && a, "null pointer");
    DG_CHECK_PLANES(C);
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)a | (uintptr_t)scale | (uintptr_t)shift) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && (((uintptr_t)x | (uintptr_t)a) & 15)), "16-byte aligned channel-blocked tensors");
    const int HW = H * W, vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)a) & 15);
    const dim3 grid = dg_grid1(N, C, HW, b8);
    hipStream_t st = (hipStream_t)stream;
    if (b8) hipLaunchKernelGGL(nz_forward_kernel<true>, grid, dim3(BG_THREADS), 0, st, x, scale, shift, a, C / 8, HW, vec);
    else hipLaunchKernelGGL(nz_forward_kernel<false>, grid, dim3(BG_THREADS), 0, st, x, scale, shift, a, C, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_bn_relu_nonzero_backward(const float *x, const float *ga, const float *scale, const float *shift, const float *mean,
                                            const float *var, const float *gain, const float *count, float eps, const float *addend,
                                            float *dx, float *dgain, float *dbias, int stored, int N, int C, int H, int W, int b8, void *ws,
                                            size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(x && ga && scale && shift && mean && var, "null pointer");
    SLR_CHECK_ARG(dx || dgain || dbias, "null pointer: nothing to compute");
    SLR_CHECK_ARG(stored == 0 || stored == 1, "stored");
    SLR_CHECK_ARG(stored || count, "null pointer: batch statistics need their counts");
    SLR_CHECK_ARG(!addend || dx, "addend goes with dx");
    DG_CHECK_PLANES(C);
    SLR_CHECK_ARG(eps >= 0.0f, "eps");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)ga | (uintptr_t)addend | (uintptr_t)dx | (uintptr_t)dgain | (uintptr_t)dbias) & 3),
                  "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && (((uintptr_t)x | (uintptr_t)ga | (uintptr_t)addend | (uintptr_t)dx) & 15)), "16-byte aligned channel-blocked tensors");
    const bool reduce = dgain || dbias || !stored;
    if (reduce && !dg_ws_ok(ws, ws_bytes, N, C, H, W)) {
        set_error("%s: ws: slr_bn_nonzero_ws_bytes(N, C, H, W) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    const int vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)ga | (uintptr_t)addend | (uintptr_t)dx) & 15);
    const int planes = b8 ? C / 8 : C;
    float *ab = nullptr;
    if (reduce) {
        double *part = (double *)ws;
        if (dx && !stored) ab = (float *)((char *)ws + dg_part_bytes(N, C, H, W) + dg_cpart_bytes(N, C, H, W));
        const dim3 grid = dg_grid(N, C, HW, b8);
        if (b8) hipLaunchKernelGGL(nz_backward_reduce_kernel<true>, grid, dim3(BG_THREADS), 0, st, x, ga, scale, shift, part, planes, HW, vec);
        else hipLaunchKernelGGL(nz_backward_reduce_kernel<false>, grid, dim3(BG_THREADS), 0, st, x, ga, scale, shift, part, planes, HW, vec);
        SLR_CHECK_LAUNCH();
        hipLaunchKernelGGL(nz_backward_final_kernel, dim3(C), dim3(256), 0, st, (const double *)part, mean, var, gain, count, eps, dgain, dbias,
                           ab, N, C, (int)grid.x, b8, stored);
        SLR_CHECK_LAUNCH();
    }
    if (dx) {
        const dim3 grid = dg_grid1(N, C, HW, b8);
        if (b8) hipLaunchKernelGGL(nz_backward_dx_kernel<true>, grid, dim3(BG_THREADS), 0, st, x, ga, scale, shift, mean, (const float *)ab, addend, dx, planes, HW, vec);
        else hipLaunchKernelGGL(nz_backward_dx_kernel<false>, grid, dim3(BG_THREADS), 0, st, x, ga, scale, shift, mean, (const float *)ab, addend, dx, planes, HW, vec);
        SLR_CHECK_LAUNCH();
    }
    return 0;
}

SLR_EXPORT int slr_pconv_train_epilogue(const float *raw0, const float *ratio, const float *um, const float *bias, const float *residual,
                                        float *out, int N, int C, int H, int W, int b8, void *stream) {
    SLR_CHECK_ARG(raw0 && ratio && um && bias && out, "null pointer");
    DG_CHECK_PLANES(C);
    SLR_CHECK_ARG(!(((uintptr_t)raw0 | (uintptr_t)ratio | (uintptr_t)um | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out) & 3),
                  "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && (((uintptr_t)raw0 | (uintptr_t)residual | (uintptr_t)out) & 15)), "16-byte aligned channel-blocked tensors");
    const int HW = H * W;
    const int vec = HW % 4 == 0 && !(((uintptr_t)raw0 | (uintptr_t)ratio | (uintptr_t)um | (uintptr_t)residual | (uintptr_t)out) & 15);
    const dim3 grid = dg_grid1(N, C, HW, b8);
    hipStream_t st = (hipStream_t)stream;
    if (b8) hipLaunchKernelGGL(pconv_train_epilogue_kernel<true>, grid, dim3(BG_THREADS), 0, st, raw0, ratio, um, bias, residual, out, C / 8, HW, vec);
    else hipLaunchKernelGGL(pconv_train_epilogue_kernel<false>, grid, dim3(BG_THREADS), 0, st, raw0, ratio, um, bias, residual, out, C, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}
