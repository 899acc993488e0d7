// decoder_grad.hip -- what the decoder's FIRST block needs to learn beyond csrc/block_grad.hip (ABI 17): ResNet_Block_Pconv2 called with the
// per-element mask (x != 0) of models/networks/architectures.py:369.  The mask k = [x != 0] is never a tensor: every kernel recomputes it
// from x, as the ReLU gate already is.  The batch-norm with this mask -- statistics, forward, backward -- is the nonzero mask kind of the
// one batch-norm family in csrc/block_grad.hip, where its four exports live; what is left here is what only the per-element mask needs:
//   * msum[n,1,h,w] = sum_c k: what the partial convolution behind the BN needs of the mask (partialconv2d.py:61-72), exact integers.
//   * the partial convolution's epilogue with given factor planes: out = (raw * ratio + bias) * um (+ residual).
// Both layouts, no atomics.  Nothing here synchronises.
#include "slr_common.hpp"
#include "block_items.hpp"

namespace slr {

// ------------------------------------------------------------------ 1. the mask as the partial convolution sees it
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

// ------------------------------------------------------------------ 2. the partial convolution's epilogue with given factor planes
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

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT int slr_nonzero_count_plane(const float *x, float *msum, int N, int C, int H, int W, int b8, void *stream) {
    SLR_CHECK_ARG(x && msum, "null pointer");
    BG_CHECK_PLANES(__func__, C);
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)msum) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && ((uintptr_t)x & 15)), "16-byte aligned channel-blocked tensors");
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, vec = HW % 4 == 0 && !(((uintptr_t)x | (uintptr_t)msum) & 15);
    const dim3 grid(bg_gx(HW, b8), N);
    if (b8) hipLaunchKernelGGL(nz_count_plane_kernel<true>, grid, dim3(BG_THREADS), 0, st, x, msum, C, HW, vec);
    else hipLaunchKernelGGL(nz_count_plane_kernel<false>, grid, dim3(BG_THREADS), 0, st, x, msum, C, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_pconv_train_epilogue(const float *raw0, const float *ratio, const float *um, const float *bias, const float *residual,
                                        float *out, int N, int C, int H, int W, int b8, void *stream) {
    SLR_CHECK_ARG(raw0 && ratio && um && bias && out, "null pointer");
    BG_CHECK_PLANES(__func__, C);
    SLR_CHECK_ARG(!(((uintptr_t)raw0 | (uintptr_t)ratio | (uintptr_t)um | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out) & 3),
                  "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && (((uintptr_t)raw0 | (uintptr_t)residual | (uintptr_t)out) & 15)), "16-byte aligned channel-blocked tensors");
    const int HW = H * W;
    const int vec = HW % 4 == 0 && !(((uintptr_t)raw0 | (uintptr_t)ratio | (uintptr_t)um | (uintptr_t)residual | (uintptr_t)out) & 15);
    const dim3 grid = bg_grid(N, C, HW, b8);
    hipStream_t st = (hipStream_t)stream;
    if (b8) hipLaunchKernelGGL(pconv_train_epilogue_kernel<true>, grid, dim3(BG_THREADS), 0, st, raw0, ratio, um, bias, residual, out, C / 8, HW, vec);
    else hipLaunchKernelGGL(pconv_train_epilogue_kernel<false>, grid, dim3(BG_THREADS), 0, st, raw0, ratio, um, bias, residual, out, C, HW, vec);
    SLR_CHECK_LAUNCH();
    return 0;
}
