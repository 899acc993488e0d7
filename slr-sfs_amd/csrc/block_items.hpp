// block_items.hpp -- what a thread of a plane pass owns, shared by csrc/block_grad.hip and csrc/decoder_grad.hip: the elements of an
// [N,C,H,W] tensor in either layout, the mask and table values that go with them, and where a workgroup's partial sums lie.
#pragma once
#include "slr_common.hpp"

namespace slr {

constexpr int BG_THREADS = 256;

// ------------------------------------------------------------------ a thread's elements of a plane pass
// Blocked: grid (ceil(HW / 256), N * C / 8), a thread = the 8 channels of one pixel (two 16-byte accesses).
// NCHW:    grid (ceil(HW / 1024), N * C), a thread = 4 consecutive pixels of one plane (one 16-byte access where `vec` allows).
template <bool B8> struct BgItem {
    static constexpr int K = B8 ? 8 : 4;
    int n, c0, cnt;            // image, first channel, valid elements (blocked: 8 or 0)
    bool v4;                   // NCHW: the four pixels as one 16-byte access
    size_t off, moff;          // offset in an [N,C,H,W] tensor of this layout / in an [N,1,H,W] plane
};

template <bool B8> __device__ __forceinline__ BgItem<B8> bg_item(int planes, int HW, int vec) {
    BgItem<B8> it;
    const int plane = blockIdx.y;
    it.n = plane / planes;
    const int cp = plane - it.n * planes;
    const int p = (blockIdx.x * BG_THREADS + threadIdx.x) * (B8 ? 1 : 4);
    const int left = HW - p;
    it.c0 = B8 ? cp * 8 : cp;
    it.cnt = B8 ? (left > 0 ? 8 : 0) : (left >= 4 ? 4 : left > 0 ? left : 0);
    it.v4 = !B8 && vec && it.cnt == 4;
    it.off = B8 ? ((size_t)plane * HW + p) * 8 : (size_t)plane * HW + p;
    it.moff = (size_t)it.n * HW + p;
    return it;
}

template <bool B8> __device__ __forceinline__ void bg_load(const BgItem<B8> &it, const float *__restrict__ t, float (&e)[BgItem<B8>::K]) {
    constexpr int K = BgItem<B8>::K;
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = 0.0f;
    if (it.cnt == 0) return;
    if constexpr (B8) {
        const float4 *q = (const float4 *)(t + it.off);
        const float4 a = q[0], b = q[1];
        e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w;
        e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
    } else if (it.v4) {
        const float4 a = *(const float4 *)(t + it.off);
        e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < it.cnt) e[k] = t[it.off + k];
    }
}

template <bool B8> __device__ __forceinline__ void bg_store(const BgItem<B8> &it, float *__restrict__ t, const float (&e)[BgItem<B8>::K]) {
    if (it.cnt == 0) return;
    if constexpr (B8) {
        float4 *q = (float4 *)(t + it.off);
        q[0] = make_float4(e[0], e[1], e[2], e[3]);
        q[1] = make_float4(e[4], e[5], e[6], e[7]);
    } else if (it.v4) {
        *(float4 *)(t + it.off) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < it.cnt) t[it.off + k] = e[k];
    }
}

// The channel-uniform mask [N,1,H,W] at the thread's elements (no mask: 1); elements past the plane get 0.
template <bool B8> __device__ __forceinline__ void bg_mask(const BgItem<B8> &it, const float *__restrict__ mask, float (&m)[BgItem<B8>::K]) {
    constexpr int K = BgItem<B8>::K;
    if (B8) {
        const float v = it.cnt == 0 ? 0.0f : mask ? mask[it.moff] : 1.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) m[k] = v;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) m[k] = (k < it.cnt && !mask) ? 1.0f : 0.0f;
        if (!mask || it.cnt == 0) return;
        if (it.v4) {
            const float4 a = *(const float4 *)(mask + it.moff);
            m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < it.cnt) m[k] = mask[it.moff + k];
        }
    }
}

// A table's values at the thread's elements: tab[row * C + c] (row = the image for [N,C] tables, 0 for per-channel ones).
template <bool B8> __device__ __forceinline__ void bg_table(const BgItem<B8> &it, const float *__restrict__ tab, int row, int C,
                                                            float (&v)[BgItem<B8>::K]) {
    constexpr int K = BgItem<B8>::K;
    const float *p = tab + (size_t)row * C + it.c0;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = B8 ? p[k] : p[0];
}

// The two partial sums of channel c, image n, workgroup bx
__device__ __forceinline__ const double *bg_part(const double *part, int n, int c, int bx, int C, int GX, int b8) {
    return b8 ? part + (((size_t)n * (C >> 3) + (c >> 3)) * GX + bx) * 16 + (c & 7) * 2 : part + (((size_t)n * C + c) * GX + bx) * 2;
}

}  // namespace slr
