// block_items.hpp -- what a thread of a plane pass owns, shared by csrc/block_grad.hip and csrc/decoder_grad.hip: the elements of an
// [N,C,H,W] tensor in either layout, the mask and table values that go with them, and where a workgroup's partial sums lie.
#pragma once
#include <type_traits>
#include "slr_common.hpp"

namespace slr {

constexpr int BG_THREADS = 256;

// ------------------------------------------------------------------ a thread's elements of a plane pass
// Blocked: a thread's item = the 8 channels of one pixel (two 16-byte accesses); grid (ceil(HW / (256 PPT)), N * C / 8).
// NCHW:    a thread's item = 4 consecutive pixels of one plane (one 16-byte access where `vec` allows); grid (ceil(HW / (1024 PPT)), N * C).
template <bool B8> struct BgItem {
    static constexpr int K = B8 ? 8 : 4;
    int n, c0, cnt;            // image, first channel, valid elements (blocked: 8 or 0)
    bool v4;                   // NCHW: the four pixels as one 16-byte access
    size_t off, moff;          // offset in an [N,C,H,W] tensor of this layout / in an [N,1,H,W] plane
};

// The thread's j-th item of PPT: workgroup bx owns the items [bx * PPT * 256, (bx + 1) * PPT * 256) of its plane, item (j * 256 + thread) of
// them; consecutive threads stay on consecutive addresses.  Items past the plane have cnt = 0, and nothing follows them: a thread's items
// go up the plane.  The elementwise kernels take one item per thread, the reductions the PPT of their mask kind (csrc/block_grad.hip).
template <bool B8, int PPT = 1> __device__ __forceinline__ BgItem<B8> bg_item(int planes, int HW, int vec, int j = 0) {
    BgItem<B8> it;
    const int plane = blockIdx.y;
    it.n = plane / planes;
    const int cp = plane - it.n * planes;
    // One item per thread: the position stays an int (bg_sizes_ok).  With more, the last workgroup's items can lie past 2^31, and their
    // offsets are not formed.
    using Pos = std::conditional_t<PPT == 1, int, long long>;
    const Pos p = ((Pos)(blockIdx.x * PPT + j) * BG_THREADS + threadIdx.x) * (B8 ? 1 : 4);
    const Pos left = (Pos)HW - p;
    it.c0 = B8 ? cp * 8 : cp;
    it.cnt = B8 ? (left > 0 ? 8 : 0) : (left >= 4 ? 4 : left > 0 ? (int)left : 0);
    it.v4 = !B8 && vec && it.cnt == 4;
    const bool in = PPT == 1 || it.cnt;
    it.off = in ? (B8 ? ((size_t)plane * HW + (size_t)p) * 8 : (size_t)plane * HW + (size_t)p) : 0;
    it.moff = in ? (size_t)it.n * HW + (size_t)p : 0;
    return it;
}

// A thread's items in turn: item(j) returns false where nothing follows.  One item is a plain call and no loop: the one-item kernels
// then compile to the straight code they were before they shared their text with the many-item ones.
template <int PPT, class F> __device__ __forceinline__ void bg_items(F &&item) {
    if constexpr (PPT == 1) item(0);
    else
#pragma unroll 2
        for (int j = 0; j < PPT; ++j)
            if (!item(j)) break;
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

// ------------------------------------------------------------------ host side: sizes and grids
inline bool bg_sizes_ok(int N, int C, int H, int W) {
    return N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C * H * W < (1LL << 31) - 4 * BG_THREADS && (long long)N * C <= 65535;       // (a thread's first pixel, rounded up to a workgroup of 4-pixel items, stays an int)
}
// workgroups per plane: an elementwise kernel (one item per thread) or a reduction with ppt items per thread
inline int bg_gx(int HW, bool b8, int ppt = 1) {
    const int per = BG_THREADS * ppt * (b8 ? 1 : 4);
    return (int)(((long long)HW + per - 1) / per);
}
inline dim3 bg_grid(int N, int C, int HW, bool b8, int ppt = 1) { return dim3(bg_gx(HW, b8, ppt), b8 ? N * (C / 8) : N * C); }

// The checks every export on [N,C,H,W] planes opens with; `fn`: the export's name
#define BG_CHECK_PLANES(fn, C)                                                                                          \
    SLR_CHECK_ARG_FN(fn, slr::bg_sizes_ok(N, C, H, W), "sizes (N * C * H * W < 2^31 - 1024, N * C <= 65535)");          \
    SLR_CHECK_ARG_FN(fn, b8 == 0 || b8 == 1, "b8");                                                                     \
    SLR_CHECK_ARG_FN(fn, !b8 || C % 8 == 0, "a channel-blocked layout needs C % 8 == 0")

// ------------------------------------------------------------------ a workgroup's partial sums
// The two partial sums of channel c, image n, workgroup bx
__device__ __forceinline__ const double *bg_part(const double *part, int n, int c, int bx, int C, int GX, int b8) {
    return b8 ? part + (((size_t)n * (C >> 3) + (c >> 3)) * GX + bx) * 16 + (c & 7) * 2 : part + (((size_t)n * C + c) * GX + bx) * 2;
}

// The workgroup's count of channel c, image n, workgroup bx (the layout of bg_part with one value per channel)
__device__ __forceinline__ unsigned bg_cpart(const unsigned *cpart, int n, int c, int bx, int C, int GX, int b8) {
    return b8 ? cpart[(((size_t)n * (C >> 3) + (c >> 3)) * GX + bx) * 8 + (c & 7)] : cpart[((size_t)n * C + c) * GX + bx];
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

}  // namespace slr
