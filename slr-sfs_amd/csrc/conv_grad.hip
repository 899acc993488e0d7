// conv_grad.hip -- the gradients a 3x3 / stride 1 / zero-pad 1 convolution needs to learn (ABI 15): what torch autograd computes for
// nn.Conv2d in models/layers/blocks.py:66-87 and for PartialConv2d in models/layers/partialconv2d.py:61-74.
//   * weight gradient  dW[co][ci][ky][kx] = sum_{n,y,x} G[n,co,y,x] * X[n,ci,y+ky-1,x+kx-1]: an implicit GEMM with M = Cout, N = 9 Cin and
//     K = N H W (the pixels) on v_mfma_f32_32x32x2_f32 -- fp32 operands, fp32 products, fp32 accumulation, the arithmetic of the fp32 rung.
//     A workgroup of four waves owns 64 co x 64 ci x 9 taps (a wave: 32 x 32 x 9 = 144 accumulator registers) over a SLAB of the pixels;
//     one G fragment serves the nine taps, the nine X operands are the same staged tile read at nine offsets.  Every slab writes its
//     partial sums to the workspace; a second launch adds the slabs in a fixed order (in double).  No atomics: the same inputs and the
//     same split count give the same bits from run to run.
//   * one bandwidth-bound pass over G: Gr = G * r (the per-pixel factor ratio * um of a partial convolution, feeding the backward-data
//     convolution and the weight gradient) and the bias gradient's partial sums of G * um, in double (slr_reduce.hpp), added in a fixed order
//     by a second launch.  Without r / um it is the bias gradient of the plain convolution.
// X and G are each read NCHW or channel-blocked ([N,C/8,H,W,8], 16-byte accesses).  The backward-data convolution is the forward kernel
// with flipped, transposed weights (csrc/conv.hip); nothing here synchronises.
#include "slr_common.hpp"
#include "slr_reduce.hpp"

namespace slr {


constexpr int WG_THREADS = 256;
constexpr int WG_TC = 64;                              // channels of G and of X per workgroup (two 32-channel MFMA tiles each)
constexpr int WG_RH = 2, WG_CW = 32;                   // a chunk: 2 rows x 32 columns of G pixels ...
constexpr int WG_GPIX = WG_RH * WG_CW;
constexpr int WG_XW = WG_CW + 2, WG_XPIX = (WG_RH + 2) * WG_XW;      // ... and its 4 x 34 halo block of X
// Staged tiles are [32-channel tile][pixel][channel]: lane l of an MFMA operand reads channel l & 31 of pixel p + (l >> 5), i.e. 32
// consecutive words per half.  Pixel stride 32 (blocked tensors: 16-byte stores, the halves on disjoint banks) or 33 (NCHW tensors: the
// staging stores of consecutive pixels fall on consecutive banks; the halves share one bank).
constexpr int wg_stride(bool b8) { return b8 ? 32 : 33; }

// Staging of PIX pixels (a block of PW columns from (y0, x0)) of WG_TC channels from c0 of image n into t[2][PIX][PS], in two halves so
// that the loads of the next chunk are in flight while the matrix pipe works on this one: wg_load into registers (outside the image or
// past the last channel: zeros), wg_store from them into LDS.  A thread's items are threadIdx.x + k * WG_THREADS: 8 channels of a pixel
// (blocked) or one value (NCHW).
template <bool B8, int PIX> struct WgRegs {
    static constexpr int ITEMS = (PIX * (B8 ? WG_TC / 8 : WG_TC) + WG_THREADS - 1) / WG_THREADS;
    float4 v[B8 ? ITEMS * 2 : 1];
    float f[B8 ? 1 : ITEMS];
};

template <bool B8, int PIX, int PW>
__device__ __forceinline__ void wg_load(WgRegs<B8, PIX> &rg, const float *__restrict__ src, int n, int C, int c0, int H, int W, int y0,
                                        int x0) {
    constexpr int ITEMS = WgRegs<B8, PIX>::ITEMS;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int item = threadIdx.x + k * WG_THREADS;
        const int c = item / PIX, pix = item - c * PIX;              // (c: a group of 8 channels for blocked tensors)
        const int py = pix / PW, px = pix - py * PW;
        const int y = y0 + py, x = x0 + px;
        const bool in = y >= 0 && y < H && x >= 0 && x < W && item < PIX * (B8 ? WG_TC / 8 : WG_TC);
        if (B8) {
            const int G8 = C >> 3, cg = (c0 >> 3) + c;
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
            if (in && cg < G8) {
                const float4 *p = (const float4 *)(src + ((((size_t)n * G8 + cg) * H + y) * W + x) * 8);
                a = p[0]; b = p[1];
            }
            rg.v[2 * k] = a; rg.v[2 * k + 1] = b;
        } else {
            float v = 0.0f;
            if (in && c0 + c < C) v = src[(((size_t)n * C + c0 + c) * H + y) * W + x];
            rg.f[k] = v;
        }
    }
}

template <bool B8, int PIX>
__device__ __forceinline__ void wg_store(float *__restrict__ t, const WgRegs<B8, PIX> &rg) {
    constexpr int PS = wg_stride(B8), ITEMS = WgRegs<B8, PIX>::ITEMS;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int item = threadIdx.x + k * WG_THREADS;
        if (item < PIX * (B8 ? WG_TC / 8 : WG_TC)) {
            const int c = item / PIX, pix = item - c * PIX;
            if (B8) {
                float4 *d = (float4 *)(t + ((c >> 2) * PIX + pix) * PS + (c & 3) * 8);
                d[0] = rg.v[2 * k]; d[1] = rg.v[2 * k + 1];
            } else {
                t[((c >> 5) * PIX + pix) * PS + (c & 31)] = rg.f[k];
            }
        }
    }
}

// grid (splits, ci tiles, co tiles).  Slab s takes the chunks [s T / S, (s + 1) T / S) of the T = N * ceil(H / 2) * ceil(W / 32) chunks in
// row-major order and writes part[s][tap][co][ci].  One wave per SIMD: 144 accumulator registers + the next chunk's staging registers
// (310 - 492 in all); the split rule launches about one workgroup per CU, so a second resident workgroup would rarely exist anyway.
template <bool XB8, bool GB8, bool EDGE>
__global__ __launch_bounds__(WG_THREADS, 1) void conv3x3_wgrad_kernel(const float *__restrict__ X, const float *__restrict__ G,
                                                                       float *__restrict__ part, int N, int Cin, int Cout, int H, int W,
                                                                       int chunks, int CY, int CX) {
    constexpr int PSX = wg_stride(XB8), PSG = wg_stride(GB8);
    __shared__ __attribute__((aligned(16))) float gs[2 * WG_GPIX * PSG];
    __shared__ __attribute__((aligned(16))) float xs[2 * WG_XPIX * PSX];
    const int s = blockIdx.x, S = gridDim.x, ci0 = blockIdx.y * WG_TC, co0 = blockIdx.z * WG_TC;
    const int first = (int)((long long)s * chunks / S), last = (int)((long long)(s + 1) * chunks / S);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tco = wave >> 1, tci = wave & 1;
    const int c = lane & 31, h = lane >> 5;
    const float *ga = gs + tco * WG_GPIX * PSG + h * PSG + c;
    const float *xa = xs + tci * WG_XPIX * PSX + h * PSX + c;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    WgRegs<GB8, WG_GPIX> rg_g;
    WgRegs<XB8, WG_XPIX> rg_x;
    const int per_image = CY * CX;
    auto load_chunk = [&](int ch) {
        const int n = ch / per_image, rem = ch - n * per_image, cy = rem / CX, cx = rem - cy * CX;
        wg_load<GB8, WG_GPIX, WG_CW>(rg_g, G, n, Cout, co0, H, W, cy * WG_RH, cx * WG_CW);
        wg_load<XB8, WG_XPIX, WG_XW>(rg_x, X, n, Cin, ci0, H, W, cy * WG_RH - 1, cx * WG_CW - 1);
    };
    load_chunk(first);                                   // (host: at most one slab per chunk, so first < last)
    for (int ch = first; ch < last; ++ch) {
        __syncthreads();                                 // (the previous chunk's reads are done)
        wg_store<GB8, WG_GPIX>(gs, rg_g);
        wg_store<XB8, WG_XPIX>(xs, rg_x);
        __syncthreads();
        if (ch + 1 < last) load_chunk(ch + 1);           // in flight during the MFMAs below
        // a k step = the pixel pair (x, x + 1) of one row; tap (ky, kx) reads X at row + ky, column + kx of the halo block.  The kx = 2
        // operand of a pair is the kx = 0 operand of the next one.  A G pixel of the chunk that lies outside the image is no term of the
        // sum: its G is zero, and its X operands are SELECTED to zero too -- they are real elements of X (the halo of the image's last
        // rows and columns), and 0 x NaN on the matrix core would put a NaN of theirs into taps it has no part in.  EDGE = false (the
        // host: H % 2 == 0 and W % 32 == 0, no chunk reaches past the image) compiles the selects away: in this loop they cost 19 %.
        const int rem = ch % per_image, cy = rem / CX, cx = rem - cy * CX;
        const int rows_in = H - cy * WG_RH, cols_in = W - cx * WG_CW - h;    // this lane's pixel (ry, 2 xp + h) is inside iff ry < rows_in, 2 xp < cols_in
#pragma unroll
        for (int ry = 0; ry < WG_RH; ++ry) {
            float carry[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) carry[ky] = xa[((ry + ky) * WG_XW) * PSX];
#pragma unroll
            for (int xp = 0; xp < WG_CW / 2; ++xp) {
                const float a = ga[(ry * WG_CW + 2 * xp) * PSG];
                const bool in = !EDGE || (ry < rows_in && 2 * xp < cols_in);
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const float b1 = xa[((ry + ky) * WG_XW + 2 * xp + 1) * PSX];
                    const float b2 = xa[((ry + ky) * WG_XW + 2 * xp + 2) * PSX];
                    const float s0 = in ? carry[ky] : 0.0f, s1 = in ? b1 : 0.0f, s2 = in ? b2 : 0.0f;
                    carry[ky] = b2;
                    acc[ky * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s0, acc[ky * 3 + 0], 0, 0, 0);
                    acc[ky * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s1, acc[ky * 3 + 1], 0, 0, 0);
                    acc[ky * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s2, acc[ky * 3 + 2], 0, 0, 0);
                }
            }
        }
    }
    // D[row = co][column = ci]: the column on the lane, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in register r
    const int ci = ci0 + tci * 32 + c;
    if (ci < Cin) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + tco * 32 + mfma32_row(r, h);
                if (co < Cout) part[(((size_t)s * 9 + t) * Cout + co) * Cin + ci] = acc[t][r];
            }
    }
}

// dW[co][ci][tap] = sum_s part[s][tap][co][ci]: 64 elements x 4 ranges of slabs per workgroup, each range in slab order, the four in order.
__global__ __launch_bounds__(256) void conv3x3_wgrad_sum_kernel(const float *__restrict__ part, float *__restrict__ dw, int S, int Cout,
                                                                int Cin) {
    __shared__ double red[4][64];
    const int total = 9 * Cout * Cin, e = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    double v = 0.0;
    if (e < total)
        for (int s = q * S / 4; s < (q + 1) * S / 4; ++s) v += (double)part[(size_t)s * total + e];
    red[q][threadIdx.x & 63] = v;
    __syncthreads();
    if (q == 0 && e < total) {
        const double sum = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        const int tap = e / (Cout * Cin), r = e - tap * (Cout * Cin);
        dw[(size_t)r * 9 + tap] = (float)sum;
    }
}

// ------------------------------------------------------------------ Gr = G * r, bias-gradient partial sums of G * um
// Blocked: grid (GX, N * C / 8), a thread = 8 channels of one pixel, part[(n * C / 8 + cg) * GX + bx][8].
// NCHW:    grid (GX, N * C), a thread = 4 consecutive pixels of a plane, part[(n * C + c) * GX + bx].
template <bool B8>
__global__ __launch_bounds__(WG_THREADS) void conv_grad_scale_bias_kernel(const float *__restrict__ g, const float *__restrict__ r,
                                                                          const float *__restrict__ um, float *__restrict__ gr,
                                                                          double *__restrict__ part, int planes, int HW, int vec) {
    constexpr int K = B8 ? 8 : 1;
    __shared__ double red[K][WG_THREADS / 64];
    const int n = blockIdx.y / planes;
    const size_t base = (size_t)blockIdx.y * HW, pbase = (size_t)n * HW;
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    if (B8) {
        const int p = blockIdx.x * WG_THREADS + threadIdx.x;
        if (p < HW) {
            const float rr = r ? r[pbase + p] : 1.0f, uu = um ? um[pbase + p] : 1.0f;
            const float4 *src = (const float4 *)(g + (base + p) * 8);
            const float4 a = src[0], b = src[1];
            const float e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (double)(e[k] * uu);
            if (gr) {
                float4 *dst = (float4 *)(gr + (base + p) * 8);
                dst[0] = make_float4(a.x * rr, a.y * rr, a.z * rr, a.w * rr);
                dst[1] = make_float4(b.x * rr, b.y * rr, b.z * rr, b.w * rr);
            }
        }
    } else {
        const int p0 = (blockIdx.x * WG_THREADS + threadIdx.x) * 4;
        const int cnt = HW - p0 >= 4 ? 4 : HW - p0 > 0 ? HW - p0 : 0;
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rr[4] = {1.0f, 1.0f, 1.0f, 1.0f}, uu[4] = {1.0f, 1.0f, 1.0f, 1.0f}, o[4];
        const bool v4 = vec && cnt == 4;                 // (vec: HW % 4 == 0 and every tensor 16-byte aligned)
        if (v4) {
            const float4 a = *(const float4 *)(g + base + p0);
            e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w;
            if (r) { const float4 q = *(const float4 *)(r + pbase + p0); rr[0] = q.x; rr[1] = q.y; rr[2] = q.z; rr[3] = q.w; }
            if (um) { const float4 q = *(const float4 *)(um + pbase + p0); uu[0] = q.x; uu[1] = q.y; uu[2] = q.z; uu[3] = q.w; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) {
                    e[k] = g[base + p0 + k];
                    if (r) rr[k] = r[pbase + p0 + k];
                    if (um) uu[k] = um[pbase + p0 + k];
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {                    // (past the end: e = 0)
            v[0] += (double)(e[k] * uu[k]);
            o[k] = e[k] * rr[k];
        }
        if (gr) {
            if (v4) *(float4 *)(gr + base + p0) = make_float4(o[0], o[1], o[2], o[3]);
            else
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) gr[base + p0 + k] = o[k];
        }
    }
    if (part) {                                          // (uniform over the grid)
        block_sum<K, WG_THREADS / 64>(v, red);
        if (threadIdx.x == 0)
#pragma unroll
            for (int k = 0; k < K; ++k) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * K + k] = v[k];
    }
}

// db[c] = the partial sums of channel c in the order (n, bx): one workgroup per channel.
__global__ __launch_bounds__(256) void conv_grad_bias_sum_kernel(const double *__restrict__ part, float *__restrict__ db, int N, int C,
                                                                 int GX, int b8) {
    __shared__ double red[1][4];
    const int c = blockIdx.x;
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < N * GX; i += 256) {
        const int n = i / GX, bx = i - n * GX;
        v[0] += b8 ? part[(((size_t)n * (C >> 3) + (c >> 3)) * GX + bx) * 8 + (c & 7)] : part[((size_t)n * C + c) * GX + bx];
    }
    block_sum<1, 4>(v, red);
    if (threadIdx.x == 0) db[c] = (float)v[0];
}

static long long wg_chunks(int N, int H, int W) { return (long long)N * ((H + WG_RH - 1) / WG_RH) * ((W + WG_CW - 1) / WG_CW); }
static int wg_tiles(int C) { return (C + WG_TC - 1) / WG_TC; }
static size_t wg_bias_bytes(int N, int C, int H, int W) {      // (the blocked form's count; the NCHW form needs a quarter)
    return al256((size_t)N * C * (((size_t)H * W + WG_THREADS - 1) / WG_THREADS) * sizeof(double));
}
static int wg_splits(int N, int Cin, int Cout, int H, int W, int splits) {
    const long long chunks = wg_chunks(N, H, W);
    long long S = splits > 0 ? splits : slr_wgrad_auto_splits(chunks, wg_tiles(Cin) * wg_tiles(Cout), (long long)Cout * Cin * 9 * 4);
    return (int)(S < chunks ? S : chunks);
}
static bool wg_sizes_ok(int N, int Cin, int Cout, int H, int W) {
    return N > 0 && Cin >= 0 && Cout > 0 && H > 0 && W > 0 && Cin <= 65535 * 64 && Cout <= 65535 * 64 &&
           (long long)N * (Cin > Cout ? Cin : Cout) * H * W < (1LL << 31) - 4 * WG_THREADS && (long long)N * Cout <= 65535 &&
           9LL * Cout * Cin < (1LL << 31) - 64;     // (a thread's first pixel, rounded up to a workgroup of 4-pixel items, and the sum kernel's element stay an int)
}

static int wg_scale_bias(const float *g, const float *r, const float *um, float *gr, float *db, int N, int C, int H, int W, int b8,
                         double *part, hipStream_t st) {
    const int HW = H * W;
    const int vec = HW % 4 == 0 && !(((uintptr_t)g | (uintptr_t)r | (uintptr_t)um | (uintptr_t)gr) & 15);
    const int GX = b8 ? (HW + WG_THREADS - 1) / WG_THREADS : (HW + 4 * WG_THREADS - 1) / (4 * WG_THREADS);
    double *p = db ? part : nullptr;
    if (b8) hipLaunchKernelGGL(conv_grad_scale_bias_kernel<true>, dim3(GX, N * (C / 8)), dim3(WG_THREADS), 0, st, g, r, um, gr, p, C / 8, HW, vec);
    else hipLaunchKernelGGL(conv_grad_scale_bias_kernel<false>, dim3(GX, N * C), dim3(WG_THREADS), 0, st, g, r, um, gr, p, C, HW, vec);
    SLR_CHECK_LAUNCH();
    if (db) {
        hipLaunchKernelGGL(conv_grad_bias_sum_kernel, dim3(C), dim3(256), 0, st, (const double *)part, db, N, C, GX, b8);
        SLR_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT size_t slr_conv3x3_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int splits) {
    if (!wg_sizes_ok(N, Cin, Cout, H, W) || splits < 0) return 0;
    const size_t bias = wg_bias_bytes(N, Cout, H, W);
    if (Cin == 0) return bias;
    return bias + al256((size_t)wg_splits(N, Cin, Cout, H, W, splits) * 9 * Cout * Cin * sizeof(float));
}

SLR_EXPORT int slr_conv3x3_weight_grad(const float *x, const float *g, float *dw, float *db, int N, int Cin, int Cout, int H, int W,
                                       int splits, int layout, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(x && g && dw, "null pointer");
    SLR_CHECK_ARG(Cin > 0 && wg_sizes_ok(N, Cin, Cout, H, W), "sizes (N * max(Cin, Cout) * H * W < 2^31 - 1024, N * Cout <= 65535, 9 * Cout * Cin < 2^31 - 64)");
    SLR_CHECK_ARG(splits >= 0, "splits (0 = chosen by the library)");
    SLR_CHECK_ARG(!(layout & ~(SLR_GRAD_X_B8 | SLR_GRAD_G_B8)), "layout");
    const bool xb8 = layout & SLR_GRAD_X_B8, gb8 = layout & SLR_GRAD_G_B8;
    SLR_CHECK_ARG(!xb8 || Cin % 8 == 0, "SLR_GRAD_X_B8 needs Cin % 8 == 0");
    SLR_CHECK_ARG(!gb8 || Cout % 8 == 0, "SLR_GRAD_G_B8 needs Cout % 8 == 0");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)g | (uintptr_t)dw | (uintptr_t)db) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(!(xb8 && ((uintptr_t)x & 15)) && !(gb8 && ((uintptr_t)g & 15)), "16-byte aligned channel-blocked tensors");
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < slr_conv3x3_grad_ws_bytes(N, Cin, Cout, H, W, splits)) {
        set_error("%s: ws: slr_conv3x3_grad_ws_bytes(N, Cin, Cout, H, W, splits) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int S = wg_splits(N, Cin, Cout, H, W, splits);
    float *part = (float *)((char *)ws + wg_bias_bytes(N, Cout, H, W));
    const dim3 grid(S, wg_tiles(Cin), wg_tiles(Cout));
    const int chunks = (int)wg_chunks(N, H, W), CY = (H + WG_RH - 1) / WG_RH, CX = (W + WG_CW - 1) / WG_CW;
    const bool edge = H % WG_RH != 0 || W % WG_CW != 0;  // some chunk reaches past the image
#define SLR_WGRAD_LAUNCH(XB, GB)                                                                                                              \
    do {                                                                                                                                      \
        if (edge) hipLaunchKernelGGL((conv3x3_wgrad_kernel<XB, GB, true>), grid, dim3(WG_THREADS), 0, st, x, g, part, N, Cin, Cout, H, W,    \
                                     chunks, CY, CX);                                                                                         \
        else hipLaunchKernelGGL((conv3x3_wgrad_kernel<XB, GB, false>), grid, dim3(WG_THREADS), 0, st, x, g, part, N, Cin, Cout, H, W,        \
                                chunks, CY, CX);                                                                                              \
    } while (0)
    if (xb8 && gb8) SLR_WGRAD_LAUNCH(true, true);
    else if (xb8) SLR_WGRAD_LAUNCH(true, false);
    else if (gb8) SLR_WGRAD_LAUNCH(false, true);
    else SLR_WGRAD_LAUNCH(false, false);
#undef SLR_WGRAD_LAUNCH
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(conv3x3_wgrad_sum_kernel, dim3((9 * Cout * Cin + 63) / 64), dim3(256), 0, st, (const float *)part, dw, S, Cout, Cin);
    SLR_CHECK_LAUNCH();
    if (db) return wg_scale_bias(g, nullptr, nullptr, nullptr, db, N, Cout, H, W, gb8, (double *)ws, st);
    return 0;
}

SLR_EXPORT int slr_conv_grad_scale_bias(const float *g, const float *r, const float *um, float *gr, float *db, int N, int C, int H, int W,
                                        int layout, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(g && (gr || db), "null pointer");
    SLR_CHECK_ARG(!gr || r, "null pointer: gr needs r");
    SLR_CHECK_ARG(wg_sizes_ok(N, 0, C, H, W), "sizes (N * C * H * W < 2^31 - 1024, N * C <= 65535)");
    SLR_CHECK_ARG(!(layout & ~SLR_GRAD_G_B8), "layout");
    const bool b8 = layout & SLR_GRAD_G_B8;
    SLR_CHECK_ARG(!b8 || C % 8 == 0, "SLR_GRAD_G_B8 needs C % 8 == 0");
    SLR_CHECK_ARG(!(((uintptr_t)g | (uintptr_t)r | (uintptr_t)um | (uintptr_t)gr | (uintptr_t)db) & 3), "4-byte aligned tensors");
    SLR_CHECK_ARG(!(b8 && (((uintptr_t)g | (uintptr_t)gr) & 15)), "16-byte aligned channel-blocked tensors");
    if (db && (!ws || ((uintptr_t)ws & 255) || ws_bytes < wg_bias_bytes(N, C, H, W))) {
        set_error("%s: ws: slr_conv3x3_grad_ws_bytes(N, 0, C, H, W, 0) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    return wg_scale_bias(g, r, um, gr, db, N, C, H, W, b8, (double *)ws, (hipStream_t)stream);
}
