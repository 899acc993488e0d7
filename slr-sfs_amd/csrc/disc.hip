// disc.hip -- the kernels of the adversarial loss (ABI 18): the multiscale PatchGAN discriminator of the reference's trainer
// (models/networks/discriminators.py:78-139 NLayerDiscriminator, :142-207 MultiscaleDiscriminator; models/layers/normalization.py:95-130
// get_D_norm_layer "spectralinstance"), forward and backward.  Everything is NCHW fp32; nothing synchronises; no atomics -- every long sum
// runs in a fixed order in double (slr_reduce.hpp), so the same inputs give the same bits.
//   * Conv2d(Cin, Cout, 4, stride 1 or 2, padding 2) and its gradient to the input: conv4x4_kernel of csrc/conv4x4.hip, the body the
//     motion U-Nets' encoder convolution runs on;
//   * its weight gradient on v_mfma_f32_32x32x2_f32: M = Cout, N = 16 Cin, K = the output pixels, split into slabs whose partial sums a second launch adds in
//     double in slab order (the scheme of conv3x3_wgrad_kernel, csrc/conv_grad.hip), and the bias gradient in double;
//   * InstanceNorm2d(affine=False) + LeakyReLU forward (y, mean, rstd) and backward, one workgroup per (n, c) plane.
#include "slr_common.hpp"
#include "slr_reduce.hpp"
#include "conv4x4.hpp"

namespace slr {

// ------------------------------------------------------------------ weight gradient
// grid (slabs, ci tiles of 32, co tiles of 32), four waves: wave ky owns the taps (ky, 0..3) of 32 co x 32 ci -- 4 accumulators.  A chunk
// is up to 32 consecutive output pixels of one output row; its G values and the four input rows they touch (S * 31 + 4 columns) are
// staged in LDS as [pixel][channel] (stride 33: conflict-free for both the staging stores and the operand reads).  A k step is a pixel
// pair; a chunk of cw pixels takes ceil(cw / 2) steps (an odd last pixel pairs with a staged zero).  Slab s takes the chunks
// [s T / S, (s + 1) T / S) of the T = N * OH * ceil(OW / 32) in row-major order and writes part[s][co][ci][ky][kx].
// PAD: the convolution's padding (2: the discriminator; 1: the motion encoder, slr_conv4x4s2_weight_grad).  PRO: the convolution reads
// leaky_relu(X, slope) -- applied while staging (leaky_relu(0) = 0: the zero padding is the same before or after it).
template <int S, int PAD = 2, bool PRO = false>
__global__ __launch_bounds__(256) void conv4x4_wgrad_kernel(const float *__restrict__ X, const float *__restrict__ G,
                                                            const float *__restrict__ gate, float *__restrict__ part, int N, int Cin,
                                                            int Cout, int H, int W, int OH, int OW, int chunks, int CX, float slope) {
    constexpr int XW = S * 31 + 4;
    __shared__ float gs[32 * 33];
    __shared__ float xs[4 * XW * 33];
    const int s = blockIdx.x, SS = gridDim.x, ci0 = blockIdx.y * 32, co0 = blockIdx.z * 32;
    const int first = (int)((long long)s * chunks / SS), last = (int)((long long)(s + 1) * chunks / SS);
    const int lane = threadIdx.x & 63, ky = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    const int per_image = OH * CX;
    for (int ch = first; ch < last; ++ch) {
        const int n = ch / per_image, rem = ch - n * per_image, oy = rem / CX, ox0 = (rem - oy * CX) * 32;
        const int cw = OW - ox0 < 32 ? OW - ox0 : 32;
        __syncthreads();                                 // (the previous chunk's reads are done)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int item = threadIdx.x + k * 256, co = item >> 5, pix = item & 31;
            float v = 0.0f;
            if (pix < cw && co0 + co < Cout) {
                const size_t idx = (((size_t)n * Cout + co0 + co) * OH + oy) * OW + ox0 + pix;
                v = G[idx];
                if (gate) v *= gate[idx] > 0.0f ? 1.0f : slope;
            }
            gs[pix * 33 + co] = v;
        }
        for (int item = threadIdx.x; item < 32 * 4 * XW; item += 256) {
            const int ci = item / (4 * XW), rr = item - ci * (4 * XW), ry = rr / XW, rx = rr - ry * XW;
            const int iy = S * oy + ry - PAD, ix = S * ox0 + rx - PAD;
            float v = 0.0f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W && ci0 + ci < Cin) v = X[(((size_t)n * Cin + ci0 + ci) * H + iy) * W + ix];
            if (PRO) v = v > 0.0f ? v : v * slope;
            xs[(ry * XW + rx) * 33 + ci] = v;
        }
        __syncthreads();
        const int npair = cw >> 1;
        for (int j = 0; j < npair; ++j) {
            const int pix = 2 * j + h;
            const float av = gs[pix * 33 + c];
            const float *xb = xs + ((ky * XW + S * pix) * 33 + c);
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) acc[kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[kx * 33], acc[kx], 0, 0, 0);
        }
        if (cw & 1) {
            // the odd last pixel's partner is no term of the sum: its G is a staged zero and its X operands are selected to zero too, or
            // 0 x NaN on the matrix core would put a NaN of a real X element into taps it has no part in
            const int pix = cw - 1 + h;
            const float av = gs[pix * 33 + c];
            const float *xb = xs + ((ky * XW + S * pix) * 33 + c);
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) acc[kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, h == 0 ? xb[kx * 33] : 0.0f, acc[kx], 0, 0, 0);
        }
    }
    // D[row = co][column = ci]: the column on the lane, row mfma32_row(q, lane >> 5) in register q
    const int ci = ci0 + c;
    if (ci < Cin) {
        const size_t total = (size_t)Cout * Cin * 16;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = co0 + mfma32_row(q, h);
            if (co < Cout) {
                float *dst = part + (size_t)s * total + ((size_t)co * Cin + ci) * 16 + ky * 4;
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) dst[kx] = acc[kx][q];
            }
        }
    }
}

// dw[e] = sum_s part[s][e], in double, in slab order.
__global__ __launch_bounds__(256) void conv4x4_wgrad_sum_kernel(const float *__restrict__ part, float *__restrict__ dw, int S,
                                                                long long total) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += (double)part[(size_t)s * total + e];
    dw[e] = (float)v;
}

// db[c] = sum over (n, pixel) of g (gated), in double: one workgroup per channel, a fixed order.
__global__ __launch_bounds__(256) void conv4x4_bias_grad_kernel(const float *__restrict__ g, const float *__restrict__ gate,
                                                                float *__restrict__ db, int N, int C, int OHW, float slope) {
    __shared__ double red[1][4];
    const int c = blockIdx.x;
    double v[1] = {0.0};
    for (int n = 0; n < N; ++n) {
        const size_t base = ((size_t)n * C + c) * OHW;
        for (int i = threadIdx.x; i < OHW; i += 256) {
            float e = g[base + i];
            if (gate) e *= gate[base + i] > 0.0f ? 1.0f : slope;
            v[0] += (double)e;
        }
    }
    block_sum<1, 4>(v, red);
    if (threadIdx.x == 0) db[c] = (float)v[0];
}

static long long dcw_chunks(int N, int H, int W, int stride) { return (long long)N * c4_out(H, stride) * ((c4_out(W, stride) + 31) / 32); }
static int dcw_splits(int N, int Cin, int Cout, int H, int W, int stride, int splits) {
    const long long chunks = dcw_chunks(N, H, W, stride);
    long long S = splits > 0 ? splits : slr_wgrad_auto_splits(chunks, (long long)c4_tiles(Cin) * c4_tiles(Cout), (long long)Cout * Cin * 16 * 4);
    if (S > 65535) S = 65535;
    return (int)(S < chunks ? S : chunks);
}

// the same for the motion encoder's convolution (stride 2, padding 1): OH = (H - 2) / 2 + 1
static int e4_out(int H) { return (H - 2) / 2 + 1; }
static bool e4_sizes_ok(int N, int Cin, int Cout, int H, int W) {
    return H >= 2 && W >= 2 && c4_sizes_ok(N, Cin, Cout, H, W, 2);
}
static long long ecw_chunks(int N, int H, int W) { return (long long)N * e4_out(H) * ((e4_out(W) + 31) / 32); }
static int ecw_splits(int N, int Cin, int Cout, int H, int W, int splits) {
    const long long chunks = ecw_chunks(N, H, W);
    long long S = splits > 0 ? splits : slr_wgrad_auto_splits(chunks, (long long)c4_tiles(Cin) * c4_tiles(Cout), (long long)Cout * Cin * 16 * 4);
    if (S > 65535) S = 65535;
    return (int)(S < chunks ? S : chunks);
}

// ------------------------------------------------------------------ instance norm + LeakyReLU
// nn.InstanceNorm2d(C, affine=False) (biased variance, eps) + nn.LeakyReLU(slope), one workgroup per (n, c) plane: mean from the double sum
// of x, variance from the double sum of (x - mean)^2 with the fp32 differences, then y.  mean and rstd are kept for the backward.
__global__ __launch_bounds__(256) void instnorm_lrelu_fwd_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                                 float *__restrict__ mean, float *__restrict__ rstd, int HW, float eps,
                                                                 float slope) {
    __shared__ double red[1][4];
    __shared__ float bc[2];
    const size_t plane = blockIdx.x;
    const float *xp = x + plane * HW;
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < HW; i += 256) v[0] += (double)xp[i];
    block_sum<1, 4>(v, red);
    if (threadIdx.x == 0) bc[0] = (float)(v[0] / (double)HW);
    __syncthreads();
    const float m = bc[0];
    v[0] = 0.0;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const double d = (double)(xp[i] - m);
        v[0] += d * d;
    }
    block_sum<1, 4>(v, red);
    if (threadIdx.x == 0) {
        bc[1] = 1.0f / sqrtf((float)(v[0] / (double)HW) + eps);
        mean[plane] = m;
        rstd[plane] = bc[1];
    }
    __syncthreads();
    const float rs = bc[1];
    float *yp = y + plane * HW;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float xh = (xp[i] - m) * rs;
        yp[i] = xh > 0.0f ? xh : xh * slope;
    }
}

// xh = (x - mean) rstd, gh = gy (xh > 0 ? 1 : slope), gx = rstd (gh - mean(gh) - xh mean(gh xh)); the two means from double sums.
__global__ __launch_bounds__(256) void instnorm_lrelu_bwd_kernel(const float *__restrict__ x, const float *__restrict__ gy,
                                                                 const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                 float *__restrict__ gx, int HW, float slope) {
    __shared__ double red[2][4];
    __shared__ float bc[2];
    const size_t plane = blockIdx.x;
    const float *xp = x + plane * HW, *gp = gy + plane * HW;
    const float m = mean[plane], rs = rstd[plane];
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float xh = (xp[i] - m) * rs;
        const float gh = gp[i] * (xh > 0.0f ? 1.0f : slope);
        v[0] += (double)gh;
        v[1] += (double)gh * (double)xh;
    }
    block_sum<2, 4>(v, red);
    if (threadIdx.x == 0) {
        bc[0] = (float)(v[0] / (double)HW);
        bc[1] = (float)(v[1] / (double)HW);
    }
    __syncthreads();
    const float m1 = bc[0], m2 = bc[1];
    float *op = gx + plane * HW;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float xh = (xp[i] - m) * rs;
        const float gh = gp[i] * (xh > 0.0f ? 1.0f : slope);
        op[i] = rs * ((gh - m1) - xh * m2);
    }
}

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT size_t slr_conv4x4_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int stride, int splits) {
    if (!c4_sizes_ok(N, Cin, Cout, H, W, stride) || splits < 0) return 0;
    return al256((size_t)dcw_splits(N, Cin, Cout, H, W, stride, splits) * 16 * Cout * Cin * sizeof(float));
}

SLR_EXPORT int slr_conv4x4_weight_grad(const float *x, const float *g, const float *gate, float *dw, float *db, int N, int Cin, int Cout,
                                       int H, int W, int stride, float slope, int splits, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(x && g && dw, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(c4_sizes_ok(N, Cin, Cout, H, W, stride), "sizes");
    SLR_CHECK_ARG(splits >= 0, "splits (0 = chosen by the library)");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)g | (uintptr_t)gate | (uintptr_t)dw | (uintptr_t)db) & 3), "4-byte aligned tensors");
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < slr_conv4x4_grad_ws_bytes(N, Cin, Cout, H, W, stride, splits)) {
        set_error("%s: ws: slr_conv4x4_grad_ws_bytes(N, Cin, Cout, H, W, stride, splits) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int OH = c4_out(H, stride), OW = c4_out(W, stride), CX = (OW + 31) / 32;
    const int S = dcw_splits(N, Cin, Cout, H, W, stride, splits), chunks = (int)dcw_chunks(N, H, W, stride);
    float *part = (float *)ws;
    const dim3 grid(S, c4_tiles(Cin), c4_tiles(Cout));
    if (stride == 1)
        hipLaunchKernelGGL(conv4x4_wgrad_kernel<1>, grid, dim3(256), 0, st, x, g, gate, part, N, Cin, Cout, H, W, OH, OW, chunks, CX, slope);
    else
        hipLaunchKernelGGL(conv4x4_wgrad_kernel<2>, grid, dim3(256), 0, st, x, g, gate, part, N, Cin, Cout, H, W, OH, OW, chunks, CX, slope);
    SLR_CHECK_LAUNCH();
    const long long total = (long long)Cout * Cin * 16;
    hipLaunchKernelGGL(conv4x4_wgrad_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float *)part, dw, S, total);
    SLR_CHECK_LAUNCH();
    if (db) {
        hipLaunchKernelGGL(conv4x4_bias_grad_kernel, dim3(Cout), dim3(256), 0, st, g, gate, db, N, Cout, OH * OW, slope);
        SLR_CHECK_LAUNCH();
    }
    return 0;
}

SLR_EXPORT size_t slr_conv4x4s2_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int splits) {
    if (!e4_sizes_ok(N, Cin, Cout, H, W) || splits < 0) return 0;
    return al256((size_t)ecw_splits(N, Cin, Cout, H, W, splits) * 16 * Cout * Cin * sizeof(float));
}

SLR_EXPORT int slr_conv4x4s2_weight_grad(const float *x, const float *g, float *dw, float *db, int N, int Cin, int Cout, int H, int W,
                                         int leaky, float slope, int splits, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(x && g && dw, "null pointer");
    SLR_CHECK_ARG(e4_sizes_ok(N, Cin, Cout, H, W), "sizes (H, W >= 2)");
    SLR_CHECK_ARG(splits >= 0, "splits (0 = chosen by the library)");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)g | (uintptr_t)dw | (uintptr_t)db) & 3), "4-byte aligned tensors");
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < slr_conv4x4s2_grad_ws_bytes(N, Cin, Cout, H, W, splits)) {
        set_error("%s: ws: slr_conv4x4s2_grad_ws_bytes(N, Cin, Cout, H, W, splits) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int OH = e4_out(H), OW = e4_out(W), CX = (OW + 31) / 32;
    const int S = ecw_splits(N, Cin, Cout, H, W, splits), chunks = (int)ecw_chunks(N, H, W);
    float *part = (float *)ws;
    const float *none = nullptr;
    const dim3 grid(S, c4_tiles(Cin), c4_tiles(Cout));
    if (leaky)
        hipLaunchKernelGGL((conv4x4_wgrad_kernel<2, 1, true>), grid, dim3(256), 0, st, x, g, none, part, N, Cin, Cout, H, W, OH, OW, chunks, CX, slope);
    else
        hipLaunchKernelGGL((conv4x4_wgrad_kernel<2, 1, false>), grid, dim3(256), 0, st, x, g, none, part, N, Cin, Cout, H, W, OH, OW, chunks, CX, slope);
    SLR_CHECK_LAUNCH();
    const long long total = (long long)Cout * Cin * 16;
    hipLaunchKernelGGL(conv4x4_wgrad_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float *)part, dw, S, total);
    SLR_CHECK_LAUNCH();
    if (db) {
        hipLaunchKernelGGL(conv4x4_bias_grad_kernel, dim3(Cout), dim3(256), 0, st, g, none, db, N, Cout, OH * OW, slope);
        SLR_CHECK_LAUNCH();
    }
    return 0;
}

static bool in_sizes_ok(int N, int C, int H, int W) {
    return N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C < (1LL << 31) && (long long)H * W < (1LL << 31) - 256 && (long long)H * W >= 4;
}

SLR_EXPORT int slr_instnorm_lrelu_forward(const float *x, float *y, float *mean, float *rstd, int N, int C, int H, int W, float eps,
                                          float slope, void *stream) {
    SLR_CHECK_ARG(x && y && mean && rstd, "null pointer");
    SLR_CHECK_ARG(in_sizes_ok(N, C, H, W), "sizes (planes of at least 2 x 2)");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)y | (uintptr_t)mean | (uintptr_t)rstd) & 3), "4-byte aligned tensors");
    hipLaunchKernelGGL(instnorm_lrelu_fwd_kernel, dim3((unsigned)(N * C)), dim3(256), 0, (hipStream_t)stream, x, y, mean, rstd, H * W, eps, slope);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_instnorm_lrelu_backward(const float *x, const float *gy, const float *mean, const float *rstd, float *gx, int N, int C,
                                           int H, int W, float slope, void *stream) {
    SLR_CHECK_ARG(x && gy && mean && rstd && gx, "null pointer");
    SLR_CHECK_ARG(in_sizes_ok(N, C, H, W), "sizes (planes of at least 2 x 2)");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)gy | (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)gx) & 3), "4-byte aligned tensors");
    hipLaunchKernelGGL(instnorm_lrelu_bwd_kernel, dim3((unsigned)(N * C)), dim3(256), 0, (hipStream_t)stream, x, gy, mean, rstd, gx, H * W, slope);
    SLR_CHECK_LAUNCH();
    return 0;
}
