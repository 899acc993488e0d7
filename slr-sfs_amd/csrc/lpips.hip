// lpips.hip -- LPIPS v0.1, net "alex" (the LPIPS column of the reference's tables: evaluation/animation/eval_CLAW.py:24,37; the trunk and
// the scaling constants: models/networks/pretrained_networks.py:45-46,154-196), ABI 26:
//   * the input scaling (x - shift) / scale, optionally of 2x - 1, written NCHW for the first convolution,
//   * the K x K convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (fp32 operands, products and accumulation: the arithmetic of
//     the fp32 rung), one kernel body for Conv2d(3, 64, 11, stride 4, padding 2) and Conv2d(64, 192, 5, padding 2), bias added, the
//     output raw (pre-ReLU) and channel-blocked,
//   * ReLU + 3x3 / stride 2 max pooling of channel-blocked activations,
//   * the LPIPS distance of two channel-blocked feature maps: ReLU, unit normalisation over the channels, the squared difference
//     weighted per channel, the spatial mean -- one pass.
// The three 3x3 convolutions of the trunk run on slr_conv3x3_forward with SLR_CONV_F32 (csrc/conv.hip).
// Nothing synchronises; no atomics; every sum has a fixed order that depends on the image alone: the same bits from run to run and
// whatever batch the image sits in.
#include "slr_common.hpp"
#include "slr_reduce.hpp"

namespace slr {

// ------------------------------------------------------------------ input scaling
// ScalingLayer of LPIPS = the shift / scale of pretrained_networks.py:45-46: float32 values.
__constant__ float LP_SHIFT[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float LP_SCALE[3] = {0.458f, 0.448f, 0.450f};

template <bool U8>
__global__ __launch_bounds__(256) void lpips_prep_kernel(const void *__restrict__ img, float *__restrict__ out, long long P, int HW,
                                                         int normalize) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const long long n = i / HW, r = i - n * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = U8 ? (float)((const unsigned char *)img)[i * 3 + c] / 255.0f : ((const float *)img)[(n * 3 + c) * HW + r];
        if (normalize) x = x * 2.0f - 1.0f;
        out[(n * 3 + c) * HW + r] = (x - LP_SHIFT[c]) / LP_SCALE[c];
    }
}

// ------------------------------------------------------------------ K x K convolution, forward
// GEMM view (as csrc/conv4x4.hip): out[m][p] = sum_k a[m][k] b[k][p]; m = an output channel, k = (input channel ci, tap t = ky K + kx),
// p = an output pixel, flat over the whole batch.  Lane l of a v_mfma_f32_32x32x2_f32 holds A[l & 31][k0 + (l >> 5)] and
// B[k0 + (l >> 5)][l & 31]: step s of a channel carries the taps t = 2 s + (l >> 5), NS = ceil(K K / 2) steps, the tap K K of an odd
// K K is zero on both sides.
// Weight fragments (one coalesced 256-byte load per MFMA), zero beyond the last channel and the last tap:
//   wf[((ct Cin + ci) NS + s) 64 + l] = w[32 ct + (l & 31)][ci][t / K][t % K],  t = 2 s + (l >> 5)
constexpr int kxk_steps(int K) { return (K * K + 1) / 2; }
static int kxk_tiles(int Cout) { return (Cout + 31) / 32; }

__global__ __launch_bounds__(256) void convkxk_weights_kernel(const float *__restrict__ w, float *__restrict__ wf, int Cout, int Cin,
                                                              int K, int NS, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    long long rest = idx >> 6;
    const int s = (int)(rest % NS);
    rest /= NS;
    const int ci = (int)(rest % Cin), co = (int)(rest / Cin) * 32 + (lane & 31);
    const int t = 2 * s + (lane >> 5);
    wf[idx] = (co < Cout && t < K * K) ? w[((size_t)co * Cin + ci) * K * K + t] : 0.0f;
}

// One workgroup = one tile of 32 output pixels x NW tiles of 32 output channels, one wave per channel tile.  The 32 pixels are flat, so a
// tile is made of up to 32 SEGMENTS, the runs of its pixels that lie in one output row of one image.  The input a segment of n pixels
// reads is a K x ((n - 1) S + K) patch per channel (its halo included); the patches of a tile's segments lie side by side in LDS, TW
// columns in all (TW <= the host's bound TWS, the row stride), CC channels at a time:
//   patch[(c K + ky) TWS + j],  column seg_base[g] + d of segment g = the input column d of its first pixel's window,  zero outside the image (the padding).
// A pixel's tap (ky, kx) is then patch[(c K + ky) TWS + pix + kx] with pix = seg_base[g] + (ox - ox_first[g]) S: every wave reads the same
// staged values, and a value of the input is fetched once per tile, not once per tap.  Per column the tables col_n / col_iy0 / col_ix
// say which image, first input row and input column it holds.
// `in` is NCHW (B8IN = false) or channel-blocked [N,Cin/8,IH,IW,8] (B8IN = true, Cin % 8 == 0, CC % 8 == 0); `out` is channel-blocked
// [N,Cout/8,OH,OW,8], raw: conv + bias.
template <int K, int S, int PAD, bool B8IN>
__global__ __launch_bounds__(512) void convkxk_kernel(const float *__restrict__ in, const float *__restrict__ wf,
                                                      const float *__restrict__ bias, float *__restrict__ out, int N, int Cin, int Cout,
                                                      int IH, int IW, int OH, int OW, int CC, int TWS) {
    constexpr int NS = kxk_steps(K);
    static_assert(K >= 2 && K >= S, "the tap walk and the bound on TW need K >= 2 and K >= S");
    extern __shared__ float lds[];
    int *col_n = (int *)lds, *col_iy0 = col_n + TWS, *col_ix = col_iy0 + TWS;
    int *seg_base = col_ix + TWS;                        // [33]
    float *patch = (float *)(seg_base + 36);              // [CC K + 1][TWS]: the last row is only ever read for the zero tap
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6, nthreads = blockDim.x;
    const int OHW = OH * OW;
    const long long P = (long long)N * OHW;
    const long long p0 = (long long)blockIdx.x * 32, pend = p0 + 32 < P ? p0 + 32 : P;
    const long long R0 = p0 / OW;                         // the first (image, output row) of the tile
    const int nseg = (int)((pend - 1) / OW - R0) + 1;
    // segment g: pixels max(p0, (R0 + g) OW) .. min(pend, (R0 + g + 1) OW) - 1
    if (threadIdx.x == 0) {
        int base = 0;
        for (int g = 0; g < nseg; ++g) {
            const long long first = (R0 + g) * OW > p0 ? (R0 + g) * OW : p0;
            const long long last = (R0 + g + 1) * OW < pend ? (R0 + g + 1) * OW : pend;
            seg_base[g] = base;
            base += ((int)(last - first) - 1) * S + K;
        }
        seg_base[nseg] = base;
    }
    __syncthreads();
    const int TW = seg_base[nseg];
    for (int j = threadIdx.x; j < TW; j += nthreads) {
        int g = 0;
        while (g + 1 < nseg && j >= seg_base[g + 1]) ++g;
        const long long R = R0 + g;
        const long long first = R * OW > p0 ? R * OW : p0;
        const int n = (int)(R / OH), oy = (int)(R - (long long)n * OH), oxf = (int)(first - R * OW);
        col_n[j] = n;
        col_iy0[j] = oy * S - PAD;
        col_ix[j] = oxf * S - PAD + (j - seg_base[g]);
    }
    // this lane's pixel
    const long long p = p0 + (lane & 31);
    const bool pv = p < P;
    const long long pp = pv ? p : p0;
    const long long Rp = pp / OW;
    const int g = (int)(Rp - R0);
    const long long firstp = Rp * OW > p0 ? Rp * OW : p0;
    const int pix = seg_base[g] + (int)(pp - firstp) * S;
    const int h = lane >> 5;
    const int ct = blockIdx.y * NW + wave;                // this wave's tile of output channels
    const size_t IHW = (size_t)IH * IW;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    for (int c0 = 0; c0 < Cin; c0 += CC) {
        const int cc = Cin - c0 < CC ? Cin - c0 : CC;
        __syncthreads();                                  // the column tables are written / the previous chunk's patch has been read
        if (B8IN) {
            // 8 channels of a (block, ky, column) in two 16-byte loads
            const int items = (cc >> 3) * K * TW;
            for (int it = threadIdx.x; it < items; it += nthreads) {
                const int j = it % TW, row = it / TW, cb = row / K, ky = row - cb * K;
                const int iy = col_iy0[j] + ky, ix = col_ix[j];
                float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
                if ((iy >= 0) & (iy < IH) & (ix >= 0) & (ix < IW)) {
                    const float4 *src = (const float4 *)in + (((size_t)col_n[j] * (Cin >> 3) + (c0 >> 3) + cb) * IHW + (size_t)iy * IW + ix) * 2;
                    lo = src[0];
                    hi = src[1];
                }
                float *dst = patch + (size_t)((cb * 8) * K + ky) * TWS + j;
                dst[0] = lo.x; dst[(size_t)K * TWS] = lo.y; dst[(size_t)2 * K * TWS] = lo.z; dst[(size_t)3 * K * TWS] = lo.w;
                dst[(size_t)4 * K * TWS] = hi.x; dst[(size_t)5 * K * TWS] = hi.y; dst[(size_t)6 * K * TWS] = hi.z; dst[(size_t)7 * K * TWS] = hi.w;
            }
        } else {
            for (int row = wave; row < cc * K; row += NW) {
                const int c = row / K, ky = row - c * K;
                for (int j = lane; j < TW; j += 64) {
                    const int iy = col_iy0[j] + ky, ix = col_ix[j];
                    float v = 0.0f;
                    if ((iy >= 0) & (iy < IH) & (ix >= 0) & (ix < IW)) v = in[((size_t)col_n[j] * Cin + c0 + c) * IHW + (size_t)iy * IW + ix];
                    patch[(size_t)row * TWS + j] = v;
                }
            }
        }
        __syncthreads();
        if (ct * 32 < Cout) {
            const float *af = wf + ((size_t)ct * Cin + c0) * (NS * 64) + lane;
            for (int c = 0; c < cc; ++c) {
                int kx = h, off = c * K * TWS + pix + h;   // tap t = 2 s + h walks the K x K window row by row
#pragma unroll 8
                for (int s = 0; s < NS; ++s) {
                    float b = patch[off];
                    if (2 * s + h >= K * K) b = 0.0f;      // (the tap beyond the window: whatever lies there, a NaN included, is not used)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[((size_t)c * NS + s) * 64], b, acc, 0, 0, 0);
                    kx += 2;
                    off += 2;
                    if (kx >= K) {
                        kx -= K;
                        off += TWS - K;
                    }
                }
            }
        }
    }
    if (!pv || ct * 32 >= Cout) return;
    const int n = (int)(p / OHW), r = (int)(p - (long long)n * OHW);
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {                      // registers 4 qb .. 4 qb + 3: channels 32 ct + 8 qb + 4 h + (0 .. 3)
        const int cm = ct * 32 + qb * 8 + 4 * h;
        if (cm < Cout) {                                  // (Cout % 8 == 0: a block of 8 is whole or absent)
            float4 y;
            y.x = acc[4 * qb] + bias[cm];
            y.y = acc[4 * qb + 1] + bias[cm + 1];
            y.z = acc[4 * qb + 2] + bias[cm + 2];
            y.w = acc[4 * qb + 3] + bias[cm + 3];
            *(float4 *)(out + (((size_t)n * (Cout >> 3) + (cm >> 3)) * OHW + r) * 8 + 4 * h) = y;
        }
    }
}

// The launch rule.  NW = the largest divisor of the channel tiles that is <= 8 waves; CC = 16 channels per stage (all of them below
// 16; fewer while the stage would not fit 64 KiB of LDS, whole blocks of 8 for a channel-blocked input); TWS = the bound on a tile's columns: a tile has at most G = min(32, 30 / OW + 2) segments, and sum_g ((n_g - 1) S + K) with
// sum n_g = 32 is (32 - G) S + G K at most (K >= S).
struct KxkPlan { int NW, CC, TWS; size_t lds; };
static KxkPlan kxk_plan(int Cin, int Cout, int OW, int K, int S, int in_b8) {
    KxkPlan pl;
    const int ntile = kxk_tiles(Cout);
    pl.NW = 1;
    for (int d = 2; d <= 8; ++d)
        if (ntile % d == 0) pl.NW = d;
    pl.CC = Cin < 16 ? Cin : 16;
    const int G = 30 / OW + 2 < 32 ? 30 / OW + 2 : 32;
    pl.TWS = (32 - G) * S + G * K;
    const int step = in_b8 ? 8 : 1;
    for (;;) {
        pl.lds = ((size_t)3 * pl.TWS + 36 + (size_t)(pl.CC * K + 1) * pl.TWS) * sizeof(float);
        if (pl.lds <= 64 * 1024 || pl.CC <= step) break;
        pl.CC -= step;
    }
    return pl;
}

template <int K, int S, int PAD>
static void kxk_launch(const float *in, const float *wf, const float *bias, float *out, int N, int Cin, int Cout, int IH, int IW, int OH,
                       int OW, int in_b8, hipStream_t st) {
    const KxkPlan pl = kxk_plan(Cin, Cout, OW, K, S, in_b8);
    const long long ptiles = ((long long)N * OH * OW + 31) / 32;
    const dim3 grid((unsigned)ptiles, kxk_tiles(Cout) / pl.NW);
    if (in_b8)
        hipLaunchKernelGGL((convkxk_kernel<K, S, PAD, true>), grid, dim3(64 * pl.NW), pl.lds, st, in, wf, bias, out, N, Cin, Cout, IH, IW,
                           OH, OW, pl.CC, pl.TWS);
    else
        hipLaunchKernelGGL((convkxk_kernel<K, S, PAD, false>), grid, dim3(64 * pl.NW), pl.lds, st, in, wf, bias, out, N, Cin, Cout, IH, IW,
                           OH, OW, pl.CC, pl.TWS);
}

// ------------------------------------------------------------------ ReLU + MaxPool2d(3, 2) on channel-blocked activations
// nn.ReLU then nn.MaxPool2d(kernel_size=3, stride=2) of torchvision's alexnet.features: floor mode, no padding; max of relu = relu of
// max.  A NaN in a window makes the window's output NaN, as torch's does (max_nan), like slr_relu_maxpool2x2_b8.
__global__ __launch_bounds__(256) void relu_maxpool3s2_b8_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, long long total,
                                                                 int H, int W, int OH, int OW) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long plane = i / ((long long)OH * OW);
    const int r = (int)(i - plane * OH * OW), oy = r / OW, ox = r - oy * OW;
    const float4 *src = in + (plane * H * W + (long long)(2 * oy) * W + 2 * ox) * 2;
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 a = src[((size_t)dy * W + dx) * 2], b = src[((size_t)dy * W + dx) * 2 + 1];
            lo.x = max_nan(lo.x, a.x); lo.y = max_nan(lo.y, a.y); lo.z = max_nan(lo.z, a.z); lo.w = max_nan(lo.w, a.w);
            hi.x = max_nan(hi.x, b.x); hi.y = max_nan(hi.y, b.y); hi.z = max_nan(hi.z, b.z); hi.w = max_nan(hi.w, b.w);
        }
    out[i * 2] = lo;
    out[i * 2 + 1] = hi;
}

// ------------------------------------------------------------------ LPIPS distance of one layer
// lpips: normalize_tensor(f) = f / (sqrt(sum_c f_c^2) + 1e-10), d = mean_hw sum_c w[c] (n(f0)_c - n(f1)_c)^2 on the ReLU'd features.
// A thread owns a pixel: one walk over the channels for the two norms, a second for the weighted squared difference of the quotients --
// the difference is formed as written, so equal features give exactly 0, and two all-zero vectors give 0 / 1e-10 - 0 / 1e-10 = 0.
// Per pixel the channel sum is fp32 in channel order; the pixels are added in double: wave butterfly, waves in order, workgroups in order.
constexpr int LD_THREADS = 256;
constexpr float LD_EPS = 1e-10f;

__device__ __forceinline__ float ld_sq(float4 a) {
    const float x = fmaxf(a.x, 0.0f), y = fmaxf(a.y, 0.0f), z = fmaxf(a.z, 0.0f), w = fmaxf(a.w, 0.0f);
    return ((x * x + y * y) + z * z) + w * w;
}

__device__ __forceinline__ float ld_term(float a, float b, float d0, float d1, float w) {
    const float d = fmaxf(a, 0.0f) / d0 - fmaxf(b, 0.0f) / d1;
    return w * (d * d);
}

__global__ __launch_bounds__(LD_THREADS) void lpips_distance_kernel(const float4 *__restrict__ f0, const float4 *__restrict__ f1,
                                                                    const float4 *__restrict__ w, double *__restrict__ part, int CB,
                                                                    int HW, int blocks) {
    __shared__ double red[1][LD_THREADS / 64];
    const int n = blockIdx.y, p = blockIdx.x * LD_THREADS + threadIdx.x;
    double v[1] = {0.0};
    if (p < HW) {
        const size_t base = (size_t)n * CB * HW;
        float s0 = 0.0f, s1 = 0.0f;
        for (int cb = 0; cb < CB; ++cb) {
            const size_t o = (base + (size_t)cb * HW + p) * 2;
            s0 += ld_sq(f0[o]); s0 += ld_sq(f0[o + 1]);
            s1 += ld_sq(f1[o]); s1 += ld_sq(f1[o + 1]);
        }
        const float d0 = sqrtf(s0) + LD_EPS, d1 = sqrtf(s1) + LD_EPS;
        float acc = 0.0f;
        for (int cb = 0; cb < CB; ++cb) {
            const size_t o = (base + (size_t)cb * HW + p) * 2;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float4 a = f0[o + k], b = f1[o + k], ww = w[cb * 2 + k];
                acc += ld_term(a.x, b.x, d0, d1, ww.x);
                acc += ld_term(a.y, b.y, d0, d1, ww.y);
                acc += ld_term(a.z, b.z, d0, d1, ww.z);
                acc += ld_term(a.w, b.w, d0, d1, ww.w);
            }
        }
        v[0] = (double)acc;
    }
    block_sum<1, LD_THREADS / 64>(v, red);
    if (threadIdx.x == 0) part[(size_t)n * blocks + blockIdx.x] = v[0];
}

__global__ __launch_bounds__(256) void lpips_distance_finish_kernel(const double *__restrict__ part, float *__restrict__ out, int blocks,
                                                                    double hw) {
    __shared__ double red[1][4];
    const int n = blockIdx.x;
    double v[1] = {0.0};
    for (int t = threadIdx.x; t < blocks; t += 256) v[0] += part[(size_t)n * blocks + t];
    block_sum<1, 4>(v, red);
    if (threadIdx.x == 0) out[n] = (float)(v[0] / hw);
}

static int ld_blocks(int H, int W) { return (int)(((long long)H * W + LD_THREADS - 1) / LD_THREADS); }

static bool kxk_shape_ok(int K, int stride, int pad) { return (K == 11 && stride == 4 && pad == 2) || (K == 5 && stride == 1 && pad == 2); }

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT int slr_lpips_prep(const void *img, int u8, int normalize, float *out, int N, int H, int W, void *stream) {
    SLR_CHECK_ARG(img && out, "null pointer");
    SLR_CHECK_ARG(N > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && (long long)N * H * W < (1LL << 40), "sizes");
    const long long P = (long long)N * H * W;
    const dim3 grid((unsigned)((P + 255) / 256));
    if (u8) hipLaunchKernelGGL(lpips_prep_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, img, out, P, H * W, normalize);
    else hipLaunchKernelGGL(lpips_prep_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, img, out, P, H * W, normalize);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_convkxk_weight_bytes(int Cout, int Cin, int K) {
    if (Cout <= 0 || Cin <= 0 || Cout >= (1 << 16) || Cin >= (1 << 16) || (K != 11 && K != 5)) return 0;
    return (size_t)kxk_tiles(Cout) * Cin * kxk_steps(K) * 64 * sizeof(float);
}

SLR_EXPORT int slr_convkxk_f32_weights(const float *w, void *wfrag, int Cout, int Cin, int K, void *stream) {
    SLR_CHECK_ARG(w && wfrag, "null pointer");
    SLR_CHECK_ARG(K == 11 || K == 5, "K (11 or 5)");
    SLR_CHECK_ARG(Cout > 0 && Cin > 0 && Cout < (1 << 16) && Cin < (1 << 16), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)w | (uintptr_t)wfrag) & 3), "4-byte aligned tensors");
    const long long total = (long long)(slr_convkxk_weight_bytes(Cout, Cin, K) / sizeof(float));
    hipLaunchKernelGGL(convkxk_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (float *)wfrag,
                       Cout, Cin, K, kxk_steps(K), total);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_convkxk_forward(const float *in, const void *wfrag, const float *bias, float *out, int N, int Cin, int Cout, int H,
                                   int W, int K, int stride, int pad, int in_b8, void *stream) {
    SLR_CHECK_ARG(in && wfrag && bias && out, "null pointer");
    SLR_CHECK_ARG(kxk_shape_ok(K, stride, pad), "(K, stride, padding): (11, 4, 2) or (5, 1, 2)");
    SLR_CHECK_ARG(N > 0 && N < 65536 && Cin > 0 && Cin < (1 << 16) && Cout > 0 && Cout < (1 << 16) && Cout % 8 == 0 && H >= 1 && W >= 1 &&
                  H < (1 << 20) && W < (1 << 20) && H + 2 * pad >= K && W + 2 * pad >= K && (long long)H * W < (1LL << 31) &&
                  (long long)N * H * W < (1LL << 31) && (long long)N * Cin * H * W < (1LL << 40), "sizes (Cout % 8 == 0, H + 2 P >= K, W + 2 P >= K)");
    SLR_CHECK_ARG(!in_b8 || Cin % 8 == 0, "a channel-blocked input needs Cin % 8 == 0");
    SLR_CHECK_ARG(!(((uintptr_t)in | (uintptr_t)wfrag | (uintptr_t)bias) & 3) && !((uintptr_t)out & 15) && !(in_b8 && ((uintptr_t)in & 15)),
                  "4-byte aligned tensors, 16-byte aligned channel-blocked ones");
    const int OH = (H + 2 * pad - K) / stride + 1, OW = (W + 2 * pad - K) / stride + 1;
    SLR_CHECK_ARG(kxk_plan(Cin, Cout, OW, K, stride, in_b8).lds <= 64 * 1024, "sizes (LDS)");
    hipStream_t st = (hipStream_t)stream;
    if (K == 11) kxk_launch<11, 4, 2>(in, (const float *)wfrag, bias, out, N, Cin, Cout, H, W, OH, OW, in_b8, st);
    else kxk_launch<5, 1, 2>(in, (const float *)wfrag, bias, out, N, Cin, Cout, H, W, OH, OW, in_b8, st);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_relu_maxpool3x3s2_b8(const float *in, float *out, int N, int C, int H, int W, void *stream) {
    SLR_CHECK_ARG(in && out, "null pointer");
    SLR_CHECK_ARG(!((uintptr_t)in & 15) && !((uintptr_t)out & 15), "16-byte aligned tensors");
    SLR_CHECK_ARG(N > 0 && C > 0 && C % 8 == 0 && H >= 3 && W >= 3 && (long long)N * C * H * W < (1LL << 40),
                  "sizes (C % 8 == 0, H, W >= 3)");
    const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    const long long total = (long long)N * (C / 8) * OH * OW;
    hipLaunchKernelGGL(relu_maxpool3s2_b8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)in, (float4 *)out, total, H, W, OH, OW);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_lpips_distance_ws_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)N * ld_blocks(H, W) * sizeof(double);
}

SLR_EXPORT int slr_lpips_distance(const float *f0, const float *f1, const float *w, float *out, int N, int C, int H, int W, void *ws,
                                  size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(f0 && f1 && w && out && ws, "null pointer");
    SLR_CHECK_ARG(!(((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)w) & 15), "16-byte aligned feature maps and weights");
    SLR_CHECK_ARG(N > 0 && N < 65536 && C > 0 && C % 8 == 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) - LD_THREADS &&
                  (long long)N * C * H * W < (1LL << 40), "sizes (C % 8 == 0)");
    SLR_CHECK_ARG(ws_bytes >= slr_lpips_distance_ws_bytes(N, H, W) && !((uintptr_t)ws & 7), "ws: slr_lpips_distance_ws_bytes(N, H, W)");
    const int blocks = ld_blocks(H, W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lpips_distance_kernel, dim3(blocks, N), dim3(LD_THREADS), 0, st, (const float4 *)f0, (const float4 *)f1,
                       (const float4 *)w, (double *)ws, C / 8, H * W, blocks);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(lpips_distance_finish_kernel, dim3(N), dim3(256), 0, st, (const double *)ws, out, blocks, (double)H * W);
    SLR_CHECK_LAUNCH();
    return 0;
}
