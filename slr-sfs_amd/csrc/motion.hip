// motion.hip -- the kernels of the motion U-Nets (models/networks/architectures.py:382-493 Unet4Motion, :602-743
// SPADEUnet4MaskMotion; models/networks/networks.py:422-463 SPADE), which predict the motion field from a still image.
// Every convolution of these networks runs on the fp32 matrix instructions (v_mfma_f32_32x32x2_f32: fp32 operands, products and
// accumulation): the predicted field goes straight into the Euler integration, whose rint() of positions turns a perturbation into
// moved trajectories.  The 3x3 convolutions use slr_conv3x3_forward with SLR_CONV_F32 (csrc/conv.hip); this file adds
//   * the 4x4 / stride 2 / pad 1 encoder convolution as an implicit GEMM (LeakyReLU prologue, bias + per-channel affine epilogue),
//   * instance-norm statistics + SPADE modulation,
//   * the SPADE segmap resized to a level (bilinear, nearest for the mask channel),
//   * the decoder's x2 up-sampling of two sources into one concatenated tensor (optional nearest channel, ReLU before or after).
#include "slr_common.hpp"

namespace slr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------ 4x4 / stride 2 / pad 1 convolution
// GEMM view: out[co][p] = sum_k w[co][k] * im2col[k][p], k = ci*16 + ky*4 + kx, p = flat (n, oy, ox) over the whole batch (small
// deep layers of several samples share one tile).  v_mfma_f32_32x32x2_f32: A = weights (row = output channel), B = input taps (column
// = output pixel); lane l holds A[l&31][k0 + (l>>5)] and B[k0 + (l>>5)][l&31].  One input channel = 16 taps = 8 MFMAs: step s covers
// k = 2s + (l>>5) -> ky = s>>1, kx = 2*(s&1) + (l>>5).
// Weight fragments: wf[((ct*Cin + ci)*8 + s)*64 + lane] = w[ct*32 + (lane&31)][ci][s>>1][2*(s&1) + (lane>>5)] (0 beyond Cout): one
// coalesced 256-byte load per MFMA.
__global__ __launch_bounds__(256) void conv4x4s2_weights_kernel(const float *__restrict__ w, float *__restrict__ wf, int Cout, int Cin,
                                                                long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    long long rest = idx >> 6;
    const int s = (int)(rest & 7);
    rest >>= 3;
    const int ci = (int)(rest % Cin), ct = (int)(rest / Cin);
    const int co = ct * 32 + (lane & 31), ky = s >> 1, kx = 2 * (s & 1) + (lane >> 5);
    wf[idx] = co < Cout ? w[(((size_t)co * Cin + ci) * 4 + ky) * 4 + kx] : 0.0f;
}

// One workgroup = CT output-channel tiles of 32 x one tile of 32 output pixels; its KW waves split the input channels (wave w takes
// ci = w, w + KW, ...) and wave 0 sums their accumulators from LDS in wave order (deterministic).  KW > 1 serves the deep layers,
// whose M*N is a few tiles while K reaches 4096.
template <int CT, bool LEAKY>
__global__ __launch_bounds__(1024) void conv4x4s2_kernel(const float *__restrict__ in, const float *__restrict__ wf,
                                                         const float *__restrict__ bias, const float *__restrict__ post_scale,
                                                         const float *__restrict__ post_shift, float *__restrict__ out,
                                                         int N, int Cin, int Cout, int H, int W, int OH, int OW, float slope) {
    extern __shared__ float red[];                       // [KW-1][CT*16][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, KW = blockDim.x >> 6;
    const int OHW = OH * OW;
    const long long P = (long long)N * OHW;
    const long long p = (long long)blockIdx.x * 32 + (lane & 31);
    const bool pv = p < P;
    const int pp = pv ? (int)p : 0;
    const int n = pp / OHW, r = pp - n * OHW, oy = r / OW, ox = r - oy * OW;
    const int h = lane >> 5;
    int off[8];
    bool ok[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int iy = 2 * oy - 1 + (s >> 1), ix = 2 * ox - 1 + 2 * (s & 1) + h;
        ok[s] = pv & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W);
        off[s] = ok[s] ? iy * W + ix : 0;
    }
    const size_t HW = (size_t)H * W;
    const float *ip = in + (size_t)n * Cin * HW;
    const int ct0 = blockIdx.y * CT;
    f32x16 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    for (int ci = wave; ci < Cin; ci += KW) {
        const float *pl = ip + (size_t)ci * HW;
        float b[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float v = pl[off[s]];
            const float x = ok[s] ? v : 0.0f;
            b[s] = LEAKY ? (x > 0.0f ? x : x * slope) : x;  // leaky_relu(0) = 0: zero padding before or after it is the same
        }
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const float *a = wf + ((size_t)(ct0 + t) * Cin + ci) * 512 + lane;
#pragma unroll
            for (int s = 0; s < 8; ++s) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s * 64], b[s], acc[t], 0, 0, 0);
        }
    }
    if (KW > 1) {
        if (wave > 0) {
            float *dst = red + (size_t)(wave - 1) * CT * 16 * 64 + lane;
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) dst[(t * 16 + q) * 64] = acc[t][q];
        }
        __syncthreads();
        if (wave > 0) return;
        for (int w = 1; w < KW; ++w) {
            const float *src = red + (size_t)(w - 1) * CT * 16 * 64 + lane;
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] += src[(t * 16 + q) * 64];
        }
    }
    if (!pv) return;
    float *op = out + (size_t)n * Cout * OHW + r;
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = (ct0 + t) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;   // C/D map of the 32x32 MFMA
            if (co < Cout) {
                float y = acc[t][q] + (bias ? bias[co] : 0.0f);
                if (post_scale) y = y * post_scale[co] + post_shift[co];
                op[(size_t)co * OHW] = y;
            }
        }
}

static int conv4x4s2_tiles(int Cout) { return (Cout + 31) / 32; }

SLR_EXPORT size_t slr_conv4x4s2_weight_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0) return 0;
    return (size_t)conv4x4s2_tiles(Cout) * Cin * 512 * sizeof(float);
}

SLR_EXPORT int slr_conv4x4s2_f32_weights(const float *w, void *wfrag, int Cout, int Cin, void *stream) {
    SLR_CHECK_ARG(w && wfrag, "null pointer");
    SLR_CHECK_ARG(Cout > 0 && Cin > 0 && Cout < (1 << 16) && Cin < (1 << 16), "sizes");
    const long long total = (long long)conv4x4s2_tiles(Cout) * Cin * 512;
    hipLaunchKernelGGL(conv4x4s2_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (float *)wfrag, Cout, Cin, total);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_conv4x4s2_forward(const float *in, const void *wfrag, const float *bias, const float *post_scale,
                                     const float *post_shift, float *out, int N, int Cin, int Cout, int H, int W, int leaky,
                                     float slope, void *stream) {
    SLR_CHECK_ARG(in && wfrag && out, "null pointer");
    SLR_CHECK_ARG(!post_scale == !post_shift, "post_scale and post_shift go together");
    SLR_CHECK_ARG(N > 0 && N < 65536 && Cin > 0 && Cin < (1 << 16) && Cout > 0 && Cout < (1 << 16) && H >= 2 && W >= 2 &&
                  (long long)H * W < (1LL << 31) && (long long)N * Cin * H * W < (1LL << 40), "sizes (H, W >= 2)");
    const int OH = (H - 2) / 2 + 1, OW = (W - 2) / 2 + 1;
    const int ntile = conv4x4s2_tiles(Cout);
    const long long ptiles = ((long long)N * OH * OW + 31) / 32;
    SLR_CHECK_ARG(ptiles < (1LL << 31), "sizes");
    // CT tiles of 32 output channels per workgroup (the input taps are loaded once for all of them); outputs of a few tiles take one
    // channel tile per workgroup and split K over up to 16 waves instead, so that the deep layers fill the chip.  LDS of the K split:
    // (KW - 1) * CT * 4 KiB <= 60 KiB.
    int CT = ntile % 4 == 0 ? 4 : ntile % 2 == 0 ? 2 : 1;
    if (ptiles * (ntile / CT) < 512) CT = 1;
    const long long wgs = ptiles * (ntile / CT);
    int KW = 1;
    while (KW < 16 / CT && wgs * KW < 2048 && 2 * KW <= Cin) KW *= 2;
    const dim3 grid((unsigned)ptiles, ntile / CT);
    const size_t lds = (size_t)(KW - 1) * CT * 16 * 64 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const float *wf = (const float *)wfrag;
#define C4_LAUNCH(T, L) hipLaunchKernelGGL((conv4x4s2_kernel<T, L>), grid, dim3(64 * KW), lds, st, in, wf, bias, post_scale, post_shift, out, \
                                           N, Cin, Cout, H, W, OH, OW, slope)
    if (CT == 4) { if (leaky) C4_LAUNCH(4, true); else C4_LAUNCH(4, false); }
    else if (CT == 2) { if (leaky) C4_LAUNCH(2, true); else C4_LAUNCH(2, false); }
    else { if (leaky) C4_LAUNCH(1, true); else C4_LAUNCH(1, false); }
#undef C4_LAUNCH
    SLR_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ instance norm + SPADE modulation
// nn.InstanceNorm2d(C) (affine=False, eps, biased variance) and out = norm(x) * (1 + gamma) + beta (networks.py:441-463); gamma / beta
// are the two halves of gb [N, 2C, H, W] (one 3x3 convolution 128 -> 2C).  One workgroup per (n, c) plane: two passes for mean and
// variance (fp32 partial sums, tree reduction), a third for the output.
__device__ __forceinline__ float block_sum1024(float v, float *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                     // (sh is reused by consecutive reductions)
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float t = 0.0f;
    for (int w = 0; w < 16; ++w) t += sh[w];
    return t;
}

__global__ __launch_bounds__(1024) void instnorm_spade_kernel(const float *__restrict__ x, const float *__restrict__ gb,
                                                              float *__restrict__ out, int C, int HW, float eps) {
    __shared__ float sh[16];
    const size_t plane = blockIdx.x;
    const int n = (int)(plane / C), c = (int)(plane % C);
    const float *xp = x + plane * HW;
    const float *g = gb + ((size_t)n * 2 * C + c) * HW;
    const float *b = g + (size_t)C * HW;
    float s = 0.0f;
    for (int i = threadIdx.x; i < HW; i += 1024) s += xp[i];
    const float mean = block_sum1024(s, sh) / (float)HW;
    float q = 0.0f;
    for (int i = threadIdx.x; i < HW; i += 1024) {
        const float d = xp[i] - mean;
        q += d * d;
    }
    const float var = block_sum1024(q, sh) / (float)HW;
    const float rstd = 1.0f / sqrtf(var + eps);
    float *op = out + plane * HW;
    for (int i = threadIdx.x; i < HW; i += 1024) op[i] = ((xp[i] - mean) * rstd) * (1.0f + g[i]) + b[i];
}

SLR_EXPORT int slr_instnorm_spade(const float *x, const float *gamma_beta, float *out, int N, int C, int H, int W, float eps,
                                  void *stream) {
    SLR_CHECK_ARG(x && gamma_beta && out, "null pointer");
    SLR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C < (1LL << 31) && (long long)H * W < (1LL << 31) - 1024, "sizes");
    hipLaunchKernelGGL(instnorm_spade_kernel, dim3((unsigned)(N * C)), dim3(1024), 0, (hipStream_t)stream, x, gamma_beta, out, C, H * W, eps);
    SLR_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ SPADE segmap at a level
// F.interpolate(segmap, size=(H >> k, W >> k)) per channel group (networks.py:446-457): bilinear, align_corners=False with
// scale = in / out = 2^k: src = max((dst + 0.5) * 2^k - 0.5, 0), i0 = (int)src, i1 = min(i0 + 1, in - 1) -- for the mask channel
// `nearest_channel` nearest: src = dst * 2^k.
__global__ __launch_bounds__(256) void resize_segmap_kernel(const float *__restrict__ in, float *__restrict__ out, int C, int H, int W,
                                                            int k, int nearest_channel) {
    const int OH = H >> k, OW = W >> k;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= OH * OW) return;
    const int oy = idx / OW, ox = idx - oy * OW;
    const size_t plane = blockIdx.y;
    const int c = (int)(plane % C);
    const float *ip = in + plane * (size_t)H * W;
    float v;
    if (c == nearest_channel) {
        v = ip[(size_t)(oy << k) * W + (ox << k)];
    } else {
        const float sc = (float)(1 << k);
        const float sy = fmaxf((oy + 0.5f) * sc - 0.5f, 0.0f), sx = fmaxf((ox + 0.5f) * sc - 0.5f, 0.0f);
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
        v = ly0 * (lx0 * ip[(size_t)y0 * W + x0] + lx1 * ip[(size_t)y0 * W + x1]) +
            ly1 * (lx0 * ip[(size_t)y1 * W + x0] + lx1 * ip[(size_t)y1 * W + x1]);
    }
    out[plane * (size_t)OH * OW + idx] = v;
}

SLR_EXPORT int slr_resize_segmap(const float *in, float *out, int N, int C, int H, int W, int k, int nearest_channel, void *stream) {
    SLR_CHECK_ARG(in && out, "null pointer");
    SLR_CHECK_ARG(N > 0 && C > 0 && k >= 0 && k < 16 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && (long long)N * C < 65536,
                  "sizes");
    SLR_CHECK_ARG(H % (1 << k) == 0 && W % (1 << k) == 0, "H and W must be multiples of 2^k");
    const int OHW = (H >> k) * (W >> k);
    hipLaunchKernelGGL(resize_segmap_kernel, dim3((OHW + 255) / 256, N * C), dim3(256), 0, (hipStream_t)stream, in, out, C, H, W, k,
                       nearest_channel);
    SLR_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ x2 up-sampling of two sources into one concatenated tensor
// out[n] = cat(up(a[n]), up(b[n])) [Ca + Cb, 2H, 2W].  up = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False), the
// expression and order of slr_upsample_bilinear2x (csrc/resample.hip), except channel `nearest_channel` OF EACH SOURCE, which is
// nn.Upsample(scale_factor=2, mode='nearest') (architectures.py:712-740).  relu = 1: ReLU of the inputs (up(relu(.)),
// architectures.py:463-489, and e8 at :710); relu = 2: ReLU of the result (relu(cat(up(.), up(.))), :715-741).
__global__ __launch_bounds__(256) void upsample2x_concat_kernel(const float *__restrict__ a, int Ca, const float *__restrict__ b, int Cb,
                                                                float *__restrict__ out, int H, int W, int nearest_channel, int relu) {
    const int OH = 2 * H, OW = 2 * W;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= OH * OW) return;
    const int oy = idx / OW, ox = idx - oy * OW;
    const int C = Ca + Cb;
    const int n = blockIdx.y / C, c = blockIdx.y % C;
    const bool from_a = c < Ca;
    const int cs = from_a ? c : c - Ca;
    const float *ip = from_a ? a + ((size_t)n * Ca + cs) * H * W : b + ((size_t)n * Cb + cs) * H * W;
    float v;
    if (cs == nearest_channel) {
        v = ip[(size_t)(oy >> 1) * W + (ox >> 1)];
        if (relu) v = fmaxf(v, 0.0f);
    } else {
        const float sy = fmaxf((oy + 0.5f) * 0.5f - 0.5f, 0.0f), sx = fmaxf((ox + 0.5f) * 0.5f - 0.5f, 0.0f);
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
        float v00 = ip[(size_t)y0 * W + x0], v01 = ip[(size_t)y0 * W + x1], v10 = ip[(size_t)y1 * W + x0], v11 = ip[(size_t)y1 * W + x1];
        if (relu == 1) {
            v00 = fmaxf(v00, 0.0f); v01 = fmaxf(v01, 0.0f); v10 = fmaxf(v10, 0.0f); v11 = fmaxf(v11, 0.0f);
        }
        v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
        if (relu == 2) v = fmaxf(v, 0.0f);
    }
    out[(size_t)blockIdx.y * OH * OW + idx] = v;
}

SLR_EXPORT int slr_upsample2x_concat(const float *a, int Ca, const float *b, int Cb, float *out, int N, int H, int W,
                                     int nearest_channel, int relu, void *stream) {
    SLR_CHECK_ARG(a && out && (Cb == 0 || b), "null pointer");
    SLR_CHECK_ARG(relu >= 0 && relu <= 2, "relu: 0 none, 1 before, 2 after the up-sampling");
    SLR_CHECK_ARG(N > 0 && Ca > 0 && Cb >= 0 && H > 0 && W > 0 && (long long)N * (Ca + Cb) < 65536 && 4LL * H * W < (1LL << 31), "sizes");
    hipLaunchKernelGGL(upsample2x_concat_kernel, dim3((4 * H * W + 255) / 256, N * (Ca + Cb)), dim3(256), 0, (hipStream_t)stream, a, Ca,
                       b, Cb, out, H, W, nearest_channel, relu);
    SLR_CHECK_LAUNCH();
    return 0;
}

}  // namespace slr
