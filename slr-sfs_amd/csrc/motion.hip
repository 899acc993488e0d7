// motion.hip -- the kernels of the motion U-Nets (models/networks/architectures.py:382-493 Unet4Motion, :602-743
// SPADEUnet4MaskMotion; models/networks/networks.py:422-463 SPADE), which predict the motion field from a still image.
// Every convolution of these networks runs on the fp32 matrix instructions (v_mfma_f32_32x32x2_f32: fp32 operands, products and
// accumulation): the predicted field goes straight into the Euler integration, whose rint() of positions turns a perturbation into
// moved trajectories.  The 3x3 convolutions use slr_conv3x3_forward with SLR_CONV_F32 (csrc/conv.hip); the 4x4 / stride 2 / pad 1
// encoder convolution is slr_conv4x4s2_forward (csrc/conv4x4.hip); this file adds
//   * instance-norm statistics + SPADE modulation,
//   * the SPADE segmap resized to a level (bilinear, nearest for the mask channel),
//   * the decoder's x2 up-sampling of two sources into one concatenated tensor (optional nearest channel, ReLU before or after).
#include "slr_common.hpp"

namespace slr {

// ------------------------------------------------------------------ instance norm + SPADE modulation
// nn.InstanceNorm2d(C) (affine=False, eps, biased variance) and out = norm(x) * (1 + gamma) + beta (networks.py:441-463); gamma / beta
// are the two halves of gb [N, 2C, H, W] (one 3x3 convolution 128 -> 2C).  One workgroup per (n, c) plane: two passes for mean and
// variance (fp32 partial sums, tree reduction), a third for the output.  KEEP: the training forward (slr_instnorm_spade_train_forward) --
// the same code, so the same bits, which also writes the plane's mean and rstd for the backward (csrc/motion_grad.hip).
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

template <bool KEEP>
__global__ __launch_bounds__(1024) void instnorm_spade_kernel(const float *__restrict__ x, const float *__restrict__ gb,
                                                              float *__restrict__ out, float *__restrict__ mean_out,
                                                              float *__restrict__ rstd_out, int C, int HW, float eps) {
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
    if (KEEP && threadIdx.x == 0) {
        mean_out[plane] = mean;
        rstd_out[plane] = rstd;
    }
    float *op = out + plane * HW;
    for (int i = threadIdx.x; i < HW; i += 1024) op[i] = ((xp[i] - mean) * rstd) * (1.0f + g[i]) + b[i];
}

SLR_EXPORT int slr_instnorm_spade(const float *x, const float *gamma_beta, float *out, int N, int C, int H, int W, float eps,
                                  void *stream) {
    SLR_CHECK_ARG(x && gamma_beta && out, "null pointer");
    SLR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C < (1LL << 31) && (long long)H * W < (1LL << 31) - 1024, "sizes");
    hipLaunchKernelGGL(instnorm_spade_kernel<false>, dim3((unsigned)(N * C)), dim3(1024), 0, (hipStream_t)stream, x, gamma_beta, out,
                       (float *)nullptr, (float *)nullptr, C, H * W, eps);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_instnorm_spade_train_forward(const float *x, const float *gamma_beta, float *out, float *mean, float *rstd, int N, int C,
                                                int H, int W, float eps, void *stream) {
    SLR_CHECK_ARG(x && gamma_beta && out && mean && rstd, "null pointer");
    SLR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C < (1LL << 31) && (long long)H * W < (1LL << 31) - 1024 &&
                  (long long)H * W >= 4, "sizes (planes of at least 2 x 2)");
    hipLaunchKernelGGL(instnorm_spade_kernel<true>, dim3((unsigned)(N * C)), dim3(1024), 0, (hipStream_t)stream, x, gamma_beta, out, mean,
                       rstd, C, H * W, eps);
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
    SLR_CHECK_ARG(N > 0 && C > 0 && k >= 0 && k < 16 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) - 256 && (long long)N * C < 65536,
                  "sizes");      // (k = 0: a work-item's pixel, rounded up to the workgroup, stays an int)
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
    SLR_CHECK_ARG(N > 0 && Ca > 0 && Cb >= 0 && H > 0 && W > 0 && (long long)N * (Ca + Cb) < 65536 && 4LL * H * W < (1LL << 31) - 256,
                  "sizes");                                       // (an output pixel's index, rounded up to the workgroup, stays an int)
    hipLaunchKernelGGL(upsample2x_concat_kernel, dim3((4 * H * W + 255) / 256, N * (Ca + Cb)), dim3(256), 0, (hipStream_t)stream, a, Ca,
                       b, Cb, out, H, W, nearest_channel, relu);
    SLR_CHECK_LAUNCH();
    return 0;
}

}  // namespace slr
