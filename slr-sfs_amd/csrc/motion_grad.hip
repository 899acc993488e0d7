// motion_grad.hip -- what the SPADE motion U-Net (models/networks/architectures.py:602-743 SPADEUnet4MaskMotion) needs to learn beyond its
// convolutions (ABI 23): the backward of the kernels of csrc/motion.hip and the motion losses of models/losses/synthesis.py:11-58, 142-160.
//   * SPADE instance norm: the gradient to x and to gamma | beta (the forward that keeps mean and rstd is instnorm_spade_kernel<true> of
//     csrc/motion.hip, the inference kernel's own code);
//   * the x2 up-sampling + concatenation (+ ReLU before or after): the gradient to both sources as a gather;
//   * EndPointError, MotionL1 and the PSNR's squared error in one pass, and their gradient to the prediction.
// The 4x4 / stride 2 / padding 1 encoder convolution's gradients are modes of conv4x4_kernel (csrc/conv4x4.hip) and of
// conv4x4_wgrad_kernel (csrc/disc.hip).  Everything is NCHW fp32; nothing synchronises; no atomics -- every long sum runs in a fixed order
// in double (slr_reduce.hpp), so the same inputs give the same bits.
#include "slr_common.hpp"
#include "slr_reduce.hpp"

namespace slr {

// ------------------------------------------------------------------ SPADE instance norm, backward
// out = xh (1 + gamma) + beta, xh = (x - mean) rstd.  From g = d out:  d beta = g,  d gamma = g xh,  gh = g (1 + gamma),
// gx = rstd (gh - mean(gh) - xh mean(gh xh)); the two means from double sums.  d gamma | d beta go to dgb [N, 2C, H, W], the layout of the
// forward's gamma_beta.  One workgroup per (n, c) plane.
__global__ __launch_bounds__(256) void instnorm_spade_bwd_kernel(const float *__restrict__ x, const float *__restrict__ gb,
                                                                 const float *__restrict__ g, const float *__restrict__ mean,
                                                                 const float *__restrict__ rstd, float *__restrict__ gx,
                                                                 float *__restrict__ dgb, int C, int HW) {
    __shared__ double red[2][4];
    __shared__ float bc[2];
    const size_t plane = blockIdx.x;
    const int n = (int)(plane / C), c = (int)(plane % C);
    const float *xp = x + plane * HW, *gp = g + plane * HW;
    const size_t go = ((size_t)n * 2 * C + c) * HW, bo = go + (size_t)C * HW;
    const float *gam = gb + go;
    const float m = mean[plane], rs = rstd[plane];
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float xh = (xp[i] - m) * rs;
        const float gi = gp[i];
        const float gh = gi * (1.0f + gam[i]);
        dgb[go + i] = gi * xh;
        dgb[bo + i] = gi;
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
        const float gh = gp[i] * (1.0f + gam[i]);
        op[i] = rs * ((gh - m1) - xh * m2);
    }
}

// ------------------------------------------------------------------ x2 up-sampling + concatenation, backward
// The forward (upsample2x_concat_kernel, csrc/motion.hip) along one axis of length L: out[2k] = .25 in[k - 1] + .75 in[k] (out[0] = in[0]),
// out[2k + 1] = .75 in[k] + .25 in[min(k + 1, L - 1)].  So source k feeds out[2k - 1] with .25 (k >= 1), out[2k] with .75 (1 at k = 0),
// out[2k + 1] with .75 (1 at k = L - 1: the clamped neighbour is k itself) and out[2k + 2] with .25 (k < L - 1).
__device__ __forceinline__ float up2_weight(int j, int k, int L) {      // j = 0 .. 3: output 2k - 1 + j
    if (j == 0) return k >= 1 ? 0.25f : 0.0f;
    if (j == 1) return k == 0 ? 1.0f : 0.75f;
    if (j == 2) return k == L - 1 ? 1.0f : 0.75f;
    return k < L - 1 ? 0.25f : 0.0f;
}

// One thread per source pixel of one (n, channel of the concatenation) plane: it sums the <= 4 x 4 output pixels it feeds, rows in order,
// columns in order (the 2 x 2 block for the nearest channel).  relu = 1: the forward up-sampled relu(src) -- the sum is gated by src > 0;
// relu = 2: the forward was relu(up(src)) -- every g is gated by fwd > 0, fwd the forward's result (for the nearest channel both are the
// same gate).  relu'(0) = 0.
__global__ __launch_bounds__(256) void upsample2x_concat_bwd_kernel(const float *__restrict__ g, const float *__restrict__ fwd,
                                                                    const float *__restrict__ a, const float *__restrict__ b,
                                                                    float *__restrict__ ga, float *__restrict__ gb, int Ca, int Cb, int H,
                                                                    int W, int nearest_channel, int relu) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int y = idx / W, x = idx - y * W;
    const int C = Ca + Cb;
    const int n = blockIdx.y / C, c = blockIdx.y % C;
    const bool from_a = c < Ca;
    const int cs = from_a ? c : c - Ca;
    const size_t so = from_a ? ((size_t)n * Ca + cs) * H * W + idx : ((size_t)n * Cb + cs) * H * W + idx;
    const int OW = 2 * W;
    const size_t po = (size_t)blockIdx.y * 4 * H * W;
    const float *gp = g + po;
    const float *fp = relu == 2 ? fwd + po : nullptr;
    float acc = 0.0f;
    if (cs == nearest_channel) {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const size_t o = (size_t)(2 * y + dy) * OW + 2 * x + dx;
                float e = gp[o];
                if (relu == 2) e = fp[o] > 0.0f ? e : 0.0f;
                acc += e;
            }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float wy = up2_weight(j, y, H);
            const int oy = 2 * y - 1 + j;
            if (wy == 0.0f) continue;                    // (outside the image)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float wx = up2_weight(i, x, W);
                const int ox = 2 * x - 1 + i;
                if (wx == 0.0f) continue;
                const size_t o = (size_t)oy * OW + ox;
                float e = gp[o];
                if (relu == 2) e = fp[o] > 0.0f ? e : 0.0f;
                acc += (wy * wx) * e;
            }
        }
    }
    if (relu == 1) {
        const float s = from_a ? a[so] : b[so];
        acc = s > 0.0f ? acc : 0.0f;
    }
    if (from_a) ga[so] = acc;
    else gb[so] = acc;
}

// ------------------------------------------------------------------ the motion losses
// Per image n, over its H W pixels p with d = pred[n, :, p] - gt[n, :, p] (two channels):
//   sums[n][0] = sum |d|_2 (EndPointError: torch.norm(pred - gt, 2, 1)),  sums[n][1] = sum |d_0| + |d_1| (MotionL1),
//   sums[n][2] = sum |d|_2^2 (PSNR's mse_err before its mean), all in double.
// Launch 1: grid (B, N), workgroup b takes the pixels [b per, (b + 1) per) and writes its three sums; launch 2 adds them in workgroup order.
constexpr int ML_PER = 4096;                              // pixels per workgroup of the first launch, at most

__global__ __launch_bounds__(256) void motion_loss_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                          double *__restrict__ part, int HW, int per) {
    __shared__ double red[3][4];
    const int n = blockIdx.y, b = blockIdx.x;
    const float *p0 = pred + (size_t)n * 2 * HW, *q0 = gt + (size_t)n * 2 * HW;
    const int first = b * per, last = min(first + per, HW);
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = first + threadIdx.x; i < last; i += 256) {
        const float d0 = p0[i] - q0[i], d1 = p0[HW + i] - q0[HW + i];
        const float sq = d0 * d0 + d1 * d1;
        v[0] += (double)sqrtf(sq);
        v[1] += (double)fabsf(d0) + (double)fabsf(d1);
        v[2] += (double)sq;
    }
    block_sum<3, 4>(v, red);
    if (threadIdx.x == 0) {
        double *dst = part + ((size_t)n * gridDim.x + b) * 3;
        dst[0] = v[0];
        dst[1] = v[1];
        dst[2] = v[2];
    }
}

__global__ __launch_bounds__(64) void motion_loss_sum_kernel(const double *__restrict__ part, double *__restrict__ sums, int N, int B) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= N * 3) return;
    const int n = e / 3, k = e - n * 3;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += part[((size_t)n * B + b) * 3 + k];
    sums[e] = s;
}

// gpred = w_epe d / |d|_2 / (N H W)  (exactly 0 where |d|_2 = 0: torch's norm backward)  +  w_l1 sign(d) / (2 N H W); w_epe, w_l1: device
// scalars (the gradients reaching the two means, times the lambdas), either may be absent.
__global__ __launch_bounds__(256) void motion_loss_grad_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                               const float *__restrict__ w_epe, const float *__restrict__ w_l1,
                                                               float *__restrict__ gpred, int HW, float inv_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const size_t o = (size_t)blockIdx.y * 2 * HW + i;
    const float d0 = pred[o] - gt[o], d1 = pred[o + HW] - gt[o + HW];
    float g0 = 0.0f, g1 = 0.0f;
    if (w_epe) {
        const float nrm = sqrtf(d0 * d0 + d1 * d1);
        const float s = w_epe[0] * inv_count;
        if (nrm != 0.0f) {
            g0 = s * (d0 / nrm);
            g1 = s * (d1 / nrm);
        }
    }
    if (w_l1) {
        const float s = w_l1[0] * (0.5f * inv_count);
        g0 += d0 > 0.0f ? s : d0 < 0.0f ? -s : 0.0f;
        g1 += d1 > 0.0f ? s : d1 < 0.0f ? -s : 0.0f;
    }
    gpred[o] = g0;
    gpred[o + HW] = g1;
}

static int ml_blocks(int H, int W) { return (int)(((long long)H * W + ML_PER - 1) / ML_PER); }

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT int slr_instnorm_spade_backward(const float *x, const float *gamma_beta, const float *g, const float *mean, const float *rstd,
                                           float *gx, float *dgamma_beta, int N, int C, int H, int W, void *stream) {
    SLR_CHECK_ARG(x && gamma_beta && g && mean && rstd && gx && dgamma_beta, "null pointer");
    SLR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C < (1LL << 31) && (long long)H * W < (1LL << 31) - 256 &&
                  (long long)H * W >= 4, "sizes (planes of at least 2 x 2)");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)gamma_beta | (uintptr_t)g | (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)gx |
                     (uintptr_t)dgamma_beta) & 3), "4-byte aligned tensors");
    hipLaunchKernelGGL(instnorm_spade_bwd_kernel, dim3((unsigned)(N * C)), dim3(256), 0, (hipStream_t)stream, x, gamma_beta, g, mean, rstd, gx,
                       dgamma_beta, C, H * W);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_upsample2x_concat_backward(const float *g, const float *fwd, const float *a, int Ca, const float *b, int Cb, float *ga,
                                              float *gb, int N, int H, int W, int nearest_channel, int relu, void *stream) {
    SLR_CHECK_ARG(g && ga && (Cb == 0 || gb), "null pointer");
    SLR_CHECK_ARG(relu >= 0 && relu <= 2, "relu: 0 none, 1 before, 2 after the up-sampling");
    SLR_CHECK_ARG(relu != 1 || (a && (Cb == 0 || b)), "relu = 1 needs the sources a (and b)");
    SLR_CHECK_ARG(relu != 2 || fwd, "relu = 2 needs the forward's result");
    SLR_CHECK_ARG(N > 0 && Ca > 0 && Cb >= 0 && H > 0 && W > 0 && (long long)N * (Ca + Cb) < 65536 && 4LL * H * W < (1LL << 31), "sizes");
    hipLaunchKernelGGL(upsample2x_concat_bwd_kernel, dim3((H * W + 255) / 256, N * (Ca + Cb)), dim3(256), 0, (hipStream_t)stream, g, fwd, a, b,
                       ga, gb, Ca, Cb, H, W, nearest_channel, relu);
    SLR_CHECK_LAUNCH();
    return 0;
}

static bool ml_sizes_ok(int N, int H, int W) {
    return N > 0 && N < 65536 && H > 0 && W > 0 && 2LL * H * W < (1LL << 31) && ((long long)H * W + ML_PER - 1) / ML_PER < 65536;
}

SLR_EXPORT size_t slr_motion_loss_ws_bytes(int N, int H, int W) {
    if (!ml_sizes_ok(N, H, W)) return 0;
    return al256((size_t)N * ml_blocks(H, W) * 3 * sizeof(double));
}

SLR_EXPORT int slr_motion_loss(const float *pred, const float *gt, double *sums, int N, int H, int W, void *ws, size_t ws_bytes,
                               void *stream) {
    SLR_CHECK_ARG(pred && gt && sums, "null pointer");
    SLR_CHECK_ARG(ml_sizes_ok(N, H, W), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)pred | (uintptr_t)gt) & 3) && !((uintptr_t)sums & 7), "aligned tensors");
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < slr_motion_loss_ws_bytes(N, H, W)) {
        set_error("%s: ws: slr_motion_loss_ws_bytes(N, H, W) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int B = ml_blocks(H, W);
    hipLaunchKernelGGL(motion_loss_kernel, dim3(B, N), dim3(256), 0, st, pred, gt, (double *)ws, H * W, ML_PER);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(motion_loss_sum_kernel, dim3((N * 3 + 63) / 64), dim3(64), 0, st, (const double *)ws, sums, N, B);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_motion_loss_grad(const float *pred, const float *gt, const float *w_epe, const float *w_l1, float *gpred, int N, int H,
                                    int W, void *stream) {
    SLR_CHECK_ARG(pred && gt && gpred, "null pointer");
    SLR_CHECK_ARG(ml_sizes_ok(N, H, W), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)w_epe | (uintptr_t)w_l1 | (uintptr_t)gpred) & 3), "4-byte aligned tensors");
    const float inv_count = (float)(1.0 / ((double)N * H * W));
    hipLaunchKernelGGL(motion_loss_grad_kernel, dim3((H * W + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, pred, gt, w_epe, w_l1, gpred,
                       H * W, inv_count);
    SLR_CHECK_LAUNCH();
    return 0;
}
