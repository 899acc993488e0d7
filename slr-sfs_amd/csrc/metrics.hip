// metrics.hip -- the clip-evaluation metrics of the reference (evaluation/animation/metrics.py, models/losses/ssim.py,
// models/networks/pretrained_networks.py: PNet "vgg"), ABI 12:
//   * SSIM + squared error of an image pair in one pass (five Gaussian-filtered moments per channel through an LDS tile),
//   * the input scaling of PNet ((x*2 - 1) - shift) / scale, written in the layout the first VGG16 convolution reads,
//   * ReLU + 2x2 / stride 2 max pooling of channel-blocked activations,
//   * the per-pixel cosine distance of two channel-blocked feature maps, 1 - mean_hw(cos).
// The 13 VGG16 convolutions themselves run on slr_conv3x3_forward with SLR_CONV_F32 (csrc/conv.hip).
// Every reduction is deterministic: per-workgroup partial sums in double, written to a caller-owned workspace and added by a second
// launch in a fixed order -- no atomics, and an image's result depends on that image only (not on its batch or its position in it).
#include "slr_common.hpp"
#include "slr_reduce.hpp"

namespace slr {

// ------------------------------------------------------------------ SSIM + squared error
// models/losses/ssim.py:_ssim with the window of create_window (1-D Gaussian, sigma 1.5, normalised, 2-D = outer product) and
// F.conv2d(padding = ws // 2): zero padding.  The 2-D filter is applied as two 1-D passes (row pass into LDS, column pass from LDS) --
// the same weights g[i]*g[j], summed in another order (fp32 rounding).  A workgroup owns SS_TH x SS_TW output pixels of one image and
// loops over its channels; the input patch with its halo of R = ws / 2 pixels is staged once per channel for both images.
constexpr int SS_TW = 64, SS_TH = 16, SS_RMAX = 7, SS_THREADS = 256;
constexpr int SS_PW = SS_TW + 2 * SS_RMAX, SS_PH = SS_TH + 2 * SS_RMAX;
constexpr float SS_C1 = (float)(0.01 * 0.01), SS_C2 = (float)(0.03 * 0.03);      // ssim.py:54-55: Python doubles, fp32 in torch's ops

struct SsimArgs {
    const void *a, *b;           // uint8 [N,H,W,C] or float [N,C,H,W]
    const float *mask;           // [N,1,H,W] or NULL
    double *part;                // [N][tiles][3]: sum of ssim (mask-weighted channel means with a mask), of squared errors, of the mask
    int C, H, W, tiles_x, tiles;
    float g[2 * SS_RMAX + 1];
};

template <bool U8>
__device__ __forceinline__ float ss_load(const void *base, int n, int c, int y, int x, int C, int H, int W) {
    if (U8) return (float)((const unsigned char *)base)[(((size_t)n * H + y) * W + x) * C + c] / 255.0f;   // ToTensor: IEEE division
    return ((const float *)base)[(((size_t)n * C + c) * H + y) * W + x];
}

template <int R, bool U8>
__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(SsimArgs p) {
    constexpr int PH = SS_TH + 2 * R, PW = SS_TW + 2 * R, WS = 2 * R + 1;
    __shared__ float P[2][SS_PH][SS_PW];                 // input patch of both images, halo included
    __shared__ float Hs[5][SS_PH][SS_TW];                // row-filtered x, y, x*x, y*y, x*y
    __shared__ double red[3][SS_THREADS / 64];
    const int n = blockIdx.y, tile = blockIdx.x;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int y0 = ty * SS_TH, x0 = tx * SS_TW;
    const int j = threadIdx.x & 63, i0 = (threadIdx.x >> 6) * 4;      // column pass: column j, rows i0 .. i0 + 3
    const int H = p.H, W = p.W, C = p.C;
    float g[WS];
#pragma unroll
    for (int k = 0; k < WS; ++k) g[k] = p.g[k];
    float ssum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, esum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < C; ++c) {
        for (int idx = threadIdx.x; idx < PH * PW; idx += SS_THREADS) {
            const int r = idx / PW, q = idx - r * PW;
            const int y = y0 - R + r, x = x0 - R + q;
            const bool in = (y >= 0) & (y < H) & (x >= 0) & (x < W);
            P[0][r][q] = in ? ss_load<U8>(p.a, n, c, y, x, C, H, W) : 0.0f;
            P[1][r][q] = in ? ss_load<U8>(p.b, n, c, y, x, C, H, W) : 0.0f;
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < PH * SS_TW; idx += SS_THREADS) {
            const int r = idx >> 6, q = idx & 63;
            float m1 = 0.0f, m2 = 0.0f, s11 = 0.0f, s22 = 0.0f, s12 = 0.0f;
#pragma unroll
            for (int k = 0; k < WS; ++k) {
                const float a = P[0][r][q + k], b = P[1][r][q + k];
                m1 += g[k] * a;
                m2 += g[k] * b;
                s11 += g[k] * (a * a);
                s22 += g[k] * (b * b);
                s12 += g[k] * (a * b);
            }
            Hs[0][r][q] = m1; Hs[1][r][q] = m2; Hs[2][r][q] = s11; Hs[3][r][q] = s22; Hs[4][r][q] = s12;
        }
        __syncthreads();
        float acc[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[m][q] = 0.0f;
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int rr = 0; rr < WS + 3; ++rr) {
                const float v = Hs[m][i0 + rr][j];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (rr - q >= 0 && rr - q < WS) acc[m][q] += g[rr - q] * v;
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) {                    // ssim.py:37-59, in its order of operations
            const float mu1 = acc[0][q], mu2 = acc[1][q];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const float sigma1_sq = acc[2][q] - mu1_sq, sigma2_sq = acc[3][q] - mu2_sq, sigma12 = acc[4][q] - mu1_mu2;
            const float s = ((2.0f * mu1_mu2 + SS_C1) * (2.0f * sigma12 + SS_C2)) /
                            ((mu1_sq + mu2_sq + SS_C1) * (sigma1_sq + sigma2_sq + SS_C2));
            const float d = P[0][R + i0 + q][R + j] - P[1][R + i0 + q][R + j];
            ssum[q] += s;
            esum[q] += d * d;
        }
        __syncthreads();                                 // (before the next channel's staging overwrites P)
    }
    double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = y0 + i0 + q, x = x0 + j;
        if (y >= H || x >= W) continue;
        if (p.mask) {
            const float m = p.mask[((size_t)n * H + y) * W + x];
            v[0] += (double)((ssum[q] / (float)C) * m);    // ssim_map.mean(dim=1) * mask   (ssim.py:61-66)
            v[1] += (double)(esum[q] * m);                 // (img1 - img2)^2 * mask         (metrics.py:12-17)
            v[2] += (double)m;
        } else {
            v[0] += (double)ssum[q];
            v[1] += (double)esum[q];
        }
    }
    block_sum<3, SS_THREADS / 64>(v, red);
    if (threadIdx.x == 0) {
        double *o = p.part + ((size_t)n * p.tiles + tile) * 3;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

// One workgroup per image: the tiles' partial sums in a fixed order -> [ssim, mse].
__global__ __launch_bounds__(256) void ssim_finish_kernel(const double *__restrict__ part, float *__restrict__ out, int tiles,
                                                          int masked, double count) {
    __shared__ double red[3][4];
    const int n = blockIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < tiles; t += 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] += part[((size_t)n * tiles + t) * 3 + k];
    block_sum<3, 4>(v, red);
    if (threadIdx.x == 0) {
        if (masked) {
            const double msum = v[2] < 1.0 ? 1.0 : v[2];                           // .clamp(min=1)
            out[2 * n] = (float)(v[0] / msum);
            out[2 * n + 1] = (float)(v[1] / (3.0 * msum));                        // metrics.py:16-17: 3 * mask sum
        } else {
            out[2 * n] = (float)(v[0] / count);
            out[2 * n + 1] = (float)(v[1] / count);
        }
    }
}

static void ss_tiles(int H, int W, int &tiles_x, int &tiles) {
    tiles_x = (W + SS_TW - 1) / SS_TW;
    tiles = tiles_x * ((H + SS_TH - 1) / SS_TH);
}

template <int R>
static void ssim_launch(bool u8, dim3 grid, const SsimArgs &a, hipStream_t st) {
    if (u8) hipLaunchKernelGGL((ssim_tile_kernel<R, true>), grid, dim3(SS_THREADS), 0, st, a);
    else hipLaunchKernelGGL((ssim_tile_kernel<R, false>), grid, dim3(SS_THREADS), 0, st, a);
}

static void ssim_dispatch(int R, bool u8, dim3 grid, const SsimArgs &a, hipStream_t st) {
    switch (R) {
        case 0: ssim_launch<0>(u8, grid, a, st); break;
        case 1: ssim_launch<1>(u8, grid, a, st); break;
        case 2: ssim_launch<2>(u8, grid, a, st); break;
        case 3: ssim_launch<3>(u8, grid, a, st); break;
        case 4: ssim_launch<4>(u8, grid, a, st); break;
        case 5: ssim_launch<5>(u8, grid, a, st); break;
        case 6: ssim_launch<6>(u8, grid, a, st); break;
        default: ssim_launch<7>(u8, grid, a, st); break;
    }
}

// ------------------------------------------------------------------ PNet input scaling
// perceptual_sim (metrics.py:29): x * 2 - 1, then PNet.forward (pretrained_networks.py:45-46, 73-74): (x - shift) / scale.
__constant__ float VGG_SHIFT[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float VGG_SCALE[3] = {0.458f, 0.448f, 0.450f};

template <bool U8>
__global__ __launch_bounds__(256) void vgg_prep_kernel(const void *__restrict__ img, float *__restrict__ out, long long P, int HW,
                                                       int from01) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const long long n = i / HW, r = i - n * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = U8 ? (float)((const unsigned char *)img)[i * 3 + c] / 255.0f : ((const float *)img)[(n * 3 + c) * HW + r];
        if (from01) x = x * 2.0f - 1.0f;
        out[(n * 3 + c) * HW + r] = (x - VGG_SHIFT[c]) / VGG_SCALE[c];
    }
}

// ------------------------------------------------------------------ ReLU + MaxPool2d(2, 2) on channel-blocked activations
// nn.ReLU then nn.MaxPool2d(kernel_size=2, stride=2) of torchvision's vgg16.features: floor mode; max of relu = relu of max.  The
// training loss runs it too (losses.py), so a NaN in a window makes the window's output NaN, as torch's does (max_nan).
__global__ __launch_bounds__(256) void relu_maxpool2_b8_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, long long total,
                                                               int H, int W, int OH, int OW) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long plane = i / ((long long)OH * OW);
    const int r = (int)(i - plane * OH * OW), oy = r / OW, ox = r - oy * OW;
    const float4 *src = in + (plane * H * W + (long long)(2 * oy) * W + 2 * ox) * 2;
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const float4 a = src[((size_t)dy * W + dx) * 2], b = src[((size_t)dy * W + dx) * 2 + 1];
            lo.x = max_nan(lo.x, a.x); lo.y = max_nan(lo.y, a.y); lo.z = max_nan(lo.z, a.z); lo.w = max_nan(lo.w, a.w);
            hi.x = max_nan(hi.x, b.x); hi.y = max_nan(hi.y, b.y); hi.z = max_nan(hi.z, b.z); hi.w = max_nan(hi.w, b.w);
        }
    out[i * 2] = lo;
    out[i * 2 + 1] = hi;
}

// ------------------------------------------------------------------ feature distance
// cos_sim of pretrained_networks.py:11-31 on ReLU'd features: normalize_tensor divides by (||f||_2 over channels + 1e-10), so the
// channel sum of the product of the two normalised maps is dot / ((|f0| + eps) (|f1| + eps)).  One pass over the channels gathers the
// per-pixel channel sums (PixelSums), cos_term turns them into the pixel's term.  (LPIPS's per-channel weighted squared difference of the
// normalised maps expands into weighted sums of f0^2, f1^2 and f0 f1 over the same pass: another accumulator and term of this shape.)
constexpr int FD_THREADS = 256;
constexpr float FD_EPS = 1e-10f;

struct PixelSums {
    float s00 = 0.0f, s11 = 0.0f, s01 = 0.0f;
    __device__ __forceinline__ void add(float a, float b) { s00 += a * a; s11 += b * b; s01 += a * b; }
    __device__ __forceinline__ void add4(float4 a, float4 b) {
        add(fmaxf(a.x, 0.0f), fmaxf(b.x, 0.0f)); add(fmaxf(a.y, 0.0f), fmaxf(b.y, 0.0f));
        add(fmaxf(a.z, 0.0f), fmaxf(b.z, 0.0f)); add(fmaxf(a.w, 0.0f), fmaxf(b.w, 0.0f));
    }
    __device__ __forceinline__ float cos_term() const { return s01 / ((sqrtf(s00) + FD_EPS) * (sqrtf(s11) + FD_EPS)); }
};

__global__ __launch_bounds__(FD_THREADS) void feature_cos_kernel(const float4 *__restrict__ f0, const float4 *__restrict__ f1,
                                                                 double *__restrict__ part, int CB, int HW, int blocks) {
    __shared__ double red[1][FD_THREADS / 64];
    const int n = blockIdx.y, p = blockIdx.x * FD_THREADS + threadIdx.x;
    double v[1] = {0.0};
    if (p < HW) {
        PixelSums s;
        const size_t base = (size_t)n * CB * HW;
        for (int cb = 0; cb < CB; ++cb) {
            const size_t o = (base + (size_t)cb * HW + p) * 2;
            s.add4(f0[o], f1[o]);
            s.add4(f0[o + 1], f1[o + 1]);
        }
        v[0] = (double)s.cos_term();
    }
    block_sum<1, FD_THREADS / 64>(v, red);
    if (threadIdx.x == 0) part[(size_t)n * blocks + blockIdx.x] = v[0];
}

__global__ __launch_bounds__(256) void feature_cos_finish_kernel(const double *__restrict__ part, float *__restrict__ out, int blocks,
                                                                 double hw) {
    __shared__ double red[1][4];
    const int n = blockIdx.x;
    double v[1] = {0.0};
    for (int t = threadIdx.x; t < blocks; t += 256) v[0] += part[(size_t)n * blocks + t];
    block_sum<1, 4>(v, red);
    if (threadIdx.x == 0) out[n] = (float)(1.0 - v[0] / hw);
}

static int fd_blocks(int H, int W) { return (int)(((long long)H * W + FD_THREADS - 1) / FD_THREADS); }

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT size_t slr_ssim_ws_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    int tiles_x = 0, tiles = 0;
    ss_tiles(H, W, tiles_x, tiles);
    return (size_t)N * tiles * 3 * sizeof(double);
}

SLR_EXPORT int slr_ssim_mse(const void *img1, const void *img2, int u8, const float *mask, float *out, int N, int C, int H, int W,
                            int window_size, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(img1 && img2 && out && ws, "null pointer");
    SLR_CHECK_ARG(N > 0 && N < 65536 && C > 0 && C <= 64 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) - 2 * SS_TW &&
                  (long long)N * C * H * W < (1LL << 40), "sizes");      // (a column past the last tile's halo stays an int)
    SLR_CHECK_ARG(window_size >= 1 && window_size <= 2 * SS_RMAX + 1 && window_size % 2 == 1, "window_size: odd, 1 .. 15");
    SLR_CHECK_ARG(ws_bytes >= slr_ssim_ws_bytes(N, H, W) && !((uintptr_t)ws & 7), "ws: slr_ssim_ws_bytes(N, H, W), 8-byte aligned");
    SsimArgs a = {};
    a.a = img1; a.b = img2; a.mask = mask; a.part = (double *)ws;
    a.C = C; a.H = H; a.W = W;
    ss_tiles(H, W, a.tiles_x, a.tiles);
    // gaussian(window_size, 1.5) of ssim.py:12-19: exp() of Python doubles stored as fp32, normalised by their fp32 sum
    const int R = window_size / 2;
    float sum = 0.0f;
    for (int k = 0; k < window_size; ++k) {
        a.g[k] = (float)exp(-(double)((k - R) * (k - R)) / (2.0 * 1.5 * 1.5));
        sum += a.g[k];
    }
    for (int k = 0; k < window_size; ++k) a.g[k] /= sum;
    hipStream_t st = (hipStream_t)stream;
    ssim_dispatch(R, u8 != 0, dim3(a.tiles, N), a, st);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(N), dim3(256), 0, st, (const double *)ws, out, a.tiles, mask ? 1 : 0,
                       (double)C * H * W);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_vgg_prep(const void *img, int u8, int from01, float *out, int N, int H, int W, void *stream) {
    SLR_CHECK_ARG(img && out, "null pointer");
    SLR_CHECK_ARG(N > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) && (long long)N * H * W < (1LL << 40), "sizes");
    SLR_CHECK_ARG(!u8 || from01, "uint8 frames are in [0, 255]: from01 = 1");
    const long long P = (long long)N * H * W;
    const dim3 grid((unsigned)((P + 255) / 256));
    if (u8) hipLaunchKernelGGL(vgg_prep_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, img, out, P, H * W, from01);
    else hipLaunchKernelGGL(vgg_prep_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, img, out, P, H * W, from01);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_relu_maxpool2x2_b8(const float *in, float *out, int N, int C, int H, int W, void *stream) {
    SLR_CHECK_ARG(in && out, "null pointer");
    SLR_CHECK_ARG(!((uintptr_t)in & 15) && !((uintptr_t)out & 15), "16-byte aligned tensors");
    SLR_CHECK_ARG(N > 0 && C > 0 && C % 8 == 0 && H >= 2 && W >= 2 && (long long)N * C * H * W < (1LL << 40),
                  "sizes (C % 8 == 0, H, W >= 2)");
    const int OH = H / 2, OW = W / 2;
    const long long total = (long long)N * (C / 8) * OH * OW;
    hipLaunchKernelGGL(relu_maxpool2_b8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)in, (float4 *)out, total, H, W, OH, OW);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_feature_cos_ws_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)N * fd_blocks(H, W) * sizeof(double);
}

SLR_EXPORT int slr_feature_cos_distance(const float *f0, const float *f1, float *out, int N, int C, int H, int W, void *ws,
                                        size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(f0 && f1 && out && ws, "null pointer");
    SLR_CHECK_ARG(!((uintptr_t)f0 & 15) && !((uintptr_t)f1 & 15), "16-byte aligned feature maps");
    SLR_CHECK_ARG(N > 0 && N < 65536 && C > 0 && C % 8 == 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) - FD_THREADS &&
                  (long long)N * C * H * W < (1LL << 40), "sizes (C % 8 == 0)");
    SLR_CHECK_ARG(ws_bytes >= slr_feature_cos_ws_bytes(N, H, W) && !((uintptr_t)ws & 7), "ws: slr_feature_cos_ws_bytes(N, H, W)");
    const int blocks = fd_blocks(H, W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(feature_cos_kernel, dim3(blocks, N), dim3(FD_THREADS), 0, st, (const float4 *)f0, (const float4 *)f1,
                       (double *)ws, C / 8, H * W, blocks);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(feature_cos_finish_kernel, dim3(N), dim3(256), 0, st, (const double *)ws, out, blocks, (double)H * W);
    SLR_CHECK_LAUNCH();
    return 0;
}
