// loss.hip -- the device code around the convolutions of the training loss (models/losses/synthesis.py), ABI 14:
//   * nn.L1Loss of an image pair with its gradient (synthesis.py:134-140),
//   * one pass over a VGG19 slice's raw features: the slice's L1 distance of the ReLU'd features (PerceptualLoss, synthesis.py:166-185),
//     and the gradient at the raw feature -- the distance's own (seed) plus the one arriving from the layers above, through the ReLU gate,
//   * the backward of ReLU + MaxPool2d(2, 2) on channel-blocked activations.
// The VGG19 convolutions and their backward-data convolutions (the same 3x3 convolution with flipped, transposed weights) run on
// slr_conv3x3_forward with SLR_CONV_F32 (csrc/conv.hip).  Nothing here synchronises; there are no atomics: sums are per-workgroup partial
// sums in double (slr_reduce.hpp), added by a second launch in a fixed order, so every result has the same bits from run to run.
#include "slr_common.hpp"
#include "slr_reduce.hpp"

namespace slr {

constexpr int LS_THREADS = 256;
constexpr int LS_L1_PER_BLOCK = LS_THREADS * 4;          // l1_loss_grad_kernel: 4 elements per thread
constexpr int LS_GATE_PER_BLOCK = LS_THREADS * 8;        // feature_l1_gate_kernel: 8 channels of one pixel (two 16-byte words) per thread

__device__ __forceinline__ float sign_of(float d) { return (float)(d > 0.0f) - (float)(d < 0.0f); }      // torch.sign: sign(0) = 0

// ------------------------------------------------------------------ nn.L1Loss + gradient
// Elements 4 i .. 4 i + 3 per thread: one 16-byte load per tensor where the tensors are aligned and the four are inside, else scalar.
__global__ __launch_bounds__(LS_THREADS) void l1_loss_grad_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                  float *__restrict__ grad, double *__restrict__ part, long long n,
                                                                  int aligned, float coef, const float *__restrict__ gscale) {
    __shared__ double red[1][LS_THREADS / 64];
    const long long e0 = ((long long)blockIdx.x * LS_THREADS + threadIdx.x) * 4;
    const long long left = n - e0;
    const int cnt = left >= 4 ? 4 : left > 0 ? (int)left : 0;
    const float k = grad ? coef * gscale[0] : 0.0f;
    float p[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4];
    const bool vec = aligned && cnt == 4;
    if (vec) {
        const float4 P = *(const float4 *)(pred + e0), G = *(const float4 *)(gt + e0);
        p[0] = P.x; p[1] = P.y; p[2] = P.z; p[3] = P.w;
        g[0] = G.x; g[1] = G.y; g[2] = G.z; g[3] = G.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) { p[e] = pred[e0 + e]; g[e] = gt[e0 + e]; }
    }
    double v[1] = {0.0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {                        // (elements past the end: p = g = 0, no contribution)
        const float d = p[e] - g[e];
        v[0] += (double)fabsf(d);
        o[e] = sign_of(d) * k;
    }
    if (grad) {
        if (vec) *(float4 *)(grad + e0) = make_float4(o[0], o[1], o[2], o[3]);
        else
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) grad[e0 + e] = o[e];
    }
    if (part) {                                          // (uniform over the grid)
        block_sum<1, LS_THREADS / 64>(v, red);
        if (threadIdx.x == 0) part[blockIdx.x] = v[0];
    }
}

// The workgroups' partial sums in a fixed order -> out[0] = sum * scale.
__global__ __launch_bounds__(256) void loss_sum_finish_kernel(const double *__restrict__ part, float *__restrict__ out, int blocks,
                                                              double scale) {
    __shared__ double red[1][4];
    double v[1] = {0.0};
    for (int t = threadIdx.x; t < blocks; t += 256) v[0] += part[t];
    block_sum<1, 4>(v, red);
    if (threadIdx.x == 0) out[0] = (float)(v[0] * scale);
}

// ------------------------------------------------------------------ slice distance + seed + ReLU gate
// Per element of the raw feature a (prediction), b (ground truth) and the gradient g arriving from the layer above:
//   d = relu(a) - relu(b);  sum += |d|;  out = a <= 0 ? 0 : g + sign(d) * k     (k = coef * gscale[0], formed once, fp32)
// without b: out = a <= 0 ? 0 : g, the ReLU backward of a layer that ends no slice.  Every operation is the fp32 one torch would do.
template <bool HAS_B>
__device__ __forceinline__ float gate_elem(float a, float b, float g, float k, double &sum) {
    float v = g;
    if (HAS_B) {
        const float d = relu_nan(a) - relu_nan(b);       // (a NaN feature makes the sum NaN; sign(NaN) = 0, torch.sign's)
        sum += (double)fabsf(d);
        v = g + sign_of(d) * k;
    }
    return a <= 0.0f ? 0.0f : v;                         // torch's ReLU backward: closed on `<= 0` only, open for a NaN a
}

template <bool HAS_B>
__device__ __forceinline__ float4 gate4(float4 a, float4 b, float4 g, float k, double &sum) {
    return make_float4(gate_elem<HAS_B>(a.x, b.x, g.x, k, sum), gate_elem<HAS_B>(a.y, b.y, g.y, k, sum),
                       gate_elem<HAS_B>(a.z, b.z, g.z, k, sum), gate_elem<HAS_B>(a.w, b.w, g.w, k, sum));
}

template <bool HAS_B>
__global__ __launch_bounds__(LS_THREADS) void feature_l1_gate_kernel(const float4 *__restrict__ a, const float4 *__restrict__ b,
                                                                     const float4 *__restrict__ g_in, float4 *__restrict__ g_out,
                                                                     double *__restrict__ part, long long n8, float coef,
                                                                     const float *__restrict__ gscale) {
    __shared__ double red[1][LS_THREADS / 64];
    const long long i = (long long)blockIdx.x * LS_THREADS + threadIdx.x;
    double v[1] = {0.0};
    if (i < n8) {
        const float k = (HAS_B && g_out) ? coef * gscale[0] : 0.0f;
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long o = i * 2 + h;
            const float4 o4 = gate4<HAS_B>(a[o], HAS_B ? b[o] : zero, g_in ? g_in[o] : zero, k, v[0]);
            if (g_out) g_out[o] = o4;
        }
    }
    if (HAS_B && part) {                                 // (uniform over the grid)
        block_sum<1, LS_THREADS / 64>(v, red);
        if (threadIdx.x == 0) part[blockIdx.x] = v[0];
    }
}

// ------------------------------------------------------------------ backward of ReLU + MaxPool2d(2, 2)
// One thread per 2x2 window of the INPUT grid rounded up (so the last row / column of an odd H / W belongs to a thread too) and 8
// channels: a complete window sends its pooled gradient to its first maximum in row-major order (torch's max_pool2d keeps the first:
// it replaces on `>` -- or on a NaN, so a window with NaNs sends it to its last NaN) if that maximum is > 0 or NaN (the ReLU), zero
// to the other three; an incomplete one (floor mode: not pooled) writes zeros.  Every output element is written exactly once.
__device__ __forceinline__ void route1(float x0, float x1, float x2, float x3, float g, float &o0, float &o1, float &o2, float &o3) {
    float best = x0;
    int at = 0;
    if (x1 > best || x1 != x1) { best = x1; at = 1; }    // torch's rule: replace on `>` or on a NaN -- the LAST NaN of a window wins
    if (x2 > best || x2 != x2) { best = x2; at = 2; }
    if (x3 > best || x3 != x3) { best = x3; at = 3; }
    const float r = best <= 0.0f ? 0.0f : g;             // torch's ReLU backward: closed on `<= 0` only, so open for a NaN
    o0 = at == 0 ? r : 0.0f;
    o1 = at == 1 ? r : 0.0f;
    o2 = at == 2 ? r : 0.0f;
    o3 = at == 3 ? r : 0.0f;
}

__global__ __launch_bounds__(LS_THREADS) void relu_maxpool2_backward_b8_kernel(const float4 *__restrict__ x, const float4 *__restrict__ g,
                                                                               float4 *__restrict__ out, long long total, int H, int W,
                                                                               int PH, int PW) {
    const long long i = (long long)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= total) return;
    const int OH = H / 2, OW = W / 2;
    const long long plane = i / ((long long)PH * PW);
    const int r = (int)(i - plane * PH * PW), py = r / PW, px = r - py * PW;
    const int y0 = 2 * py, x0 = 2 * px;
    const bool right = x0 + 1 < W, below = y0 + 1 < H;
    const long long base = (plane * H * W + (long long)y0 * W + x0) * 2;        // (in 16-byte words; y0 < H and x0 < W always)
    const long long row = (long long)W * 2;
    if (right && below) {
        const long long gb = (plane * OH * OW + (long long)py * OW + px) * 2;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 a = x[base + h], b = x[base + 2 + h], c = x[base + row + h], d = x[base + row + 2 + h], gg = g[gb + h];
            float4 oa, ob, oc, od;
            route1(a.x, b.x, c.x, d.x, gg.x, oa.x, ob.x, oc.x, od.x);
            route1(a.y, b.y, c.y, d.y, gg.y, oa.y, ob.y, oc.y, od.y);
            route1(a.z, b.z, c.z, d.z, gg.z, oa.z, ob.z, oc.z, od.z);
            route1(a.w, b.w, c.w, d.w, gg.w, oa.w, ob.w, oc.w, od.w);
            out[base + h] = oa; out[base + 2 + h] = ob; out[base + row + h] = oc; out[base + row + 2 + h] = od;
        }
    } else {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            out[base + h] = zero;
            if (right) out[base + 2 + h] = zero;
            if (below) out[base + row + h] = zero;
        }
    }
}

static long long ls_blocks(long long count, int per_block) { return (count + per_block - 1) / per_block; }

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT size_t slr_loss_ws_bytes(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)ls_blocks((long long)N * C * H * W, LS_L1_PER_BLOCK) * sizeof(double);      // (covers the gate kernel's fewer workgroups)
}

SLR_EXPORT int slr_l1_loss_grad(const float *pred, const float *gt, float *loss, float *grad, float coef, const float *gscale,
                                int N, int C, int H, int W, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(pred && gt && (loss || grad), "null pointer");
    SLR_CHECK_ARG(!grad || gscale, "null pointer: grad needs gscale");
    SLR_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * C * H * W < (1LL << 40), "sizes");
    SLR_CHECK_ARG(!loss || (ws && ws_bytes >= slr_loss_ws_bytes(N, C, H, W) && !((uintptr_t)ws & 7)),
                  "ws: slr_loss_ws_bytes(N, C, H, W), 8-byte aligned");
    const long long n = (long long)N * C * H * W, blocks = ls_blocks(n, LS_L1_PER_BLOCK);
    const int aligned = !(((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)grad) & 15);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l1_loss_grad_kernel, dim3((unsigned)blocks), dim3(LS_THREADS), 0, st, pred, gt, grad,
                       loss ? (double *)ws : nullptr, n, aligned, coef, gscale);
    SLR_CHECK_LAUNCH();
    if (loss) {
        hipLaunchKernelGGL(loss_sum_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)ws, loss, (int)blocks, 1.0 / (double)n);
        SLR_CHECK_LAUNCH();
    }
    return 0;
}

SLR_EXPORT int slr_feature_l1_gate_b8(const float *a, const float *b, const float *g_in, float *sum, float *g_out, float coef,
                                      const float *gscale, int N, int C, int H, int W, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(a && (sum || g_out), "null pointer");
    SLR_CHECK_ARG(!sum || b, "null pointer: the sum needs b");
    SLR_CHECK_ARG(b || g_in, "null pointer: without b, g_in is the gradient to gate");
    SLR_CHECK_ARG(!(b && g_out) || gscale, "null pointer: the seed needs gscale");
    SLR_CHECK_ARG(!(((uintptr_t)a | (uintptr_t)b | (uintptr_t)g_in | (uintptr_t)g_out) & 15), "16-byte aligned tensors");
    SLR_CHECK_ARG(N > 0 && C > 0 && C % 8 == 0 && H > 0 && W > 0 && (long long)N * C * H * W < (1LL << 40), "sizes (C % 8 == 0)");
    SLR_CHECK_ARG(!sum || (ws && ws_bytes >= slr_loss_ws_bytes(N, C, H, W) && !((uintptr_t)ws & 7)),
                  "ws: slr_loss_ws_bytes(N, C, H, W), 8-byte aligned");
    const long long n8 = (long long)N * C * H * W / 8, blocks = ls_blocks(n8, LS_THREADS);
    hipStream_t st = (hipStream_t)stream;
    double *part = sum ? (double *)ws : nullptr;
    if (b) hipLaunchKernelGGL(feature_l1_gate_kernel<true>, dim3((unsigned)blocks), dim3(LS_THREADS), 0, st, (const float4 *)a,
                              (const float4 *)b, (const float4 *)g_in, (float4 *)g_out, part, n8, coef, gscale);
    else hipLaunchKernelGGL(feature_l1_gate_kernel<false>, dim3((unsigned)blocks), dim3(LS_THREADS), 0, st, (const float4 *)a,
                            (const float4 *)nullptr, (const float4 *)g_in, (float4 *)g_out, part, n8, coef, gscale);
    SLR_CHECK_LAUNCH();
    if (sum) {
        hipLaunchKernelGGL(loss_sum_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)ws, sum, (int)blocks, 1.0);
        SLR_CHECK_LAUNCH();
    }
    return 0;
}

SLR_EXPORT int slr_relu_maxpool2x2_backward_b8(const float *x, const float *g, float *out, int N, int C, int H, int W, void *stream) {
    SLR_CHECK_ARG(x && g && out, "null pointer");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)g | (uintptr_t)out) & 15), "16-byte aligned tensors");
    SLR_CHECK_ARG(N > 0 && C > 0 && C % 8 == 0 && H >= 2 && W >= 2 && (long long)N * C * H * W < (1LL << 40),
                  "sizes (C % 8 == 0, H, W >= 2)");
    const int PH = (H + 1) / 2, PW = (W + 1) / 2;
    const long long total = (long long)N * (C / 8) * PH * PW;
    hipLaunchKernelGGL(relu_maxpool2_backward_b8_kernel, dim3((unsigned)ls_blocks(total, LS_THREADS)), dim3(LS_THREADS), 0,
                       (hipStream_t)stream, (const float4 *)x, (const float4 *)g, (float4 *)out, total, H, W, PH, PW);
    SLR_CHECK_LAUNCH();
    return 0;
}
