// conv4x4.hip -- the 4x4 convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32 (fp32 operands, products and accumulation: the
// arithmetic of the fp32 rung), one kernel body and one launch rule for
//   * the encoder convolution of the motion U-Nets: stride 2, padding 1, LeakyReLU of the input, bias + per-channel affine epilogue
//     (slr_conv4x4s2_*; the rest of those networks: csrc/motion.hip);
//   * Conv2d(Cin, Cout, 4, stride 1 or 2, padding 2) of the discriminator, optional bias and LeakyReLU of the output (slr_conv4x4_forward);
//   * its gradient to the input as a gather: a 4x4 / pad 1 correlation with the flipped weights at stride 1, the 2x2 taps of the pixel's
//     parity class at stride 2 (K = 4 Cout) -- every element of gin is stored once (slr_conv4x4_backward_data; the weight gradient and the
//     rest of the discriminator: csrc/disc.hip).
// Everything is NCHW fp32; nothing synchronises; no atomics: the same inputs give the same bits.
#include "slr_common.hpp"
#include "conv4x4.hpp"

namespace slr {

// GEMM view: out[m][p] = sum_k a[m][k] * b[k][p]; m = the channel that is produced, k = (the channel that is summed, a tap), p = a pixel
// of the produced tensor, flat over the whole batch (small deep layers of several samples share one tile).  Lane l of a
// v_mfma_f32_32x32x2_f32 holds A[l & 31][k0 + (l >> 5)] and B[k0 + (l >> 5)][l & 31].
//   C4_FWD1 / C4_FWD2  out = conv(in, w): 16 taps = 8 steps per summed channel ci; step s: ky = s >> 1, kx = 2 (s & 1) + (l >> 5); the tap
//                      reads in[S oy - 2 + ky][S ox - 2 + kx].
//   C4_ENC2            C4_FWD2 with padding 1: the tap reads in[2 oy - 1 + ky][2 ox - 1 + kx].
//   C4_BWD1            gin = the stride-1 adjoint: 8 steps per summed channel co; step s: ty = s >> 1, tx = 2 (s & 1) + (l >> 5) reads
//                      g[iy - 1 + ty][ix - 1 + tx] against w[co][ci][3 - ty][3 - tx].
//   C4_BWD2            gin = the stride-2 adjoint.  Pixel (iy, ix) = (2a + py, 2b + px) of parity class (py, px) = blockIdx.z gets the taps
//                      ky = py + 2 ty, kx = px + 2 tx (the ones for which (iy + 2 - ky) / 2 is exact): 2 steps per co; step s: ty = s,
//                      tx = l >> 5 reads g[a + 1 - ty][b + 1 - tx].  A tile's 32 pixels are of one class, so they share the A fragment.
//   C4_ENCB2           gin = the adjoint of C4_ENC2 (stride 2, padding 1): iy = 2 oy - 1 + ky, so class (py, px) gets the taps
//                      ky = (1 - py) + 2 ty, kx = (1 - px) + 2 tx and reads g[a + py - ty][b + px - tx].  Those are the taps of C4_BWD2's
//                      class (1 - py, 1 - px): the C4_BWD2 fragments serve, read at class cls ^ 3 -- no preparation of its own.
// Weight fragments (one coalesced 256-byte load per MFMA), T = ceil(produced channels / 32), zero beyond the last channel:
//   forward   wf[((ct Cin + ci) 8 + s) 64 + l]                = w[32 ct + (l & 31)][ci][s >> 1][2 (s & 1) + (l >> 5)] * scale
//   C4_BWD1   wf[((ct Cout + co) 8 + s) 64 + l]               = w[co][32 ct + (l & 31)][3 - (s >> 1)][3 - 2 (s & 1) - (l >> 5)] * scale
//   C4_BWD2   wf[(((cls T + ct) Cout + co) 2 + s) 64 + l]     = w[co][32 ct + (l & 31)][py + 2 s][px + 2 (l >> 5)] * scale, cls = 2 py + px
// scale: a device scalar or none -- the 1 / sigma of spectral normalisation costs no pass of its own and no host synchronisation.
// (tools/disc_train_bench.py sorts the kernels of a trace by the first template argument: 0 / 1 forward, 2 / 3 backward-data of the
// discriminator; C4_ENC2 is neither.)
enum { C4_FWD1 = 0, C4_FWD2 = 1, C4_BWD1 = 2, C4_BWD2 = 3, C4_ENC2 = 4, C4_ENCB2 = 5 };

__global__ __launch_bounds__(256) void conv4x4_weights_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                                              float *__restrict__ wf, int Cout, int Cin, int mode, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63), c = lane & 31, h = lane >> 5;
    long long rest = idx >> 6;
    int co, ci, ky, kx;
    bool ok;
    if (mode == C4_BWD2) {
        const int T = (Cin + 31) / 32;
        const int s = (int)(rest & 1);
        rest >>= 1;
        co = (int)(rest % Cout);
        rest /= Cout;
        const int ct = (int)(rest % T), cls = (int)(rest / T);
        ci = ct * 32 + c;
        ky = (cls >> 1) + 2 * s;
        kx = (cls & 1) + 2 * h;
        ok = ci < Cin;
    } else {
        const int s = (int)(rest & 7);
        rest >>= 3;
        if (mode == C4_BWD1) {
            co = (int)(rest % Cout);
            ci = (int)(rest / Cout) * 32 + c;
            ky = 3 - (s >> 1);
            kx = 3 - 2 * (s & 1) - h;
            ok = ci < Cin;
        } else {
            ci = (int)(rest % Cin);
            co = (int)(rest / Cin) * 32 + c;
            ky = s >> 1;
            kx = 2 * (s & 1) + h;
            ok = co < Cout;
        }
    }
    float v = 0.0f;
    if (ok) {
        v = w[(((size_t)co * Cin + ci) * 4 + ky) * 4 + kx];
        if (scale) v *= scale[0];
    }
    wf[idx] = v;
}

// One workgroup = CT tiles of 32 produced channels x one tile of 32 pixels; its KW waves split the summed channels (wave w takes
// c = w, w + KW, ...) and wave 0 adds their accumulators from LDS in wave order (deterministic).  KW > 1 serves the deep layers, whose
// M * N is a few tiles while K reaches 4096.  `in` [N,Ck,IH,IW] is what is read, `out` [N,Cm,OH,OW] what is produced.
// F: C4_FWD1 / C4_FWD2 -- LeakyReLU of the output; C4_ENC2 -- LeakyReLU of the value read (leaky_relu(0) = 0: zero padding before or
// after it is the same); backward -- the value read is g * (gate > 0 ? 1 : slope) with `gate` a tensor of g's shape (the LeakyReLU output
// of the layer whose gradient this is).  Epilogue: C4_FWD1 / C4_FWD2 add `bias` if there is one; C4_ENC2 adds bias or 0, then
// y * post_scale[c] + post_shift[c] if there is a scale; C4_ENCB2 -- F: the result times (gate > 0 ? 1 : slope) with `gate` the raw input
// of the convolution, a tensor of gin's shape (the LeakyReLU sits in front of the encoder convolution, so its gate is applied to what is
// produced, not to what is read).  Every mode reads only its own pointers; MODE and F are resolved at compile time.
template <int MODE, int CT, bool F>
__global__ __launch_bounds__(1024) void conv4x4_kernel(const float *__restrict__ in, const float *__restrict__ gate,
                                                       const float *__restrict__ wf, const float *__restrict__ bias,
                                                       const float *__restrict__ post_scale, const float *__restrict__ post_shift,
                                                       float *__restrict__ out, int N, int Ck, int Cm, int IH, int IW, int OH, int OW,
                                                       float slope) {
    constexpr bool BWD = MODE == C4_BWD1 || MODE == C4_BWD2;
    constexpr bool PAR = MODE == C4_BWD2 || MODE == C4_ENCB2;   // one launch per parity class of the produced pixels
    constexpr int NS = PAR ? 2 : 8;
    extern __shared__ float red[];                       // [KW-1][CT*16][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, KW = blockDim.x >> 6;
    const int cls = PAR ? blockIdx.z : 0, py = cls >> 1, px = cls & 1;
    const int wcls = MODE == C4_ENCB2 ? cls ^ 3 : cls;   // the class whose weight fragments hold this class's taps
    // the pixel grid of this launch: the whole produced tensor, or its pixels of one parity class
    const int PH = PAR ? (OH - py + 1) / 2 : OH, PW = PAR ? (OW - px + 1) / 2 : OW;
    const int PHW = PH * PW;
    const long long P = (long long)N * PHW;
    if ((long long)blockIdx.x * 32 >= P) return;         // (uniform over the workgroup; an empty class has P = 0)
    const long long p = (long long)blockIdx.x * 32 + (lane & 31);
    const bool pv = p < P;
    const int pp = pv ? (int)p : 0;
    const int n = pp / PHW, r = pp - n * PHW, a = r / PW, b = r - a * PW;
    const int h = lane >> 5;
    int off[NS];
    bool ok[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        int iy, ix;
        if (MODE == C4_BWD2) {
            iy = a + 1 - s;
            ix = b + 1 - h;
        } else if (MODE == C4_ENCB2) {
            iy = a + py - s;
            ix = b + px - h;
        } else {
            const int S = MODE == C4_FWD1 || MODE == C4_BWD1 ? 1 : 2, PAD = MODE == C4_FWD1 || MODE == C4_FWD2 ? 2 : 1;
            iy = S * a - PAD + (s >> 1);
            ix = S * b - PAD + 2 * (s & 1) + h;
        }
        ok[s] = pv & (iy >= 0) & (iy < IH) & (ix >= 0) & (ix < IW);
        off[s] = ok[s] ? iy * IW + ix : 0;
    }
    const size_t IHW = (size_t)IH * IW;
    const float *ip = in + (size_t)n * Ck * IHW;
    const float *gp = (BWD && F) ? gate + (size_t)n * Ck * IHW : nullptr;
    const int ct0 = blockIdx.y * CT, T = gridDim.y * CT;
    f32x16 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    for (int c = wave; c < Ck; c += KW) {
        const float *pl = ip + (size_t)c * IHW;
        float bv[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float v = pl[off[s]];
            if (BWD && F) v *= gp[(size_t)c * IHW + off[s]] > 0.0f ? 1.0f : slope;
            v = ok[s] ? v : 0.0f;
            bv[s] = (MODE == C4_ENC2 && F) ? (v > 0.0f ? v : v * slope) : v;
        }
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const float *af = wf + (((size_t)wcls * T + ct0 + t) * Ck + c) * (NS * 64) + lane;
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s * 64], bv[s], acc[t], 0, 0, 0);
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
    const size_t OHW = (size_t)OH * OW;
    const size_t o0 = (size_t)n * Cm * OHW + (PAR ? (size_t)(2 * a + py) * OW + 2 * b + px : (size_t)r);
    float *op = out + o0;
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int cm = (ct0 + t) * 32 + mfma32_row(q, h);
            if (cm < Cm) {
                float y = acc[t][q];
                if (MODE == C4_ENC2) {
                    y = y + (bias ? bias[cm] : 0.0f);        // (+ 0 without a bias: -0 leaves as +0)
                    if (post_scale) y = y * post_scale[cm] + post_shift[cm];
                } else if (MODE == C4_ENCB2) {
                    if (F) y *= gate[o0 + (size_t)cm * OHW] > 0.0f ? 1.0f : slope;
                } else if (!BWD) {
                    if (bias) y += bias[cm];
                    if (F) y = y > 0.0f ? y : y * slope;
                }
                op[(size_t)cm * OHW] = y;
            }
        }
}

// The launch rule.  `pixels`: of the largest pixel grid of the launch; ntile tiles of produced channels; Ck summed channels.
template <int MODE, bool F>
static void c4_launch(const float *in, const float *gate, const float *wf, const float *bias, const float *post_scale,
                      const float *post_shift, float *out, int N, int Ck, int Cm, int IH, int IW, int OH, int OW, long long pixels,
                      float slope, hipStream_t st) {
    const int ntile = c4_tiles(Cm);
    const long long ptiles = (pixels + 31) / 32;
    // CT channel tiles per workgroup (the taps are loaded once for all of them); launches of a few tiles take one and split K over up to
    // 16 waves instead, so that the deep layers fill the chip.  LDS of the K split: (KW - 1) * CT * 4 KiB <= 60 KiB.
    int CT = ntile % 4 == 0 ? 4 : ntile % 2 == 0 ? 2 : 1;
    const int classes = MODE == C4_BWD2 || MODE == C4_ENCB2 ? 4 : 1;
    if (ptiles * classes * (ntile / CT) < 512) CT = 1;
    const long long wgs = ptiles * classes * (ntile / CT);
    int KW = 1;
    while (KW < 16 / CT && wgs * KW < 2048 && 2 * KW <= Ck) KW *= 2;
    const dim3 grid((unsigned)ptiles, ntile / CT, classes);
    const size_t lds = (size_t)(KW - 1) * CT * 16 * 64 * sizeof(float);
#define C4_LAUNCH(T) hipLaunchKernelGGL((conv4x4_kernel<MODE, T, F>), grid, dim3(64 * KW), lds, st, in, gate, wf, bias, post_scale, post_shift, \
                                        out, N, Ck, Cm, IH, IW, OH, OW, slope)
    if (CT == 4) C4_LAUNCH(4);
    else if (CT == 2) C4_LAUNCH(2);
    else C4_LAUNCH(1);
#undef C4_LAUNCH
}

template <int MODE, typename... Args>
static void c4_launch_if(bool f, Args... args) {
    if (f) c4_launch<MODE, true>(args...);
    else c4_launch<MODE, false>(args...);
}

// bytes of the fragments of `produced` x `summed` channels (all 16 taps of a pair, whichever the order)
static size_t c4_weight_bytes(int produced, int summed) { return (size_t)c4_tiles(produced) * summed * 512 * sizeof(float); }

static void c4_weights(const float *w, const float *scale, void *wfrag, int Cout, int Cin, int mode, void *stream) {
    const long long total = (long long)(c4_weight_bytes(mode == C4_FWD1 ? Cout : Cin, mode == C4_FWD1 ? Cin : Cout) / sizeof(float));
    hipLaunchKernelGGL(conv4x4_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, scale,
                       (float *)wfrag, Cout, Cin, mode, total);
}

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI: the encoder convolution of the motion U-Nets

SLR_EXPORT size_t slr_conv4x4s2_weight_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0) return 0;
    return c4_weight_bytes(Cout, Cin);
}

SLR_EXPORT int slr_conv4x4s2_f32_weights(const float *w, void *wfrag, int Cout, int Cin, void *stream) {
    SLR_CHECK_ARG(w && wfrag, "null pointer");
    SLR_CHECK_ARG(Cout > 0 && Cin > 0 && Cout < (1 << 16) && Cin < (1 << 16), "sizes");
    c4_weights(w, nullptr, wfrag, Cout, Cin, C4_FWD1, stream);
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
    const long long pixels = (long long)N * OH * OW;
    SLR_CHECK_ARG((pixels + 31) / 32 < (1LL << 31), "sizes");
    c4_launch_if<C4_ENC2>(leaky != 0, in, nullptr, (const float *)wfrag, bias, post_scale, post_shift, out, N, Cin, Cout, H, W, OH, OW, pixels,
                       slope, (hipStream_t)stream);
    SLR_CHECK_LAUNCH();
    return 0;
}

static bool e4_sizes_ok(int N, int Cin, int Cout, int H, int W) {
    return N > 0 && N < 65536 && Cin > 0 && Cin < (1 << 16) && Cout > 0 && Cout < (1 << 16) && H >= 2 && W >= 2 && H < (1 << 20) && W < (1 << 20) &&
           (long long)H * W < (1LL << 31) && (long long)N * H * W < (1LL << 31) && (long long)N * Cin * H * W < (1LL << 40);
}

SLR_EXPORT int slr_conv4x4s2_backward_data(const float *g, const float *xin, const void *wfrag, float *gin, int N, int Cin, int Cout, int H,
                                           int W, float slope, void *stream) {
    SLR_CHECK_ARG(g && wfrag && gin, "null pointer");
    SLR_CHECK_ARG(e4_sizes_ok(N, Cin, Cout, H, W), "sizes (H, W >= 2)");
    SLR_CHECK_ARG(!(((uintptr_t)g | (uintptr_t)xin | (uintptr_t)wfrag | (uintptr_t)gin) & 3), "4-byte aligned tensors");
    const int OH = (H - 2) / 2 + 1, OW = (W - 2) / 2 + 1;
    const float *none = nullptr;
    const long long pixels = (long long)N * ((H + 1) / 2) * ((W + 1) / 2);   // the even-even class, the largest
    c4_launch_if<C4_ENCB2>(xin != nullptr, g, xin, (const float *)wfrag, none, none, none, gin, N, Cout, Cin, OH, OW, H, W, pixels, slope,
                           (hipStream_t)stream);
    SLR_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ C ABI: the discriminator's convolution, forward and data gradient

SLR_EXPORT size_t slr_conv4x4_weight_bytes(int Cout, int Cin, int backward) {
    if (Cout <= 0 || Cin <= 0 || Cout >= (1 << 16) || Cin >= (1 << 16)) return 0;
    return backward ? c4_weight_bytes(Cin, Cout) : c4_weight_bytes(Cout, Cin);
}

SLR_EXPORT int slr_conv4x4_f32_weights(const float *w, const float *scale, void *wfrag, int Cout, int Cin, int stride, int backward,
                                       void *stream) {
    SLR_CHECK_ARG(w && wfrag, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(Cout > 0 && Cin > 0 && Cout < (1 << 16) && Cin < (1 << 16), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)w | (uintptr_t)scale | (uintptr_t)wfrag) & 3), "4-byte aligned tensors");
    c4_weights(w, scale, wfrag, Cout, Cin, !backward ? C4_FWD1 : stride == 1 ? C4_BWD1 : C4_BWD2, stream);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_conv4x4_forward(const float *in, const void *wfrag, const float *bias, float *out, int N, int Cin, int Cout, int H,
                                   int W, int stride, int leaky, float slope, void *stream) {
    SLR_CHECK_ARG(in && wfrag && out, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(c4_sizes_ok(N, Cin, Cout, H, W, stride), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)in | (uintptr_t)wfrag | (uintptr_t)bias | (uintptr_t)out) & 3), "4-byte aligned tensors");
    const int OH = c4_out(H, stride), OW = c4_out(W, stride);
    const long long pixels = (long long)N * OH * OW;
    hipStream_t st = (hipStream_t)stream;
    const float *wf = (const float *)wfrag, *none = nullptr;
    if (stride == 1) c4_launch_if<C4_FWD1>(leaky != 0, in, none, wf, bias, none, none, out, N, Cin, Cout, H, W, OH, OW, pixels, slope, st);
    else c4_launch_if<C4_FWD2>(leaky != 0, in, none, wf, bias, none, none, out, N, Cin, Cout, H, W, OH, OW, pixels, slope, st);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_conv4x4_backward_data(const float *g, const float *gate, const void *wfrag, float *gin, int N, int Cin, int Cout,
                                         int H, int W, int stride, float slope, void *stream) {
    SLR_CHECK_ARG(g && wfrag && gin, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(c4_sizes_ok(N, Cin, Cout, H, W, stride), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)g | (uintptr_t)gate | (uintptr_t)wfrag | (uintptr_t)gin) & 3), "4-byte aligned tensors");
    const int OH = c4_out(H, stride), OW = c4_out(W, stride);
    hipStream_t st = (hipStream_t)stream;
    const float *wf = (const float *)wfrag, *none = nullptr;
    // the largest pixel grid: the whole of gin at stride 1, its even-even class at stride 2
    const long long pixels = stride == 1 ? (long long)N * H * W : (long long)N * ((H + 1) / 2) * ((W + 1) / 2);
    if (stride == 1) c4_launch_if<C4_BWD1>(gate != nullptr, g, gate, wf, none, none, none, gin, N, Cout, Cin, OH, OW, H, W, pixels, slope, st);
    else c4_launch_if<C4_BWD2>(gate != nullptr, g, gate, wf, none, none, none, gin, N, Cout, Cin, OH, OW, H, W, pixels, slope, st);
    SLR_CHECK_LAUNCH();
    return 0;
}
