// disc.hip -- the kernels of the adversarial loss (ABI 18): the multiscale PatchGAN discriminator of the reference's trainer
// (models/networks/discriminators.py:78-139 NLayerDiscriminator, :142-207 MultiscaleDiscriminator; models/layers/normalization.py:95-130
// get_D_norm_layer "spectralinstance"), forward and backward.  Everything is NCHW fp32; nothing synchronises; no atomics -- every long sum
// runs in a fixed order in double (slr_reduce.hpp), so the same inputs give the same bits.
//   * Conv2d(Cin, Cout, 4, stride 1 or 2, padding 2) as an implicit GEMM on v_mfma_f32_32x32x2_f32 (fp32 operands, products and
//     accumulation: the arithmetic of the fp32 rung, as conv4x4s2_kernel of csrc/motion.hip), optional bias and LeakyReLU of the output;
//   * its gradient to the input as a gather on the same kernel body: a 4x4 / pad 1 correlation with the flipped weights at stride 1, the
//     2x2 taps of the pixel's parity class at stride 2 (K = 4 Cout) -- every element of gin is stored once;
//   * its weight gradient: M = Cout, N = 16 Cin, K = the output pixels, split into slabs whose partial sums a second launch adds in
//     double in slab order (the scheme of conv3x3_wgrad_kernel, csrc/conv_grad.hip), and the bias gradient in double;
//   * InstanceNorm2d(affine=False) + LeakyReLU forward (y, mean, rstd) and backward, one workgroup per (n, c) plane.
#include "slr_common.hpp"
#include "slr_reduce.hpp"

namespace slr {

typedef float dc_f16v __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------ the three convolution-shaped passes on one kernel body
// GEMM view: out[m][p] = sum_k a[m][k] * b[k][p]; m = the channel that is produced, k = (the channel that is summed, a tap), p = a pixel
// of the produced tensor.  Lane l of a v_mfma_f32_32x32x2_f32 holds A[l & 31][k0 + (l >> 5)] and B[k0 + (l >> 5)][l & 31].
//   DC_FWD1 / DC_FWD2  out = conv(in, w): 16 taps = 8 steps per summed channel ci; step s: ky = s >> 1, kx = 2 (s & 1) + (l >> 5); the tap
//                      reads in[S oy - 2 + ky][S ox - 2 + kx].
//   DC_BWD1            gin = the stride-1 adjoint: 8 steps per summed channel co; step s: ty = s >> 1, tx = 2 (s & 1) + (l >> 5) reads
//                      g[iy - 1 + ty][ix - 1 + tx] against w[co][ci][3 - ty][3 - tx].
//   DC_BWD2            gin = the stride-2 adjoint.  Pixel (iy, ix) = (2a + py, 2b + px) of parity class (py, px) = blockIdx.z gets the taps
//                      ky = py + 2 ty, kx = px + 2 tx (the ones for which (iy + 2 - ky) / 2 is exact): 2 steps per co; step s: ty = s,
//                      tx = l >> 5 reads g[a + 1 - ty][b + 1 - tx].  A tile's 32 pixels are of one class, so they share the A fragment.
// Weight fragments (one coalesced 256-byte load per MFMA), T = ceil(produced channels / 32), zero beyond the last channel:
//   forward   wf[((ct Cin + ci) 8 + s) 64 + l]                = w[32 ct + (l & 31)][ci][s >> 1][2 (s & 1) + (l >> 5)] * scale
//   DC_BWD1   wf[((ct Cout + co) 8 + s) 64 + l]               = w[co][32 ct + (l & 31)][3 - (s >> 1)][3 - 2 (s & 1) - (l >> 5)] * scale
//   DC_BWD2   wf[(((cls T + ct) Cout + co) 2 + s) 64 + l]     = w[co][32 ct + (l & 31)][py + 2 s][px + 2 (l >> 5)] * scale, cls = 2 py + px
// scale: a device scalar or none -- the 1 / sigma of spectral normalisation costs no pass of its own and no host synchronisation.
enum { DC_FWD1 = 0, DC_FWD2 = 1, DC_BWD1 = 2, DC_BWD2 = 3 };

__global__ __launch_bounds__(256) void conv4x4_weights_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                                              float *__restrict__ wf, int Cout, int Cin, int mode, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63), c = lane & 31, h = lane >> 5;
    long long rest = idx >> 6;
    int co, ci, ky, kx;
    bool ok;
    if (mode == DC_BWD2) {
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
        if (mode == DC_BWD1) {
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
// c = w, w + KW, ...) and wave 0 adds their accumulators from LDS in wave order (deterministic), as conv4x4s2_kernel does.
// `in` [N,Ck,IH,IW] is what is read, `out` [N,Cm,OH,OW] what is produced.  F: forward -- LeakyReLU of the output; backward -- the value
// read is g * (gate > 0 ? 1 : slope) with `gate` a tensor of g's shape (the LeakyReLU output of the layer whose gradient this is).
template <int MODE, int CT, bool F>
__global__ __launch_bounds__(1024) void conv4x4_kernel(const float *__restrict__ in, const float *__restrict__ gate,
                                                       const float *__restrict__ wf, const float *__restrict__ bias,
                                                       float *__restrict__ out, int N, int Ck, int Cm, int IH, int IW, int OH, int OW,
                                                       float slope) {
    constexpr bool FWD = MODE == DC_FWD1 || MODE == DC_FWD2;
    constexpr int NS = MODE == DC_BWD2 ? 2 : 8;
    extern __shared__ float red[];                       // [KW-1][CT*16][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, KW = blockDim.x >> 6;
    const int cls = MODE == DC_BWD2 ? blockIdx.z : 0, py = cls >> 1, px = cls & 1;
    // the pixel grid of this launch: the whole produced tensor, or its pixels of one parity class
    const int PH = MODE == DC_BWD2 ? (OH - py + 1) / 2 : OH, PW = MODE == DC_BWD2 ? (OW - px + 1) / 2 : OW;
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
        if (MODE == DC_BWD2) {
            iy = a + 1 - s;
            ix = b + 1 - h;
        } else {
            const int S = MODE == DC_FWD2 ? 2 : 1, PAD = MODE == DC_BWD1 ? 1 : 2;
            iy = S * a - PAD + (s >> 1);
            ix = S * b - PAD + 2 * (s & 1) + h;
        }
        ok[s] = pv & (iy >= 0) & (iy < IH) & (ix >= 0) & (ix < IW);
        off[s] = ok[s] ? iy * IW + ix : 0;
    }
    const size_t IHW = (size_t)IH * IW;
    const float *ip = in + (size_t)n * Ck * IHW;
    const float *gp = (!FWD && F) ? gate + (size_t)n * Ck * IHW : nullptr;
    const int ct0 = blockIdx.y * CT, T = gridDim.y * CT;
    dc_f16v acc[CT];
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
            if (!FWD && F) v *= gp[(size_t)c * IHW + off[s]] > 0.0f ? 1.0f : slope;
            bv[s] = ok[s] ? v : 0.0f;
        }
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const float *af = wf + (((size_t)cls * T + ct0 + t) * Ck + c) * (NS * 64) + lane;
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
    const int oy = MODE == DC_BWD2 ? 2 * a + py : a, ox = MODE == DC_BWD2 ? 2 * b + px : b;
    const size_t OHW = (size_t)OH * OW;
    float *op = out + (size_t)n * Cm * OHW + (size_t)oy * OW + ox;
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int cm = (ct0 + t) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;   // C/D map of the 32x32 MFMA
            if (cm < Cm) {
                float y = acc[t][q];
                if (FWD) {
                    if (bias) y += bias[cm];
                    if (F) y = y > 0.0f ? y : y * slope;
                }
                op[(size_t)cm * OHW] = y;
            }
        }
}

static int dc_tiles(int C) { return (C + 31) / 32; }
static int dc_out(int H, int stride) { return H / stride + 1; }     // (H + 2 * 2 - 4) / stride + 1
static bool dc_sizes_ok(int N, int Cin, int Cout, int H, int W, int stride) {
    if (!(N > 0 && N < 65536 && Cin > 0 && Cin < (1 << 16) && Cout > 0 && Cout < (1 << 16) && H > 0 && W > 0 && H < (1 << 20) && W < (1 << 20)))
        return false;
    if (stride != 1 && stride != 2) return false;
    const long long OH = dc_out(H, stride), OW = dc_out(W, stride);
    return (long long)H * W < (1LL << 31) && OH * OW < (1LL << 31) && (long long)N * H * W < (1LL << 31) && (long long)N * OH * OW < (1LL << 31) &&
           (long long)N * Cin * H * W < (1LL << 40) && (long long)N * Cout * OH * OW < (1LL << 40);
}

// `pixels`: of the largest pixel grid of the launch; ntile tiles of produced channels; Ck summed channels.
template <int MODE, bool F>
static void dc_launch(const float *in, const float *gate, const float *wf, const float *bias, float *out, int N, int Ck, int Cm, int IH,
                      int IW, int OH, int OW, long long pixels, float slope, hipStream_t st) {
    const int ntile = dc_tiles(Cm);
    const long long ptiles = (pixels + 31) / 32;
    // CT channel tiles per workgroup (the taps are loaded once for all of them); launches of a few tiles take one and split K over up to
    // 16 waves instead, so that the deep layers fill the chip -- the rule of slr_conv4x4s2_forward.  LDS: (KW - 1) * CT * 4 KiB <= 60 KiB.
    int CT = ntile % 4 == 0 ? 4 : ntile % 2 == 0 ? 2 : 1;
    const int classes = MODE == DC_BWD2 ? 4 : 1;
    if (ptiles * classes * (ntile / CT) < 512) CT = 1;
    const long long wgs = ptiles * classes * (ntile / CT);
    int KW = 1;
    while (KW < 16 / CT && wgs * KW < 2048 && 2 * KW <= Ck) KW *= 2;
    const dim3 grid((unsigned)ptiles, ntile / CT, classes);
    const size_t lds = (size_t)(KW - 1) * CT * 16 * 64 * sizeof(float);
#define DC_LAUNCH(T) hipLaunchKernelGGL((conv4x4_kernel<MODE, T, F>), grid, dim3(64 * KW), lds, st, in, gate, wf, bias, out, N, Ck, Cm, IH, \
                                        IW, OH, OW, slope)
    if (CT == 4) DC_LAUNCH(4);
    else if (CT == 2) DC_LAUNCH(2);
    else DC_LAUNCH(1);
#undef DC_LAUNCH
}

// ------------------------------------------------------------------ weight gradient
// grid (slabs, ci tiles of 32, co tiles of 32), four waves: wave ky owns the taps (ky, 0..3) of 32 co x 32 ci -- 4 accumulators.  A chunk
// is up to 32 consecutive output pixels of one output row; its G values and the four input rows they touch (S * 31 + 4 columns) are
// staged in LDS as [pixel][channel] (stride 33: conflict-free for both the staging stores and the operand reads).  A k step is a pixel
// pair; a chunk of cw pixels takes ceil(cw / 2) steps (an odd last pixel pairs with a staged zero).  Slab s takes the chunks
// [s T / S, (s + 1) T / S) of the T = N * OH * ceil(OW / 32) in row-major order and writes part[s][co][ci][ky][kx].
template <int S>
__global__ __launch_bounds__(256) void conv4x4_wgrad_kernel(const float *__restrict__ X, const float *__restrict__ G,
                                                            const float *__restrict__ gate, float *__restrict__ part, int N, int Cin,
                                                            int Cout, int H, int W, int OH, int OW, int chunks, int CX, float slope) {
    constexpr int XW = S * 31 + 4;
    __shared__ float gs[32 * 33];
    __shared__ float xs[4 * XW * 33];
    const int s = blockIdx.x, SS = gridDim.x, ci0 = blockIdx.y * 32, co0 = blockIdx.z * 32;
    const int first = (int)((long long)s * chunks / SS), last = (int)((long long)(s + 1) * chunks / SS);
    const int lane = threadIdx.x & 63, ky = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    dc_f16v acc[4];
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
            const int iy = S * oy + ry - 2, ix = S * ox0 + rx - 2;
            float v = 0.0f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W && ci0 + ci < Cin) v = X[(((size_t)n * Cin + ci0 + ci) * H + iy) * W + ix];
            xs[(ry * XW + rx) * 33 + ci] = v;
        }
        __syncthreads();
        const int npair = (cw + 1) >> 1;
        for (int j = 0; j < npair; ++j) {
            const int pix = 2 * j + h;
            const float av = gs[pix * 33 + c];
            const float *xb = xs + ((ky * XW + S * pix) * 33 + c);
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) acc[kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[kx * 33], acc[kx], 0, 0, 0);
        }
    }
    // D[row = co][column = ci]: the column on the lane, row (q & 3) + 8 (q >> 2) + 4 (lane >> 5) in register q
    const int ci = ci0 + c;
    if (ci < Cin) {
        const size_t total = (size_t)Cout * Cin * 16;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = co0 + (q & 3) + 8 * (q >> 2) + 4 * h;
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

static long long dcw_chunks(int N, int H, int W, int stride) { return (long long)N * dc_out(H, stride) * ((dc_out(W, stride) + 31) / 32); }
static int dcw_splits(int N, int Cin, int Cout, int H, int W, int stride, int splits) {
    const long long chunks = dcw_chunks(N, H, W, stride);
    long long S = splits > 0 ? splits : slr_wgrad_auto_splits(chunks, (long long)dc_tiles(Cin) * dc_tiles(Cout), (long long)Cout * Cin * 16 * 4);
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

SLR_EXPORT size_t slr_conv4x4_weight_bytes(int Cout, int Cin, int backward) {
    if (Cout <= 0 || Cin <= 0 || Cout >= (1 << 16) || Cin >= (1 << 16)) return 0;
    return backward ? (size_t)dc_tiles(Cin) * Cout * 512 * sizeof(float) : (size_t)dc_tiles(Cout) * Cin * 512 * sizeof(float);
}

SLR_EXPORT int slr_conv4x4_f32_weights(const float *w, const float *scale, void *wfrag, int Cout, int Cin, int stride, int backward,
                                       void *stream) {
    SLR_CHECK_ARG(w && wfrag, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(Cout > 0 && Cin > 0 && Cout < (1 << 16) && Cin < (1 << 16), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)w | (uintptr_t)scale | (uintptr_t)wfrag) & 3), "4-byte aligned tensors");
    const long long total = (long long)(slr_conv4x4_weight_bytes(Cout, Cin, backward) / sizeof(float));
    const int mode = !backward ? DC_FWD1 : stride == 1 ? DC_BWD1 : DC_BWD2;
    hipLaunchKernelGGL(conv4x4_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, scale,
                       (float *)wfrag, Cout, Cin, mode, total);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_conv4x4_forward(const float *in, const void *wfrag, const float *bias, float *out, int N, int Cin, int Cout, int H,
                                   int W, int stride, int leaky, float slope, void *stream) {
    SLR_CHECK_ARG(in && wfrag && out, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(dc_sizes_ok(N, Cin, Cout, H, W, stride), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)in | (uintptr_t)wfrag | (uintptr_t)bias | (uintptr_t)out) & 3), "4-byte aligned tensors");
    const int OH = dc_out(H, stride), OW = dc_out(W, stride);
    const long long pixels = (long long)N * OH * OW;
    hipStream_t st = (hipStream_t)stream;
    const float *wf = (const float *)wfrag;
#define DC_FWD(M) do { if (leaky) dc_launch<M, true>(in, nullptr, wf, bias, out, N, Cin, Cout, H, W, OH, OW, pixels, slope, st); \
                       else dc_launch<M, false>(in, nullptr, wf, bias, out, N, Cin, Cout, H, W, OH, OW, pixels, slope, st); } while (0)
    if (stride == 1) DC_FWD(DC_FWD1); else DC_FWD(DC_FWD2);
#undef DC_FWD
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_conv4x4_backward_data(const float *g, const float *gate, const void *wfrag, float *gin, int N, int Cin, int Cout,
                                         int H, int W, int stride, float slope, void *stream) {
    SLR_CHECK_ARG(g && wfrag && gin, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(dc_sizes_ok(N, Cin, Cout, H, W, stride), "sizes");
    SLR_CHECK_ARG(!(((uintptr_t)g | (uintptr_t)gate | (uintptr_t)wfrag | (uintptr_t)gin) & 3), "4-byte aligned tensors");
    const int OH = dc_out(H, stride), OW = dc_out(W, stride);
    hipStream_t st = (hipStream_t)stream;
    const float *wf = (const float *)wfrag;
    // the largest pixel grid: the whole of gin at stride 1, its even-even class at stride 2
    const long long pixels = stride == 1 ? (long long)N * H * W : (long long)N * ((H + 1) / 2) * ((W + 1) / 2);
#define DC_BWD(M) do { if (gate) dc_launch<M, true>(g, gate, wf, nullptr, gin, N, Cout, Cin, OH, OW, H, W, pixels, slope, st); \
                       else dc_launch<M, false>(g, nullptr, wf, nullptr, gin, N, Cout, Cin, OH, OW, H, W, pixels, slope, st); } while (0)
    if (stride == 1) DC_BWD(DC_BWD1); else DC_BWD(DC_BWD2);
#undef DC_BWD
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_conv4x4_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int stride, int splits) {
    if (!dc_sizes_ok(N, Cin, Cout, H, W, stride) || splits < 0) return 0;
    return al256((size_t)dcw_splits(N, Cin, Cout, H, W, stride, splits) * 16 * Cout * Cin * sizeof(float));
}

SLR_EXPORT int slr_conv4x4_weight_grad(const float *x, const float *g, const float *gate, float *dw, float *db, int N, int Cin, int Cout,
                                       int H, int W, int stride, float slope, int splits, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(x && g && dw, "null pointer");
    SLR_CHECK_ARG(stride == 1 || stride == 2, "stride (1 or 2)");
    SLR_CHECK_ARG(dc_sizes_ok(N, Cin, Cout, H, W, stride), "sizes");
    SLR_CHECK_ARG(splits >= 0, "splits (0 = chosen by the library)");
    SLR_CHECK_ARG(!(((uintptr_t)x | (uintptr_t)g | (uintptr_t)gate | (uintptr_t)dw | (uintptr_t)db) & 3), "4-byte aligned tensors");
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < slr_conv4x4_grad_ws_bytes(N, Cin, Cout, H, W, stride, splits)) {
        set_error("%s: ws: slr_conv4x4_grad_ws_bytes(N, Cin, Cout, H, W, stride, splits) bytes, 256-byte aligned", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int OH = dc_out(H, stride), OW = dc_out(W, stride), CX = (OW + 31) / 32;
    const int S = dcw_splits(N, Cin, Cout, H, W, stride, splits), chunks = (int)dcw_chunks(N, H, W, stride);
    float *part = (float *)ws;
    const dim3 grid(S, dc_tiles(Cin), dc_tiles(Cout));
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
