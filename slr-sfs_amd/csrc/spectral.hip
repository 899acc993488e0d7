// spectral.hip -- spectral normalisation of the generator's weights (ABI 20; the list-wide gradient: ABI 21): what torch.nn.utils.spectral_norm does for every 3x3, partial
// 3x3 and 1x1 convolution and every noise linear of the reference's generator under --norm_G sync:spectral_batch (models/layers/blocks.py:5-35,
// models/layers/normalization.py:6-16), over ANY number of weight matrices in one launch.  A plan in device memory (layout:
// include/slr_splat.h) lists the matrices; it is never passed as kernel arguments.  No atomics, nothing synchronises, every sum is
// accumulated in double in an order fixed by the matrix's own shape: the same bits from run to run and whatever else is in the list.
//   (a) spectral_sigma_kernel, one workgroup per matrix W [rows, cols] (weight_orig viewed as [Cout, Cin k k]); matrices of at least
//       SLR_SPECTRAL_SPLIT_ELEMENTS elements are first cut into bands of SLR_SPECTRAL_BAND_ROWS rows, a workgroup per band, in two
//       launches of their own (below), so that no single workgroup walks a large matrix alone:
//         training:  v <- W^T u / max(|W^T u|, eps);  u <- W v / max(|W v|, eps)   (one power iteration, torch's order; the max is
//         torch.clamp's: a NaN norm stays NaN, so a NaN in W makes all of its u, v and sigma NaN)
//         both:      inv_sigma = 1 / (u^T W v);  u and v are copied into the call's saved arrays for the backward.
//       Phase 1 (W^T u) walks the rows with the lanes along the columns, four adjacent columns per lane; row groups are added in group
//       order through LDS.  Phase 2 (W v) gives a row to a wave, the lanes along the columns again, and a butterfly over the wave.
//       16-byte loads where W is 16-byte aligned and cols % 4 == 0, four scalar loads of the same elements otherwise: the order of every
//       sum, and with it every bit, is the same on both paths.
//       Banded matrices: spectral_band_wtu_kernel writes each band's partial W^T u (rows in order) to the plan's scratch;
//       spectral_band_wv_kernel adds the partials in band order (every band's workgroup does, in the same order: the same v in each),
//       normalises, and computes W v for its own rows; spectral_sigma_kernel then only finishes u and sigma.  Whether a matrix is banded
//       and where the bands lie depends on (rows, cols) alone: the bits still do not depend on the list.
//   (b) the scaled weight preparation lives next to the fragment-order code it reuses (csrc/conv.hip).
//   (c) spectral_dot_kernel + spectral_grad_kernel: the gradient to weight_orig from the gradient dW at the effective weight
//       W_eff = weight_orig * inv_sigma:  (dW - <dW, W_eff> u v^T) * inv_sigma, u and v the constants of that forward.  Chunk partials of
//       <dW, weight_orig> in double, then every workgroup of the update adds the partials in chunk order.
//   (d) spectral_dot_multi_kernel + spectral_grad_multi_kernel (ABI 21): (c) for every tensor of a list in two launches, whatever the
//       list -- a workgroup per (tensor, chunk) of a plan in device memory, the chunk bodies of (c): bit-equal to (c) on each tensor.
#include <math.h>
#include <string.h>

#include "slr_reduce.hpp"

namespace slr {

constexpr int SPEC_THREADS = 512, SPEC_WAVES = SPEC_THREADS / 64;
constexpr int SPEC_MAXDIM = SLR_SPECTRAL_MAX_DIM;      // rows and cols of a matrix: what the LDS tables hold
constexpr int SPEC_CHUNK = SLR_SPECTRAL_GRAD_CHUNK;    // elements per workgroup of (c)
constexpr int SPEC_GRAD_THREADS = 256;
constexpr size_t SPEC_HEADER = 64;

constexpr int SPEC_BAND = SLR_SPECTRAL_BAND_ROWS, SPEC_BAND_THREADS = 256, SPEC_BAND_WAVES = SPEC_BAND_THREADS / 64;
constexpr long long SPEC_SPLIT = SLR_SPECTRAL_SPLIT_ELEMENTS;

struct SpecTensor {                                    // 64 bytes
    const float *w;
    float *u, *v;
    int rows, cols, slot, bands;                       // bands: 0 = one workgroup does it all
    long long u_off, v_off;                            // in elements, into the saved arrays
    long long scratch;                                 // banded: bytes from the plan's start to [bands][cols] + [rows] doubles
};
struct SpecWork {                                      // 8 bytes
    int tensor, band;
};
static_assert(sizeof(SpecTensor) == 64 && sizeof(SpecWork) == 8, "the documented plan layout");

__host__ __device__ inline int spec_bands(int rows, int cols) {
    return (long long)rows * cols >= SPEC_SPLIT && rows >= 2 * SPEC_BAND ? (rows + SPEC_BAND - 1) / SPEC_BAND : 0;
}
inline size_t spec_work_off(int n) { return (SPEC_HEADER + (size_t)n * sizeof(SpecTensor) + 15) & ~(size_t)15; }
inline size_t spec_scratch_off(int n, long long n_work) { return al256(spec_work_off(n) + (size_t)n_work * sizeof(SpecWork)); }
// work items and scratch bytes of the list, or -1 where it is not a legal one
static long long spec_count(int n, const int *rows, const int *cols, size_t *scratch) {
    if (n <= 0 || !rows || !cols) return -1;
    long long work = 0;
    size_t sc = 0;
    for (int t = 0; t < n; ++t) {
        if (rows[t] <= 0 || cols[t] <= 0 || rows[t] > SLR_SPECTRAL_MAX_DIM || cols[t] > SLR_SPECTRAL_MAX_DIM) return -1;
        const int b = spec_bands(rows[t], cols[t]);
        work += b;
        if (b) sc += al256(((size_t)b * cols[t] + rows[t]) * sizeof(double));
    }
    if (scratch) *scratch = sc;
    return work;
}
inline size_t spec_total(int n, long long n_work, size_t scratch) { return al256(spec_scratch_off(n, n_work) + scratch); }

__device__ __forceinline__ void load_quad(const float *__restrict__ row, int q, int cols, bool wide, float (&x)[4]) {
    if (wide) {
        const float4 f = reinterpret_cast<const float4 *>(row)[q];
        x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = 4 * q + j < cols ? row[4 * q + j] : 0.0f;
    }
}

// Sum of a[i]^2 (b = nullptr) or a[i] * b[i] over i < n, every thread gets it.  Fixed order: thread-strided, wave butterfly, waves in order.
__device__ __forceinline__ double spec_dot(const double *a, const float *b, int n, double (*red)[SPEC_WAVES], double *bcast) {
    double s[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += SPEC_THREADS) s[0] += a[i] * (b ? (double)b[i] : a[i]);
    __syncthreads();                                   // (red and bcast may still be read from the previous call)
    block_sum<1, SPEC_WAVES>(s, red);
    if (threadIdx.x == 0) *bcast = s[0];
    __syncthreads();
    return *bcast;
}

// Banded matrices, launch 1 (training): partial[band][c] = sum over the band's rows, in order, of W[r][c] u[r].  A thread owns column quads.
__global__ __launch_bounds__(SPEC_BAND_THREADS) void spectral_band_wtu_kernel(char *__restrict__ plan, const SpecTensor *__restrict__ tens,
                                                                              const SpecWork *__restrict__ work) {
    const SpecWork wk = work[blockIdx.x];
    const SpecTensor t = tens[wk.tensor];
    const int R = t.rows, C = t.cols, nq = (C + 3) >> 2;
    const bool wide = !((uintptr_t)t.w & 15) && !(C & 3);
    const int r0 = wk.band * SPEC_BAND, r1 = r0 + SPEC_BAND < R ? r0 + SPEC_BAND : R;
    double *partial = (double *)(plan + t.scratch) + (size_t)wk.band * C;
    for (int q = threadIdx.x; q < nq; q += SPEC_BAND_THREADS) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int r = r0; r < r1; ++r) {
            float x[4];
            load_quad(t.w + (size_t)r * C, q, C, wide, x);
            const double ur = (double)t.u[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (double)x[j] * ur;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < C) partial[4 * q + j] = acc[j];
    }
}

// Banded matrices, launch 2: v (training: the partials added in band order, normalised -- every band's workgroup computes the same v, band
// 0 stores it; eval: the stored v), then s[r] = sum_c W[r][c] v[c] for the band's rows into the scratch, a wave per row as below.
__global__ __launch_bounds__(SPEC_BAND_THREADS) void spectral_band_wv_kernel(char *__restrict__ plan, const SpecTensor *__restrict__ tens,
                                                                             const SpecWork *__restrict__ work, float *__restrict__ saved_v,
                                                                             int training, double eps) {
    __shared__ double tmp[SPEC_MAXDIM];
    __shared__ float vec[SPEC_MAXDIM];
    __shared__ double red[1][SPEC_BAND_WAVES];
    __shared__ double bcast;
    const SpecWork wk = work[blockIdx.x];
    const SpecTensor t = tens[wk.tensor];
    const int R = t.rows, C = t.cols, nq = (C + 3) >> 2;
    const bool wide = !((uintptr_t)t.w & 15) && !(C & 3);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *scratch = (double *)(plan + t.scratch);
    if (training) {
        double sq[1] = {0.0};
        for (int c = tid; c < C; c += SPEC_BAND_THREADS) {
            double s = 0.0;
            for (int b = 0; b < t.bands; ++b) s += scratch[(size_t)b * C + c];
            tmp[c] = s;
            sq[0] += s * s;
        }
        block_sum<1, SPEC_BAND_WAVES>(sq, red);
        if (tid == 0) bcast = sq[0];
        __syncthreads();
        const double nv = sqrt(bcast), dv = nv <= eps ? eps : nv;
        for (int c = tid; c < C; c += SPEC_BAND_THREADS) {
            const float vc = (float)(tmp[c] / dv);
            vec[c] = vc;
            if (wk.band == 0) {
                t.v[c] = vc;
                saved_v[t.v_off + c] = vc;
            }
        }
    } else {
        for (int c = tid; c < C; c += SPEC_BAND_THREADS) {
            const float vc = t.v[c];
            vec[c] = vc;
            if (wk.band == 0) saved_v[t.v_off + c] = vc;
        }
    }
    __syncthreads();
    double *s_out = scratch + (size_t)t.bands * C;
    const int rb = wk.band * SPEC_BAND, re = rb + SPEC_BAND < R ? rb + SPEC_BAND : R;
    for (int r0 = rb + wave; r0 < re; r0 += 2 * SPEC_BAND_WAVES) {
        const int r1 = r0 + SPEC_BAND_WAVES;
        double a0 = 0.0, a1 = 0.0;
        for (int q = lane; q < nq; q += 64) {
            float x0[4], x1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            load_quad(t.w + (size_t)r0 * C, q, C, wide, x0);
            if (r1 < re) load_quad(t.w + (size_t)r1 * C, q, C, wide, x1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double vc = 4 * q + j < C ? (double)vec[4 * q + j] : 0.0;
                a0 += (double)x0[j] * vc;
                a1 += (double)x1[j] * vc;
            }
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (lane == 0) {
            s_out[r0] = a0;
            if (r1 < re) s_out[r1] = a1;
        }
    }
}

__global__ __launch_bounds__(SPEC_THREADS) void spectral_sigma_kernel(const char *__restrict__ plan, const SpecTensor *__restrict__ tens, float *__restrict__ inv_sigma,
                                                                      float *__restrict__ saved_u, float *__restrict__ saved_v,
                                                                      int training, double eps) {
    __shared__ double tmp[SPEC_MAXDIM];                // W^T u, then W v
    __shared__ float vec[SPEC_MAXDIM];                 // v, then the stored u (eval)
    __shared__ double part[SPEC_THREADS][4];
    __shared__ double red[1][SPEC_WAVES];
    __shared__ double bcast;
    const SpecTensor t = tens[blockIdx.x];
    const int R = t.rows, C = t.cols, nq = (C + 3) >> 2;
    const bool wide = !((uintptr_t)t.w & 15) && !(C & 3);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    if (t.bands) {                                     // banded: v and W v are done (the two band kernels); only u and sigma are left
        const double *s_in = (const double *)(plan + t.scratch) + (size_t)t.bands * C;
        for (int r = tid; r < R; r += SPEC_THREADS) tmp[r] = s_in[r];
    } else if (training) {
        // phase 1: tmp[c] = sum_r W[r][c] u[r]
        int cw = 1;
        while (cw < nq && cw < 64) cw <<= 1;           // lanes along the column quads: a power of two up to a wave
        const int G = SPEC_THREADS / cw, ql = tid & (cw - 1), g = tid / cw;
        const int groups = G < R ? G : R;              // row groups that hold anything
        for (int q0 = 0; q0 < nq; q0 += cw) {
            const int q = q0 + ql;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            if (q < nq) {
#pragma unroll 4
                for (int r = g; r < R; r += G) {
                    float x[4];
                    load_quad(t.w + (size_t)r * C, q, C, wide, x);
                    const double ur = (double)t.u[r];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += (double)x[j] * ur;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) part[tid][j] = acc[j];
            __syncthreads();
            if (tid < 4 * cw) {                        // one column each: the groups in order
                const int cq = tid >> 2, j = tid & 3, c = 4 * (q0 + cq) + j;
                if (c < C) {
                    double s = 0.0;
                    for (int k = 0; k < groups; ++k) s += part[k * cw + cq][j];
                    tmp[c] = s;
                }
            }
            __syncthreads();
        }
        const double nv = sqrt(spec_dot(tmp, nullptr, C, red, &bcast));
        const double dv = nv <= eps ? eps : nv;
        for (int c = tid; c < C; c += SPEC_THREADS) {
            const float vc = (float)(tmp[c] / dv);
            vec[c] = vc;
            t.v[c] = vc;
            saved_v[t.v_off + c] = vc;
        }
    } else {
        for (int c = tid; c < C; c += SPEC_THREADS) {
            const float vc = t.v[c];
            vec[c] = vc;
            saved_v[t.v_off + c] = vc;
        }
    }
    __syncthreads();

    // phase 2: tmp[r] = sum_c W[r][c] v[c]; a wave per row, two rows in flight
    for (int r0 = t.bands ? R : wave; r0 < R; r0 += 2 * SPEC_WAVES) {
        const int r1 = r0 + SPEC_WAVES;
        double a0 = 0.0, a1 = 0.0;
        for (int q = lane; q < nq; q += 64) {
            float x0[4], x1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            load_quad(t.w + (size_t)r0 * C, q, C, wide, x0);
            if (r1 < R) load_quad(t.w + (size_t)r1 * C, q, C, wide, x1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double vc = 4 * q + j < C ? (double)vec[4 * q + j] : 0.0;
                a0 += (double)x0[j] * vc;
                a1 += (double)x1[j] * vc;
            }
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (lane == 0) {
            tmp[r0] = a0;
            if (r1 < R) tmp[r1] = a1;
        }
    }
    __syncthreads();

    double sigma;
    if (training) {
        const double nu = sqrt(spec_dot(tmp, nullptr, R, red, &bcast));
        const double du = nu <= eps ? eps : nu;
        for (int r = tid; r < R; r += SPEC_THREADS) {
            const float ur = (float)(tmp[r] / du);
            vec[r] = ur;                               // (v is no longer needed)
            t.u[r] = ur;
            saved_u[t.u_off + r] = ur;
        }
    } else {
        for (int r = tid; r < R; r += SPEC_THREADS) {
            const float ur = t.u[r];
            vec[r] = ur;
            saved_u[t.u_off + r] = ur;
        }
    }
    __syncthreads();
    sigma = spec_dot(tmp, vec, R, red, &bcast);        // u^T (W v) with the u that is stored
    if (tid == 0) inv_sigma[t.slot] = (float)(1.0 / sigma);
}

// (c) the chunk bodies, shared by the single-tensor and the list-wide kernels: one source, one order of every sum, the same bits.
// Chunk `chunk` of <dW, W>: thread-strided in double, wave butterfly, waves in order; thread 0 holds the sum.
__device__ __forceinline__ double spec_chunk_dot(const float *dw, const float *w, long long numel, int chunk, double (*red)[SPEC_GRAD_THREADS / 64]) {
    const long long start = (long long)chunk * SPEC_CHUNK;
    const int count = (int)(numel - start < SPEC_CHUNK ? numel - start : SPEC_CHUNK);
    double s[1] = {0.0};
    for (int i = threadIdx.x; i < count; i += SPEC_GRAD_THREADS) s[0] += (double)dw[start + i] * (double)w[start + i];
    block_sum<1, SPEC_GRAD_THREADS / 64>(s, red);
    return s[0];
}

// Chunk `chunk` of out = (dW - d u v^T) * inv_sigma with d = inv_sigma * sum_k partial[k], the partials added in chunk order.  out may be dw.
__device__ __forceinline__ void spec_chunk_grad(const float *dw, const float *u, const float *v, const float *inv_sigma, const double *partial,
                                                int n_chunks, float *out, long long numel, int cols, int chunk, double *dshared) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < n_chunks; ++k) s += partial[k];
        *dshared = s;
    }
    __syncthreads();
    const double is = (double)inv_sigma[0], d = *dshared * is;
    const long long start = (long long)chunk * SPEC_CHUNK;
    const int count = (int)(numel - start < SPEC_CHUNK ? numel - start : SPEC_CHUNK);
    for (int i = threadIdx.x; i < count; i += SPEC_GRAD_THREADS) {
        const long long e = start + i;
        const int r = (int)(e / cols), c = (int)(e - (long long)r * cols);
        out[e] = (float)(((double)dw[e] - d * (double)u[r] * (double)v[c]) * is);
    }
}

// (c) launch 1: partial[k] = sum over chunk k of dW[i] * W[i], in double
__global__ __launch_bounds__(SPEC_GRAD_THREADS) void spectral_dot_kernel(const float *__restrict__ dw, const float *__restrict__ w, long long numel,
                                                                         double *__restrict__ partial) {
    __shared__ double red[1][SPEC_GRAD_THREADS / 64];
    const double s = spec_chunk_dot(dw, w, numel, (int)blockIdx.x, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// (c) launch 2: out = (dW - d u v^T) * inv_sigma, every workgroup adding the partials in chunk order
__global__ __launch_bounds__(SPEC_GRAD_THREADS) void spectral_grad_kernel(const float *dw, const float *__restrict__ u,
                                                                          const float *__restrict__ v, const float *__restrict__ inv_sigma,
                                                                          const double *__restrict__ partial, int n_chunks, float *out,
                                                                          long long numel, int cols) {
    __shared__ double dshared;
    spec_chunk_grad(dw, u, v, inv_sigma, partial, n_chunks, out, numel, cols, (int)blockIdx.x, &dshared);
}

// (d) the same for every tensor of a list in two launches, a workgroup per (tensor, chunk) of the plan: the chunk bodies of (c) on the
// tensor's own chunks, its partials in its own doubles of the plan's scratch -- nothing of one tensor's result depends on the others.
struct SpecGradTensor {                                // 64 bytes
    const float *dw, *w;
    float *out;
    int rows, cols, slot, chunks;
    long long u_off, v_off;                            // in elements, into the saved arrays of the forward
    long long first;                                   // its first work item: its partials are doubles [first, first + chunks) of the scratch
};
static_assert(sizeof(SpecGradTensor) == 64, "the documented plan layout");

__global__ __launch_bounds__(SPEC_GRAD_THREADS) void spectral_dot_multi_kernel(const SpecGradTensor *__restrict__ tens, const SpecWork *__restrict__ work,
                                                                               double *__restrict__ scratch) {
    __shared__ double red[1][SPEC_GRAD_THREADS / 64];
    const SpecWork wk = work[blockIdx.x];
    const SpecGradTensor t = tens[wk.tensor];
    const double s = spec_chunk_dot(t.dw, t.w, (long long)t.rows * t.cols, wk.band, red);
    if (threadIdx.x == 0) scratch[t.first + wk.band] = s;
}

__global__ __launch_bounds__(SPEC_GRAD_THREADS) void spectral_grad_multi_kernel(const SpecGradTensor *__restrict__ tens, const SpecWork *__restrict__ work,
                                                                                const double *__restrict__ scratch, const float *__restrict__ inv_sigma,
                                                                                const float *__restrict__ saved_u, const float *__restrict__ saved_v) {
    __shared__ double dshared;
    const SpecWork wk = work[blockIdx.x];
    const SpecGradTensor t = tens[wk.tensor];
    spec_chunk_grad(t.dw, saved_u + t.u_off, saved_v + t.v_off, inv_sigma + t.slot, scratch + t.first, t.chunks, t.out, (long long)t.rows * t.cols,
                    t.cols, wk.band, &dshared);
}

static long long spec_chunks(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return -1;
    const long long numel = (long long)rows * cols;
    return numel < (1LL << 40) ? (numel + SPEC_CHUNK - 1) / SPEC_CHUNK : -1;
}

inline size_t spec_grad_work_off(int n) { return (SPEC_HEADER + (size_t)n * sizeof(SpecGradTensor) + 15) & ~(size_t)15; }
inline size_t spec_grad_scratch_off(int n, long long n_work) { return al256(spec_grad_work_off(n) + (size_t)n_work * sizeof(SpecWork)); }
inline size_t spec_grad_total(int n, long long n_work) { return spec_grad_scratch_off(n, n_work) + al256((size_t)n_work * sizeof(double)); }
// work items (chunks) of the list, or -1 where it is not a legal one
static long long spec_grad_count(int n, const int *rows, const int *cols) {
    if (n <= 0 || !rows || !cols) return -1;
    long long work = 0;
    for (int t = 0; t < n; ++t) {
        if (rows[t] <= 0 || cols[t] <= 0 || rows[t] > SLR_SPECTRAL_MAX_DIM || cols[t] > SLR_SPECTRAL_MAX_DIM) return -1;
        work += spec_chunks(rows[t], cols[t]);
    }
    return work;
}

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT size_t slr_spectral_plan_bytes(int n, const int *rows, const int *cols) {
    size_t scratch = 0;
    const long long work = spec_count(n, rows, cols, &scratch);
    return work < 0 ? 0 : spec_total(n, work, scratch);
}

SLR_EXPORT int slr_spectral_plan_fill(void *host_buf, size_t bytes, int n, const unsigned long long *w, const unsigned long long *u,
                                      const unsigned long long *v, const int *rows, const int *cols) {
    SLR_CHECK_ARG(n > 0, "n (at least one tensor)");
    SLR_CHECK_ARG(host_buf && w && u && v && rows && cols, "null pointer");
    size_t scratch = 0;
    const long long n_work = spec_count(n, rows, cols, &scratch);
    SLR_CHECK_ARG(n_work >= 0 && n_work < (1LL << 31), "rows, cols (1 .. SLR_SPECTRAL_MAX_DIM)");
    const size_t need = spec_total(n, n_work, scratch);
    SLR_CHECK_ARG(bytes >= need, "bytes (slr_spectral_plan_bytes(n, rows, cols) at least)");
    for (int t = 0; t < n; ++t) {
        SLR_CHECK_ARG(w[t] && u[t] && v[t], "null tensor pointer");
        SLR_CHECK_ARG(!((w[t] | u[t] | v[t]) & 3), "4-byte aligned tensors");
    }
    char *base = (char *)host_buf;
    memset(base, 0, spec_scratch_off(n, n_work));      // (the scratch behind it is written before it is read: left as it is)
    SpecTensor *tens = (SpecTensor *)(base + SPEC_HEADER);
    SpecWork *work = (SpecWork *)(base + spec_work_off(n));
    long long u_off = 0, v_off = 0, k = 0;
    size_t sc = spec_scratch_off(n, n_work);
    for (int t = 0; t < n; ++t) {
        const int b = spec_bands(rows[t], cols[t]);
        tens[t] = {(const float *)w[t], (float *)u[t], (float *)v[t], rows[t], cols[t], t, b, u_off, v_off, b ? (long long)sc : 0};
        for (int i = 0; i < b; ++i) work[k++] = {t, i};
        if (b) sc += al256(((size_t)b * cols[t] + rows[t]) * sizeof(double));
        u_off += rows[t];
        v_off += cols[t];
    }
    const unsigned int head32[4] = {SLR_SPECTRAL_PLAN_MAGIC, (unsigned)SPEC_MAXDIM, (unsigned)n, (unsigned)n_work};
    const unsigned long long head64[6] = {SPEC_HEADER, need, (unsigned long long)u_off, (unsigned long long)v_off, spec_work_off(n),
                                          spec_scratch_off(n, n_work)};
    memcpy(base, head32, sizeof head32);
    memcpy(base + 16, head64, sizeof head64);
    return 0;
}

SLR_EXPORT int slr_spectral_sigma(void *plan_dev, int n_tensors, int n_work, float *inv_sigma, float *saved_u, float *saved_v, int training,
                                  void *stream) {
    SLR_CHECK_ARG(plan_dev && inv_sigma && saved_u && saved_v, "null pointer");
    SLR_CHECK_ARG(n_tensors > 0, "n_tensors (at least one tensor)");
    SLR_CHECK_ARG(n_work >= 0, "n_work (what slr_spectral_plan_fill wrote into the plan's header)");
    SLR_CHECK_ARG(!((uintptr_t)plan_dev & 15) && !(((uintptr_t)inv_sigma | (uintptr_t)saved_u | (uintptr_t)saved_v) & 3),
                  "plan 16-byte, arrays 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)plan_dev;
    const SpecTensor *tens = (const SpecTensor *)(base + SPEC_HEADER);
    const SpecWork *work = (const SpecWork *)(base + spec_work_off(n_tensors));
    if (n_work > 0) {
        if (training) {
            hipLaunchKernelGGL(spectral_band_wtu_kernel, dim3(n_work), dim3(SPEC_BAND_THREADS), 0, st, base, tens, work);
            SLR_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(spectral_band_wv_kernel, dim3(n_work), dim3(SPEC_BAND_THREADS), 0, st, base, tens, work, saved_v, training ? 1 : 0,
                           1e-12);
        SLR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(spectral_sigma_kernel, dim3(n_tensors), dim3(SPEC_THREADS), 0, st, (const char *)base, tens, inv_sigma, saved_u, saved_v,
                       training ? 1 : 0, 1e-12);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_spectral_grad_ws_bytes(int rows, int cols) {
    const long long chunks = spec_chunks(rows, cols);
    return chunks < 0 ? 0 : al256((size_t)chunks * sizeof(double));
}

SLR_EXPORT int slr_spectral_weight_grad(const float *dw, const float *w, const float *u, const float *v, const float *inv_sigma, float *out,
                                        int rows, int cols, void *ws, size_t ws_bytes, void *stream) {
    SLR_CHECK_ARG(dw && w && u && v && inv_sigma && out, "null pointer");
    const long long chunks = spec_chunks(rows, cols);
    SLR_CHECK_ARG(chunks > 0 && chunks < (1LL << 31), "rows, cols");
    SLR_CHECK_ARG(!(((uintptr_t)dw | (uintptr_t)w | (uintptr_t)u | (uintptr_t)v | (uintptr_t)inv_sigma | (uintptr_t)out) & 3), "4-byte aligned tensors");
    if (!ws || ((uintptr_t)ws & 15) || ws_bytes < al256((size_t)chunks * sizeof(double))) {
        set_error("%s: workspace too small or misaligned (slr_spectral_grad_ws_bytes bytes, 16-byte aligned)", __func__);
        return SLR_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long numel = (long long)rows * cols;
    hipLaunchKernelGGL(spectral_dot_kernel, dim3((unsigned)chunks), dim3(SPEC_GRAD_THREADS), 0, st, dw, w, numel, (double *)ws);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(spectral_grad_kernel, dim3((unsigned)chunks), dim3(SPEC_GRAD_THREADS), 0, st, dw, u, v, inv_sigma, (const double *)ws,
                       (int)chunks, out, numel, cols);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT size_t slr_spectral_grad_plan_bytes(int n, const int *rows, const int *cols) {
    const long long work = spec_grad_count(n, rows, cols);
    return work < 0 || work >= (1LL << 31) ? 0 : spec_grad_total(n, work);
}

SLR_EXPORT int slr_spectral_grad_plan_fill(void *host_buf, size_t bytes, int n, const unsigned long long *dw, const unsigned long long *w,
                                           const unsigned long long *out, const int *rows, const int *cols, const long long *u_off,
                                           const long long *v_off, const int *slot) {
    SLR_CHECK_ARG(n > 0, "n (at least one tensor)");
    SLR_CHECK_ARG(host_buf && dw && w && out && rows && cols && u_off && v_off && slot, "null pointer");
    const long long n_work = spec_grad_count(n, rows, cols);
    SLR_CHECK_ARG(n_work >= 0 && n_work < (1LL << 31), "rows, cols (1 .. SLR_SPECTRAL_MAX_DIM)");
    const size_t need = spec_grad_total(n, n_work);
    SLR_CHECK_ARG(bytes >= need, "bytes (slr_spectral_grad_plan_bytes(n, rows, cols) at least)");
    for (int t = 0; t < n; ++t) {
        SLR_CHECK_ARG(dw[t] && w[t] && out[t], "null tensor pointer");
        SLR_CHECK_ARG(!((dw[t] | w[t] | out[t]) & 3), "4-byte aligned tensors");
        SLR_CHECK_ARG(u_off[t] >= 0 && v_off[t] >= 0 && slot[t] >= 0, "u_off, v_off, slot (not negative)");
    }
    char *base = (char *)host_buf;
    memset(base, 0, spec_grad_scratch_off(n, n_work));  // (the scratch behind it is written before it is read: left as it is)
    SpecGradTensor *tens = (SpecGradTensor *)(base + SPEC_HEADER);
    SpecWork *work = (SpecWork *)(base + spec_grad_work_off(n));
    long long k = 0;
    for (int t = 0; t < n; ++t) {
        const int chunks = (int)spec_chunks(rows[t], cols[t]);
        tens[t] = {(const float *)dw[t], (const float *)w[t], (float *)out[t], rows[t], cols[t], slot[t], chunks, u_off[t], v_off[t], k};
        for (int i = 0; i < chunks; ++i) work[k++] = {t, i};
    }
    const unsigned int head32[4] = {SLR_SPECTRAL_GRAD_PLAN_MAGIC, (unsigned)SPEC_CHUNK, (unsigned)n, (unsigned)n_work};
    const unsigned long long head64[4] = {SPEC_HEADER, need, spec_grad_work_off(n), spec_grad_scratch_off(n, n_work)};
    memcpy(base, head32, sizeof head32);
    memcpy(base + 16, head64, sizeof head64);
    return 0;
}

SLR_EXPORT int slr_spectral_weight_grad_multi(void *plan_dev, int n_tensors, int n_work, const float *inv_sigma, const float *saved_u,
                                              const float *saved_v, void *stream) {
    SLR_CHECK_ARG(plan_dev && inv_sigma && saved_u && saved_v, "null pointer");
    SLR_CHECK_ARG(n_tensors > 0, "n_tensors (at least one tensor)");
    SLR_CHECK_ARG(n_work >= n_tensors, "n_work (what slr_spectral_grad_plan_fill wrote into the plan's header)");
    SLR_CHECK_ARG(!((uintptr_t)plan_dev & 15) && !(((uintptr_t)inv_sigma | (uintptr_t)saved_u | (uintptr_t)saved_v) & 3),
                  "plan 16-byte, arrays 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)plan_dev;
    const SpecGradTensor *tens = (const SpecGradTensor *)(base + SPEC_HEADER);
    const SpecWork *work = (const SpecWork *)(base + spec_grad_work_off(n_tensors));
    double *scratch = (double *)(base + spec_grad_scratch_off(n_tensors, n_work));
    hipLaunchKernelGGL(spectral_dot_multi_kernel, dim3((unsigned)n_work), dim3(SPEC_GRAD_THREADS), 0, st, tens, work, scratch);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(spectral_grad_multi_kernel, dim3((unsigned)n_work), dim3(SPEC_GRAD_THREADS), 0, st, tens, work, (const double *)scratch,
                       inv_sigma, saved_u, saved_v);
    SLR_CHECK_LAUNCH();
    return 0;
}
