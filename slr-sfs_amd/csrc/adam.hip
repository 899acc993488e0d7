// adam.hip -- the optimiser step (ABI 19): torch.optim.Adam without weight decay and amsgrad (what the reference's trainer runs,
// models/base_model.py:15-46) over ANY number of fp32 tensors in at most two launches.  A plan in device memory (layout: include/slr_splat.h)
// lists the tensors and cuts them into work items of at most ADAM_CHUNK elements; it is never passed as kernel arguments, so the number
// of tensors has no limit.  Nothing synchronises, no atomics: every element is read and written by exactly one thread, so the result does
// not depend on the grid or on how tensors are grouped into plans.
//   (a) adam_prepare_kernel, one workgroup: per tensor step += 1 and the two bias corrections, evaluated in double, into the plan's scratch
//       table.  This keeps pow out of the streaming kernel, and no workgroup of (b) advances a counter another one still has to read.
//   (b) adam_update_kernel: a capped grid striding over the work items; 16-byte accesses of all four streams where the four pointers of a
//       tensor are 16-byte aligned (a work item starts at a multiple of ADAM_CHUNK elements: it is aligned as its tensor is), scalar
//       accesses otherwise and for the last count % 4 elements.
// The arithmetic is torch's, fp32 with single roundings (the library is built with -ffp-contract=off):
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),  bc = 1 - beta^step.
#include <math.h>
#include <string.h>

#include "slr_common.hpp"

namespace slr {

constexpr int ADAM_CHUNK = SLR_ADAM_CHUNK;             // elements per work item (include/slr_splat.h); a multiple of 4 * ADAM_THREADS
constexpr int ADAM_THREADS = 256;
constexpr int ADAM_VEC_ITERS = ADAM_CHUNK / (4 * ADAM_THREADS);
constexpr int ADAM_MAX_GRID = 2048;                    // 256 CUs x 8 workgroups; the work items beyond are reached by the grid's stride
static_assert(ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "a full work item is a whole number of float4 per thread");

struct AdamTensor {                                    // 48 bytes
    float *p, *g, *m, *v, *step;
    long long numel;
};
struct AdamWork {                                      // 16 bytes
    int tensor, count;
    long long start;
};
static_assert(sizeof(AdamTensor) == 48 && sizeof(AdamWork) == 16, "the documented plan layout");

constexpr size_t ADAM_HEADER = 64;
inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t adam_work_off(int n) { return al16(ADAM_HEADER + (size_t)n * sizeof(AdamTensor)); }
inline size_t adam_scratch_off(int n, long long n_work) { return al16(adam_work_off(n) + (size_t)n_work * sizeof(AdamWork)); }
inline size_t adam_total(int n, long long n_work) { return al256(adam_scratch_off(n, n_work) + (size_t)n * 2 * sizeof(float)); }

// work items of the list, or -1 where the list is not a legal one
static long long adam_count_work(int n, const long long *numel) {
    if (n <= 0 || !numel) return -1;
    long long work = 0;
    for (int t = 0; t < n; ++t) {
        if (numel[t] < 0) return -1;
        work += (numel[t] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    }
    return work < (1LL << 31) ? work : -1;
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_prepare_kernel(const AdamTensor *__restrict__ tens, float2 *__restrict__ bc, int n,
                                                                    double beta1, double beta2) {
    for (int t = threadIdx.x; t < n; t += ADAM_THREADS) {
        float *sp = tens[t].step;
        const float s = *sp + 1.0f;
        *sp = s;
        bc[t] = make_float2((float)(1.0 - pow(beta1, (double)s)), (float)sqrt(1.0 - pow(beta2, (double)s)));
    }
}

struct AdamCoef {
    float b1, omb1, b2, omb2, eps, step_size, bc2_sqrt;
};

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamCoef &c) {
    m = c.b1 * m + c.omb1 * g;
    v = c.b2 * v + c.omb2 * g * g;
    p = p - c.step_size * m / (sqrtf(v) / c.bc2_sqrt + c.eps);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_update_kernel(const AdamTensor *__restrict__ tens, const AdamWork *__restrict__ work,
                                                                   const float2 *__restrict__ bc, int n_work,
                                                                   const float *__restrict__ lr_dev, float b1, float omb1, float b2,
                                                                   float omb2, float eps, int zero) {
    const float lr = *lr_dev;
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        const AdamWork wk = work[w];
        const AdamTensor t = tens[wk.tensor];
        const float2 corr = bc[wk.tensor];
        const AdamCoef c = {b1, omb1, b2, omb2, eps, lr / corr.x, corr.y};
        float *__restrict__ p = t.p + wk.start;
        float *__restrict__ g = t.g + wk.start;
        float *__restrict__ m = t.m + wk.start;
        float *__restrict__ v = t.v + wk.start;
        int done = 0;
        if (!(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15)) {
            const int n4 = wk.count >> 2;
            float4 *p4 = (float4 *)p, *g4 = (float4 *)g, *m4 = (float4 *)m, *v4 = (float4 *)v;
            float4 P[ADAM_VEC_ITERS], G[ADAM_VEC_ITERS], M[ADAM_VEC_ITERS], V[ADAM_VEC_ITERS];
#pragma unroll
            for (int k = 0; k < ADAM_VEC_ITERS; ++k) {     // every load of the work item first: 16 B x 4 streams x ADAM_VEC_ITERS in flight
                const int i = threadIdx.x + k * ADAM_THREADS;
                if (i < n4) {
                    P[k] = p4[i];
                    G[k] = g4[i];
                    M[k] = m4[i];
                    V[k] = v4[i];
                }
            }
#pragma unroll
            for (int k = 0; k < ADAM_VEC_ITERS; ++k) {
                const int i = threadIdx.x + k * ADAM_THREADS;
                if (i < n4) {
                    adam_element(P[k].x, G[k].x, M[k].x, V[k].x, c);
                    adam_element(P[k].y, G[k].y, M[k].y, V[k].y, c);
                    adam_element(P[k].z, G[k].z, M[k].z, V[k].z, c);
                    adam_element(P[k].w, G[k].w, M[k].w, V[k].w, c);
                    p4[i] = P[k];
                    m4[i] = M[k];
                    v4[i] = V[k];
                    if (zero) g4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
            done = n4 << 2;
        }
        for (int i = done + threadIdx.x; i < wk.count; i += ADAM_THREADS) {
            float pe = p[i], me = m[i], ve = v[i];
            adam_element(pe, g[i], me, ve, c);
            p[i] = pe;
            m[i] = me;
            v[i] = ve;
            if (zero) g[i] = 0.0f;
        }
    }
}

}  // namespace slr

using namespace slr;

// ------------------------------------------------------------------ C ABI

SLR_EXPORT size_t slr_adam_plan_bytes(int n, const long long *numel) {
    const long long work = adam_count_work(n, numel);
    return work < 0 ? 0 : adam_total(n, work);
}

SLR_EXPORT int slr_adam_plan_fill(void *host_buf, size_t bytes, int n, const unsigned long long *p, const unsigned long long *g,
                                  const unsigned long long *m, const unsigned long long *v, const unsigned long long *step,
                                  const long long *numel) {
    SLR_CHECK_ARG(n > 0, "n (at least one tensor)");
    SLR_CHECK_ARG(host_buf && p && g && m && v && step && numel, "null pointer");
    const long long n_work = adam_count_work(n, numel);
    SLR_CHECK_ARG(n_work >= 0, "numel (non-negative, fewer than 2^31 work items in all)");
    const size_t need = adam_total(n, n_work);
    SLR_CHECK_ARG(bytes >= need, "bytes (slr_adam_plan_bytes(n, numel) at least)");
    for (int t = 0; t < n; ++t) {
        SLR_CHECK_ARG(step[t], "null step pointer");
        SLR_CHECK_ARG(!numel[t] || (p[t] && g[t] && m[t] && v[t]), "null tensor pointer");
        SLR_CHECK_ARG(!((p[t] | g[t] | m[t] | v[t] | step[t]) & 3), "4-byte aligned tensors");
    }
    char *base = (char *)host_buf;
    memset(base, 0, need);
    const unsigned int head32[4] = {SLR_ADAM_PLAN_MAGIC, (unsigned)ADAM_CHUNK, (unsigned)n, (unsigned)n_work};
    const unsigned long long head64[4] = {ADAM_HEADER, adam_work_off(n), adam_scratch_off(n, n_work), need};
    memcpy(base, head32, sizeof head32);
    memcpy(base + 16, head64, sizeof head64);
    AdamTensor *tens = (AdamTensor *)(base + ADAM_HEADER);
    AdamWork *work = (AdamWork *)(base + adam_work_off(n));
    long long w = 0;
    for (int t = 0; t < n; ++t) {
        tens[t] = {(float *)p[t], (float *)g[t], (float *)m[t], (float *)v[t], (float *)step[t], numel[t]};
        for (long long s = 0; s < numel[t]; s += ADAM_CHUNK) {
            const long long left = numel[t] - s;
            work[w++] = {t, (int)(left < ADAM_CHUNK ? left : ADAM_CHUNK), s};
        }
    }
    return 0;
}

SLR_EXPORT int slr_adam_step(void *plan_dev, int n_tensors, int n_work, const float *lr_dev, const double *betas, float eps, int flags,
                             void *stream) {
    SLR_CHECK_ARG(plan_dev && lr_dev && betas, "null pointer (plan, lr or betas)");
    SLR_CHECK_ARG(n_tensors > 0, "n_tensors (at least one tensor)");
    SLR_CHECK_ARG(n_work >= 0, "n_work (what slr_adam_plan_fill wrote into the plan's header)");
    SLR_CHECK_ARG(betas[0] >= 0.0 && betas[0] < 1.0 && betas[1] >= 0.0 && betas[1] < 1.0, "betas (each in [0, 1))");
    SLR_CHECK_ARG(eps > 0.0f, "eps (> 0)");
    SLR_CHECK_ARG(!(flags & ~SLR_ADAM_ZERO_GRADS), "flags (unknown bits)");
    SLR_CHECK_ARG(!((uintptr_t)plan_dev & 15) && !((uintptr_t)lr_dev & 3), "plan 16-byte and lr 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)plan_dev;
    const AdamTensor *tens = (const AdamTensor *)(base + ADAM_HEADER);
    const AdamWork *work = (const AdamWork *)(base + adam_work_off(n_tensors));
    float2 *bc = (float2 *)(base + adam_scratch_off(n_tensors, n_work));
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, tens, bc, n_tensors, betas[0], betas[1]);
    SLR_CHECK_LAUNCH();
    if (n_work == 0) return 0;                           // (every tensor is empty)
    const int grid = n_work < ADAM_MAX_GRID ? n_work : ADAM_MAX_GRID;
    hipLaunchKernelGGL(adam_update_kernel, dim3(grid), dim3(ADAM_THREADS), 0, st, tens, work, (const float2 *)bc, n_work, lr_dev,
                       (float)betas[0], (float)(1.0 - betas[0]), (float)betas[1], (float)(1.0 - betas[1]), eps,
                       flags & SLR_ADAM_ZERO_GRADS);
    SLR_CHECK_LAUNCH();
    return 0;
}
