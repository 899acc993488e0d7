// euler.hip -- Euler integration of a static Eulerian motion field (gfx950).
//
// Replaces models/projection/euler_integration_manipulator.py:7-56: the reference runs a
// Python loop of ~15 tiny torch kernels per step (with a boolean-mask index_put that syncs
// the host), re-started from scratch for every frame.  Pixels are independent -- each step
// only GATHERS from the static field -- so one work-item integrates one pixel for all steps
// with its coordinate in registers.  The field (2 planes, 7.9 MB at 768x1280) stays in
// L2 / Infinity Cache; the kernel is latency-bound on the dependent gather chain, so it runs
// at full occupancy with 256-thread workgroups and lanes mapped to consecutive x (coalesced
// plane stores for the all-frames variant).
#include "slr_common.hpp"

namespace slr {

// One reference step (euler_integration_manipulator.py:37-46).  Bit-exact: fp32 adds only
// (sign is +-1, so sign*m is exact), rintf == torch.round (half to even).
__device__ __forceinline__ void euler_step(const float *__restrict__ mx, const float *__restrict__ my,
                                           int H, int W, float sign, float ox, float oy,
                                           float &px, float &py, bool &inv) {
    int ix = (int)rintf(px);
    int iy = (int)rintf(py);
    int g = iy * W + ix;
    float nx = px + sign * mx[g];
    float ny = py + sign * my[g];
    bool oob = (nx > (float)(W - 1)) | (nx < 0.0f) | (ny > (float)(H - 1)) | (ny < 0.0f) |
               !(nx == nx) | !(ny == ny);
    inv |= oob;
    px = inv ? ox : nx;
    py = inv ? oy : ny;
}

// grid.y = sample of a batch; steps (device, one count per sample) overrides nsteps when given: the batch form of
// EulerIntegration.forward (euler_integration_manipulator.py:58-71) is ONE launch with no step count read back by the host.
__global__ __launch_bounds__(256) void euler_kernel(const float *__restrict__ motion, int H, int W,
                                                    int nsteps, const long long *__restrict__ steps, float sign,
                                                    float *__restrict__ disp, float *__restrict__ visible) {
    const int HW = H * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const size_t b = blockIdx.y;
    motion += b * 2 * HW; disp += b * 2 * HW;
    if (visible) visible += b * HW;
    if (steps) nsteps = (int)min(max(steps[b], 0ll), (long long)0x7fffffff);      // (range(1, n + 1): no step for n <= 0)
    const float *mx = motion, *my = motion + HW;
    const int y = i / W, x = i - y * W;
    const float ox = (float)x, oy = (float)y;
    float px = ox, py = oy;
    bool inv = false;
    for (int s = 0; s < nsteps; ++s) {
        euler_step(mx, my, H, W, sign, ox, oy, px, py, inv);
        if (inv) break;                       // sticky: later steps cannot change the result
    }
    const float big = (float)(H > W ? H : W) + 1.0f;
    disp[i] = inv ? big : px - ox;
    disp[HW + i] = inv ? big : py - oy;
    if (visible) visible[i] = inv ? 0.0f : 1.0f;
}

// All frames t = 0 .. nmax of one direction in one pass; a work-item carries SLR_EULER_PPT pixels (256 apart: every store of a wave is
// 256 contiguous bytes).  The displacement maps are written once and read by later kernels only: nontemporal stores (round 5: 135 ->
// 115-127 us per direction at 768x1280, N = 60 = 480 MB written: ~4 TB/s, store-bound).  More independent gather chains per lane do
// not help -- 2 pixels per work-item 125-134 us, 4: 144-151 (the chain's latency is hidden already; fewer waves store less evenly).
#define SLR_EULER_PPT 1
__global__ __launch_bounds__(256) void euler_all_kernel(const float *__restrict__ motion, int H, int W,
                                                        int nmax, float sign,
                                                        float *__restrict__ disp_all,
                                                        float *__restrict__ vis_all) {
    constexpr int P = SLR_EULER_PPT;
    const int HW = H * W;
    const int i0 = blockIdx.x * (256 * P) + threadIdx.x;
    const float *mx = motion, *my = motion + HW;
    const float big = (float)(H > W ? H : W) + 1.0f;
    float ox[P], oy[P], px[P], py[P];
    bool inv[P], on[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int i = i0 + 256 * k;
        on[k] = i < HW;
        const int ii = on[k] ? i : 0, y = ii / W, x = ii - y * W;
        ox[k] = px[k] = (float)x; oy[k] = py[k] = (float)y;
        inv[k] = false;
    }
    for (int t = 0; t <= nmax; ++t) {
#pragma unroll
        for (int k = 0; k < P; ++k)
            if (t > 0 && !inv[k]) euler_step(mx, my, H, W, sign, ox[k], oy[k], px[k], py[k], inv[k]);
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (!on[k]) continue;
            const size_t o = (size_t)t * 2 * HW + i0 + 256 * k;
            __builtin_nontemporal_store(inv[k] ? big : px[k] - ox[k], disp_all + o);
            __builtin_nontemporal_store(inv[k] ? big : py[k] - oy[k], disp_all + o + HW);
            if (vis_all) vis_all[(size_t)t * HW + i0 + 256 * k] = inv[k] ? 0.0f : 1.0f;
        }
    }
}

// Backward of euler_kernel w.r.t. the motion field -- what torch autograd computes through the reference's loop
// (euler_integration_manipulator.py:36-55): the gather at the rounded coordinate (:37-38) is the only differentiable
// use of `motion`, so each step of a pixel's path receives the pixel's output gradient; a pixel that ever leaves the
// image has its coordinate and its displacement overwritten with constants (:45-46, :55) -> no gradient.
// One work-item per pixel: pass 1 finds out whether the path stays valid, pass 2 re-walks it and scatters (global fp32
// atomics: many paths cross the same cell; training-only path, HBM-atomic-bound, order as unspecified as torch's own
// index_put_(accumulate=True) backward).
__global__ __launch_bounds__(256) void euler_backward_kernel(const float *__restrict__ motion, int H, int W, int nsteps,
                                                             const long long *__restrict__ steps,
                                                             float sign, const float *__restrict__ gdisp,
                                                             float *__restrict__ gmotion) {
    const int HW = H * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const size_t b = blockIdx.y;                          // sample of a batch (see euler_kernel)
    motion += b * 2 * HW; gdisp += b * 2 * HW; gmotion += b * 2 * HW;
    if (steps) nsteps = (int)min(max(steps[b], 0ll), (long long)0x7fffffff);
    const float *mx = motion, *my = motion + HW;
    const int y = i / W, x = i - y * W;
    const float ox = (float)x, oy = (float)y;
    float px = ox, py = oy;
    bool inv = false;
    for (int s = 0; s < nsteps && !inv; ++s) euler_step(mx, my, H, W, sign, ox, oy, px, py, inv);
    if (inv) return;
    const float gx = sign * gdisp[i], gy = sign * gdisp[HW + i];
    px = ox; py = oy;
    for (int s = 0; s < nsteps; ++s) {
        const int g = (int)rintf(py) * W + (int)rintf(px);
        atomicAdd(&gmotion[g], gx);
        atomicAdd(&gmotion[HW + g], gy);
        euler_step(mx, my, H, W, sign, ox, oy, px, py, inv);
    }
}

__global__ __launch_bounds__(256) void zero_f32_kernel(float *__restrict__ p, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.0f;
}

}  // namespace slr

SLR_EXPORT int slr_euler_integrate(const float *motion, int H, int W, int nsteps, float sign,
                                   float *disp, float *visible, void *stream) {
    SLR_CHECK_ARG(motion && disp, "null pointer");
    SLR_CHECK_ARG(H > 0 && W > 0 && nsteps >= 0, "sizes");
    SLR_CHECK_ARG((long long)H * W < (1LL << 30), "H*W too large");
    SLR_CHECK_ARG(sign == 1.0f || sign == -1.0f, "sign must be +1 or -1");
    int blocks = (H * W + 255) / 256;
    hipLaunchKernelGGL(slr::euler_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       motion, H, W, nsteps, (const long long *)nullptr, sign, disp, visible);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_euler_integrate_batch(const float *motion, const long long *steps, int B, int H, int W, float sign,
                                         float *disp, float *visible, void *stream) {
    SLR_CHECK_ARG(motion && steps && disp, "null pointer");
    SLR_CHECK_ARG(B > 0 && B < 65536 && H > 0 && W > 0, "sizes");
    SLR_CHECK_ARG((long long)H * W < (1LL << 30), "H*W too large");
    SLR_CHECK_ARG(sign == 1.0f || sign == -1.0f, "sign must be +1 or -1");
    hipLaunchKernelGGL(slr::euler_kernel, dim3((H * W + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,
                       motion, H, W, 0, steps, sign, disp, visible);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_euler_integrate_all(const float *motion, int H, int W, int nmax, float sign,
                                       float *disp_all, float *vis_all, void *stream) {
    SLR_CHECK_ARG(motion && disp_all, "null pointer");
    SLR_CHECK_ARG(H > 0 && W > 0 && nmax >= 0, "sizes");
    SLR_CHECK_ARG((long long)H * W < (1LL << 30), "H*W too large");
    SLR_CHECK_ARG(sign == 1.0f || sign == -1.0f, "sign must be +1 or -1");
    int blocks = (H * W + 256 * SLR_EULER_PPT - 1) / (256 * SLR_EULER_PPT);
    hipLaunchKernelGGL(slr::euler_all_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       motion, H, W, nmax, sign, disp_all, vis_all);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_euler_backward(const float *motion, int H, int W, int nsteps, float sign, const float *grad_disp,
                                  float *grad_motion, void *stream) {
    SLR_CHECK_ARG(motion && grad_disp && grad_motion, "null pointer");
    SLR_CHECK_ARG(H > 0 && W > 0 && nsteps >= 0, "sizes");
    SLR_CHECK_ARG((long long)H * W < (1LL << 30), "H*W too large");
    SLR_CHECK_ARG(sign == 1.0f || sign == -1.0f, "sign must be +1 or -1");
    const int blocks = (H * W + 255) / 256;
    hipLaunchKernelGGL(slr::zero_f32_kernel, dim3(2 * blocks), dim3(256), 0, (hipStream_t)stream, grad_motion,
                       (size_t)2 * H * W);
    hipLaunchKernelGGL(slr::euler_backward_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, motion, H, W, nsteps,
                       (const long long *)nullptr, sign, grad_disp, grad_motion);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_euler_backward_batch(const float *motion, const long long *steps, int B, int H, int W, float sign,
                                        const float *grad_disp, float *grad_motion, void *stream) {
    SLR_CHECK_ARG(motion && steps && grad_disp && grad_motion, "null pointer");
    SLR_CHECK_ARG(B > 0 && B < 65536 && H > 0 && W > 0, "sizes");
    // (the zero kernel's grid, ceil(2 B H W / 256) workgroups, stays below 2^31)
    SLR_CHECK_ARG((long long)H * W < (1LL << 30) && (long long)B * H * W < (1LL << 38) - 128, "sizes too large");
    SLR_CHECK_ARG(sign == 1.0f || sign == -1.0f, "sign must be +1 or -1");
    const int blocks = (H * W + 255) / 256;
    const size_t n = (size_t)B * 2 * H * W;
    hipLaunchKernelGGL(slr::zero_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_motion, n);
    hipLaunchKernelGGL(slr::euler_backward_kernel, dim3(blocks, B), dim3(256), 0, (hipStream_t)stream, motion, H, W, 0,
                       steps, sign, grad_disp, grad_motion);
    SLR_CHECK_LAUNCH();
    return 0;
}

// ---- the two-direction operator of the training step (ABI 28) -----------------------------------------------------------------------
// forward: euler_kernel with the direction as grid.y (0: +motion for steps_f[b], 1: -motion for steps_p[b]) -- one launch where the
// training step had a negation and two; the same euler_step, so per sample and direction the bits of slr_euler_integrate_batch.
//
// backward: d(disp_f, disp_p)/d motion as ONE tensor whose bits do not depend on the order in which the contributions arrive.  The
// definition is euler_backward_kernel's; the sum is taken in 64-bit fixed point, whose addition commutes.
//   Per sample: M = the largest finite |g| over both displacement gradients, e = the exponent with 2^(e-1) <= M < 2^e (e = 0 when M = 0),
//   A = (n_f + n_p) H W >= the number of (path, step) visits any cell can receive, L = ceil(log2 A), F = min(60, 63 - L) fraction bits.
//   A visit's value is q = llrint(g 2^(F-e)), |q| <= 2^F - 1 (the clamp never binds while F >= 24: a float below 2^e is at most
//   2^e (1 - 2^-24)), so every partial sum is at most 2^L (2^F - 1) < 2^63 in magnitude: no overflow, whatever the order.
//   g 2^(F-e) is a double product by a power of two: exact.  Hence |q 2^(e-F) - g| <= 2^(e-F-1) per visit; a run of m consecutive steps in
//   one cell is added as m q, which is m visits' worth of that.
// RESOLUTION.  For a cell with K_c visits (both directions, every step counted) and exact sum s_c of its sign * g:
//       |out_c - s_c| <= Q_c + 2^-24 (|s_c| + Q_c),     Q_c = K_c 2^(e-F-1)
//   -- the quantisation, then ONE float rounding of the fixed-point sum (int64 -> float is correctly rounded, the scaling by 2^(e-F) is
//   exact above the denormal range; below it add 2^-150).  F < 24 (A > 2^39: more than 500 steps at 2^30 pixels) adds up to 2^(e-F) per
//   visit that rounds onto the clamp.  With A <= 2^30 (768 x 1280 at n <= 500), L <= 30 and F >= 33: the quantum 2^(e-F) is at most
//   M 2^-32, 32 bits below the sample's largest |g|.  Beyond that F shrinks by one bit per doubling of A and the bound above still holds.
// NON-FINITE g: left out of M, never quantised; the visit ORs its class (+Inf, -Inf, NaN of sign * g) into a bit plane with an integer
//   atomic, and finish writes what a float sum of that cell would be: NaN (canonical) for a NaN or for both infinities, else the infinity.
//   The classes absorb any finite sum, so the result is the same for every order -- and lands on the cells torch sends it to, only there.
// Integer atomics on vector memory only; no float atomic.
namespace slr {

constexpr int EP_PARTIALS = 256;                         // partial maxima per sample (one per workgroup of the scale launch)
constexpr size_t EP_HEAD = 256 + 4 * EP_PARTIALS;        // bytes per sample in front of the planes: {e, F, bits of M, 0}, pad, partials
constexpr unsigned EP_PINF = 1u, EP_NINF = 2u, EP_NAN = 4u;

struct EulerPairWs {
    unsigned char *head; long long *acc; unsigned *cls;
    __host__ __device__ EulerPairWs(void *ws, int B, int H, int W) {
        head = (unsigned char *)ws;
        acc = (long long *)(head + (size_t)B * EP_HEAD);
        cls = (unsigned *)(acc + (size_t)B * 2 * H * W);
    }
    __device__ int *info(size_t b) const { return (int *)(head + b * EP_HEAD); }
    __device__ unsigned *partials(size_t b) const { return (unsigned *)(head + b * EP_HEAD + 256); }
};

__device__ __forceinline__ int euler_pair_steps(const long long *steps, size_t b) {
    return (int)min(max(steps[b], 0ll), (long long)0x7fffffff);
}

// {e, F} of sample b from the partial maxima and the step counts; every work-item of the 256-wide workgroup must call it (the walk launch).
__device__ __forceinline__ void euler_pair_scale(const EulerPairWs &ws, size_t b, int nf, int np, int HW, int &e, int &F, unsigned &mbits) {
    __shared__ unsigned sh[EP_PARTIALS];
    sh[threadIdx.x] = ws.partials(b)[threadIdx.x];
    __syncthreads();
    for (int s = EP_PARTIALS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    mbits = sh[0];                                       // (bits of a non-negative finite float: ordered as unsigned)
    e = 0;
    if (mbits) (void)frexp((double)__uint_as_float(mbits), &e);
    const unsigned long long A = ((unsigned long long)nf + (unsigned long long)np) * (unsigned long long)HW;
    const int L = A <= 1 ? 0 : 64 - __clzll((long long)(A - 1));
    F = min(60, 63 - L);
}

__global__ __launch_bounds__(256) void euler_pair_kernel(const float *__restrict__ motion, int H, int W,
                                                         const long long *__restrict__ steps_f, const long long *__restrict__ steps_p,
                                                         float *__restrict__ disp_f, float *__restrict__ disp_p,
                                                         float *__restrict__ vis_f, float *__restrict__ vis_p) {
    const int HW = H * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const size_t b = blockIdx.z;
    const bool back = blockIdx.y != 0;
    const float sign = back ? -1.0f : 1.0f;
    const int nsteps = euler_pair_steps(back ? steps_p : steps_f, b);
    float *disp = (back ? disp_p : disp_f) + b * 2 * HW;
    float *visible = back ? vis_p : vis_f;
    const float *mx = motion + b * 2 * HW, *my = mx + HW;
    const int y = i / W, x = i - y * W;
    const float ox = (float)x, oy = (float)y;
    float px = ox, py = oy;
    bool inv = false;
    for (int s = 0; s < nsteps; ++s) {
        euler_step(mx, my, H, W, sign, ox, oy, px, py, inv);
        if (inv) break;
    }
    const float big = (float)(H > W ? H : W) + 1.0f;
    disp[i] = inv ? big : px - ox;
    disp[HW + i] = inv ? big : py - oy;
    if (visible) visible[b * HW + i] = inv ? 0.0f : 1.0f;
}

// launch 1 of 3: grid (EP_PARTIALS, B).  A workgroup zeroes its slice of the sample's planes and stores the largest finite |g| of the slice.
__global__ __launch_bounds__(256) void euler_pair_scale_kernel(const float *__restrict__ gdisp_f, const float *__restrict__ gdisp_p,
                                                               int B, int H, int W, void *__restrict__ workspace) {
    const int HW = H * W;
    const size_t b = blockIdx.y;
    const EulerPairWs ws(workspace, B, H, W);
    const int slice = (HW + EP_PARTIALS - 1) / EP_PARTIALS;
    const int lo = blockIdx.x * slice, hi = min(HW, lo + slice);
    long long *acc = ws.acc + b * 2 * HW;
    unsigned *cls = ws.cls + b * 2 * HW;
    const float *gf = gdisp_f + b * 2 * HW, *gp = gdisp_p + b * 2 * HW;
    unsigned m = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        acc[i] = 0; acc[HW + i] = 0; cls[i] = 0; cls[HW + i] = 0;
        const float v[4] = {gf[i], gf[HW + i], gp[i], gp[HW + i]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned a = __float_as_uint(v[k]) & 0x7fffffffu;
            if (a < 0x7f800000u) m = max(m, a);
        }
    }
    __shared__ unsigned sh[256];
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) ws.partials(b)[blockIdx.x] = sh[0];
}

__device__ __forceinline__ void euler_pair_add(long long *acc, long long v) {
    if (v) atomicAdd((unsigned long long *)acc, (unsigned long long)v);     // (two's complement: the signed sum; global_atomic_add_x2)
}

// launch 2 of 3: grid (ceil(HW / 256), 2, B), one work-item per (sample, direction, pixel).
__global__ __launch_bounds__(256) void euler_pair_walk_kernel(const float *__restrict__ motion, int B, int H, int W,
                                                              const long long *__restrict__ steps_f, const long long *__restrict__ steps_p,
                                                              const float *__restrict__ gdisp_f, const float *__restrict__ gdisp_p,
                                                              void *__restrict__ workspace) {
    const int HW = H * W;
    const size_t b = blockIdx.z;
    const EulerPairWs ws(workspace, B, H, W);
    const int nf = euler_pair_steps(steps_f, b), np = euler_pair_steps(steps_p, b);
    int e, F;
    unsigned mbits;
    euler_pair_scale(ws, b, nf, np, HW, e, F, mbits);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool back = blockIdx.y != 0;
    if (i == 0 && !back) {                                 // the sample's scale, for finish and for whoever states the bound
        int *info = ws.info(b);
        info[0] = e; info[1] = F; info[2] = (int)mbits; info[3] = 0;
    }
    if (i >= HW) return;
    const float sign = back ? -1.0f : 1.0f;
    const int nsteps = back ? np : nf;
    const float *gd = (back ? gdisp_p : gdisp_f) + b * 2 * HW;
    const float gx = sign * gd[i], gy = sign * gd[HW + i];
    if (nsteps == 0 || (gx == 0.0f && gy == 0.0f)) return;
    const float *mx = motion + b * 2 * HW, *my = mx + HW;
    const int y = i / W, x = i - y * W;
    const float ox = (float)x, oy = (float)y;
    float px = ox, py = oy;
    bool inv = false;
    for (int s = 0; s < nsteps && !inv; ++s) euler_step(mx, my, H, W, sign, ox, oy, px, py, inv);
    if (inv) return;
    // one value per channel: the quantised gradient, or the class of a non-finite one
    const long long qmax = (1ll << F) - 1;
    const double up = ldexp(1.0, F - e);
    const bool finx = fabsf(gx) < INFINITY, finy = fabsf(gy) < INFINITY;      // (false for a NaN)
    const long long qx = finx ? min(max(llrint((double)gx * up), -qmax), qmax) : 0;
    const long long qy = finy ? min(max(llrint((double)gy * up), -qmax), qmax) : 0;
    const unsigned cx = finx ? 0u : (gx != gx ? EP_NAN : (gx > 0.0f ? EP_PINF : EP_NINF));
    const unsigned cy = finy ? 0u : (gy != gy ? EP_NAN : (gy > 0.0f ? EP_PINF : EP_NINF));
    long long *acc = ws.acc + b * 2 * HW;
    unsigned *cls = ws.cls + b * 2 * HW;
    px = ox; py = oy;
    int cell = i, run = 0;                                // (step 0 gathers from the pixel's own cell)
    for (int s = 0; s < nsteps; ++s) {
        const int g = (int)rintf(py) * W + (int)rintf(px);
        if (g != cell) {
            euler_pair_add(acc + cell, run * qx);
            euler_pair_add(acc + HW + cell, run * qy);
            if (cx) atomicOr(cls + cell, cx);
            if (cy) atomicOr(cls + HW + cell, cy);
            cell = g; run = 0;
        }
        ++run;
        euler_step(mx, my, H, W, sign, ox, oy, px, py, inv);
    }
    euler_pair_add(acc + cell, run * qx);
    euler_pair_add(acc + HW + cell, run * qy);
    if (cx) atomicOr(cls + cell, cx);
    if (cy) atomicOr(cls + HW + cell, cy);
}

// launch 3 of 3: grid (ceil(2 HW / 256), B): every element of grad_motion is written once, with the {e, F} the walk launch left in the header.
__global__ __launch_bounds__(256) void euler_pair_finish_kernel(int B, int H, int W, void *__restrict__ workspace,
                                                                float *__restrict__ grad_motion) {
    const int HW = H * W;
    const size_t b = blockIdx.y;
    const EulerPairWs ws(workspace, B, H, W);
    const int e = ws.info(b)[0], F = ws.info(b)[1];
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;           // (2 H W may pass 2^31)
    if (k >= (size_t)2 * HW) return;
    const long long v = ws.acc[b * 2 * HW + k];
    const unsigned c = ws.cls[b * 2 * HW + k];
    float out = ldexpf((float)v, e - F);
    if (c) out = (c & EP_NAN) || (c & (EP_PINF | EP_NINF)) == (EP_PINF | EP_NINF) ? __uint_as_float(0x7fc00000u)
                                                                                 : (c & EP_PINF ? INFINITY : -INFINITY);
    grad_motion[b * 2 * HW + k] = out;
}

}  // namespace slr

static int euler_pair_check_sizes(const char *fn, int B, int H, int W) {
    SLR_CHECK_ARG_FN(fn, B > 0 && B < 65536 && H > 0 && W > 0, "sizes");
    SLR_CHECK_ARG_FN(fn, (long long)H * W < (1LL << 30), "H*W too large");
    return 0;
}

SLR_EXPORT size_t slr_euler_pair_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || B >= 65536 || H <= 0 || W <= 0 || (long long)H * W >= (1LL << 30)) return 0;
    return (size_t)B * (slr::EP_HEAD + (size_t)H * W * 24);
}

SLR_EXPORT int slr_euler_pair_forward(const float *motion, const long long *steps_f, const long long *steps_p, int B, int H, int W,
                                      float *disp_f, float *disp_p, float *vis_f, float *vis_p, void *stream) {
    SLR_CHECK_ARG(motion && steps_f && steps_p && disp_f && disp_p, "null pointer");
    if (int rc = euler_pair_check_sizes(__func__, B, H, W)) return rc;
    hipLaunchKernelGGL(slr::euler_pair_kernel, dim3((H * W + 255) / 256, 2, B), dim3(256), 0, (hipStream_t)stream, motion, H, W,
                       steps_f, steps_p, disp_f, disp_p, vis_f, vis_p);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_euler_pair_backward(const float *motion, const long long *steps_f, const long long *steps_p, int B, int H, int W,
                                       const float *gdisp_f, const float *gdisp_p, float *grad_motion, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    SLR_CHECK_ARG(motion && steps_f && steps_p && gdisp_f && gdisp_p && grad_motion && workspace, "null pointer");
    if (int rc = euler_pair_check_sizes(__func__, B, H, W)) return rc;
    if (workspace_bytes < slr_euler_pair_workspace_bytes(B, H, W) || ((uintptr_t)workspace & 7)) {
        slr::set_error("%s: workspace too small or misaligned (%zu bytes, %zu needed, 8-byte aligned)", __func__, workspace_bytes,
                       slr_euler_pair_workspace_bytes(B, H, W));
        return SLR_E_WORKSPACE;
    }
    const int HW = H * W;
    hipLaunchKernelGGL(slr::euler_pair_scale_kernel, dim3(slr::EP_PARTIALS, B), dim3(256), 0, (hipStream_t)stream, gdisp_f, gdisp_p, B, H,
                       W, workspace);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(slr::euler_pair_walk_kernel, dim3((HW + 255) / 256, 2, B), dim3(256), 0, (hipStream_t)stream, motion, B, H, W,
                       steps_f, steps_p, gdisp_f, gdisp_p, workspace);
    SLR_CHECK_LAUNCH();
    hipLaunchKernelGGL(slr::euler_pair_finish_kernel, dim3((unsigned)(((size_t)2 * HW + 255) / 256), B), dim3(256), 0,
                       (hipStream_t)stream, B, H, W, workspace, grad_motion);
    SLR_CHECK_LAUNCH();
    return 0;
}
