// blend.hip -- the splat half of the training step as ONE differentiable operator (models/animating_softmax_splating.py:587-692):
// both directions' features weighted by exp(clamp(Z - max Z)) * alpha | 1 - alpha, splatted, added, divided by the clamped normaliser --
// and its backward.  Per sample b and direction d in {f, p}: values V_d [C,H,W], logits Z_d [H,W], displacements D_d [2,H,W],
//   w_d = exp(clamp(Z_d - max Z_d, lo, hi)) * a_d            a_f = alpha[b], a_p = 1 - alpha[b];  Z_d absent: w_d = a_d
//   S_c(q) = sum_d sum_p sum_k beta_dpk(q) V_d,c(p) w_d(p)   n(q) = sum_d sum_p sum_k beta_dpk(q) w_d(p)     out_c = S_c / max(n, eps)
// Forward: per direction the tile kernels of splat_op.hip in their RAW form (splat_weighted_sum: the weight computed from the logits,
// the device maximum and alpha[n] where the softmax mode applies exp(metric); raw sums of the C planes + the raw normaliser plane),
// then blend_normalize_kernel adds the two directions and divides.  No weighted stack exists.  (the per-sample two-flow
// plan of the clip path, which would also drop the raw sums, is what is left.)
// Backward, with G = dL/dout, A_c = G_c / max(n, eps), R = -sum_c A_c out_c where n >= eps (else 0: the clamp's derivative):
//   blend_prepass_kernel   one read of G and out per destination -> (1 / max(n, eps), R), two planes per sample;
//   blend_gather_kernel    one work-item per SOURCE pixel, both directions and all channel groups in one launch: the corner weights once
//                          for all channels, G at the four corners scaled by the inverse normaliser on the fly (A is never written),
//                          dV_d,c = w_d g_c with g_c = sum_k beta_k A_c(q_k), and per channel group the partial sums of
//                          h = sum_c V_c g_c and of the displacement gradient's channel part;
//   blend_finish_kernel    per source pixel: the groups' partial sums in group order, the R terms, dZ_d (zero where the clamp bites),
//                          dD_d, and per workgroup a float64 partial sum of dZ_d for the maximum's correction;
//   blend_max_fix_kernel   one workgroup per direction: the partial sums in a fixed order, subtracted at the element that holds the
//                          maximum (the first one in memory order: ties are not split as torch splits them).
// No float atomics anywhere: every result is the same from run to run given the same forward result.
// A source pixel's footprint (`Foot`) and the corner sums of one channel (`corner_sum`, `disp_grad_add`) are those of grad.hip, in
// splat_gather.hpp; the gather passes the weights multiplied by the corners' inverse normaliser.
#include "splat_core.hpp"
#include "splat_gather.hpp"

namespace slr {

struct BlendDir {
    const float *v, *z, *d, *zmax;     // [N,C,H,W], [N,1,H,W] or null, [N,2,H,W], device scalar or null
    float *gv, *gz, *gd;               // gradients, each may be null
};

struct BlendArgs {
    BlendDir dir[2];
    const float *alpha;                // [N] on the device
    const float *out, *norm, *gout;    // [N,C,H,W], [N,1,H,W], [N,C,H,W]
    float *aux;                        // [N][2][HW]: 1 / max(n, eps), R
    float *part;                       // [groups][2N][3][HW]: h, gx, gy of a channel group
    double *bsum;                      // [2][N * blocks]: per-workgroup sums of dZ
    int *maxidx;                       // [2]: first element that holds the maximum
    float lo, hi, eps;
    int N, C, H, W, cper, groups;
};

// w_d at element zi of the logits; `pass`: the clamp lets the gradient through (torch.clamp: lo <= x <= hi)
__device__ __forceinline__ float blend_weight(const BlendDir &D, size_t zi, float a, float lo, float hi, bool &pass) {
    pass = false;
    if (!D.z) return a;
    float zn = D.z[zi] - (D.zmax ? D.zmax[0] : 0.0f);
    pass = (zn >= lo) & (zn <= hi);
    zn = fminf(fmaxf(zn, lo), hi);
    return expf(zn) * a;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// out = (S_f + S_p) / max(n_f + n_p, eps), norm = n_f + n_p (one reciprocal per pixel, like the fused kernels: splat_core.hpp)
__global__ __launch_bounds__(256) void blend_normalize_kernel(const float *__restrict__ sf, const float *__restrict__ sp,
                                                              const float *__restrict__ nf, const float *__restrict__ np,
                                                              float *__restrict__ out, float *__restrict__ norm, float eps, int C, int HW) {
    const int n = blockIdx.x / ((HW + 255) / 256);
    const int i = (blockIdx.x - n * ((HW + 255) / 256)) * 256 + threadIdx.x;
    if (i >= HW) return;
    const float *a = sf + (size_t)n * C * HW + i, *b = sp + (size_t)n * C * HW + i;
    float *o = out + (size_t)n * C * HW + i;
    const float nrm = nf[(size_t)n * HW + i] + np[(size_t)n * HW + i];
    norm[(size_t)n * HW + i] = nrm;
    const float inv = 1.0f / fmaxf(nrm, eps);
    int c = 0;
    for (; c + 4 <= C; c += 4) {
        float x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { x[u] = a[(size_t)(c + u) * HW]; y[u] = b[(size_t)(c + u) * HW]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) o[(size_t)(c + u) * HW] = (x[u] + y[u]) * inv;
    }
    for (; c < C; ++c) o[(size_t)c * HW] = (a[(size_t)c * HW] + b[(size_t)c * HW]) * inv;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void blend_prepass_kernel(BlendArgs a) {
    const int HW = a.H * a.W, C = a.C;
    const int n = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 2) a.maxidx[threadIdx.x] = 0x7fffffff;
    if (i >= HW) return;
    const float *g = a.gout + (size_t)n * C * HW + i, *o = a.out + (size_t)n * C * HW + i;
    const float nrm = a.norm[(size_t)n * HW + i];
    const float inv = 1.0f / fmaxf(nrm, a.eps);
    float s = 0.0f;
    int c = 0;
    for (; c + 4 <= C; c += 4) {
        float x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { x[u] = g[(size_t)(c + u) * HW]; y[u] = o[(size_t)(c + u) * HW]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) s += x[u] * y[u];
    }
    for (; c < C; ++c) s += g[(size_t)c * HW] * o[(size_t)c * HW];
    float *ax = a.aux + (size_t)n * 2 * HW + i;
    ax[0] = inv;
    ax[HW] = nrm >= a.eps ? -(s * inv) : 0.0f;
}

// GV: some direction wants dV; GH: some direction wants dZ or dD (the partial sums).  grid (HW / 256, 2N, groups).
template <bool GV, bool GH>
__global__ __launch_bounds__(256) void blend_gather_kernel(BlendArgs a) {
    constexpr int U = SLR_BLEND_U;
    const int H = a.H, W = a.W, HW = H * W;
    const int n2 = blockIdx.y, second = n2 >= a.N, n = n2 - (second ? a.N : 0);
    const BlendDir D = a.dir[second];
    const bool want_v = GV && D.gv, want_h = GH && (D.gz || D.gd);
    if (!want_v && !want_h) return;                               // (workgroup-uniform)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const int gz = blockIdx.z, cb = gz * a.cper, C = min(a.cper, a.C - cb);
    const int y = i / W, x = i - y * W;
    const float *f = D.d + (size_t)n * 2 * HW;
    const Foot t(f[i], f[HW + i], x, y, i, H, W);
    // A_c(q_k) = G_c(q_k) * inv(q_k): the inverse normaliser joins the corner's weight and its derivatives once
    const float *ax = a.aux + (size_t)n * 2 * HW;
    float bw[4], bdx[4], bdy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float iv = ax[t.o[k]];
        bw[k] = t.w[k] * iv; bdx[k] = t.dx[k] * iv; bdy[k] = t.dy[k] * iv;
    }
    float w = 0.0f;
    if (want_v) {
        bool pass;
        const float al = a.alpha[n];
        w = blend_weight(D, (size_t)n * HW + i, second ? 1.0f - al : al, a.lo, a.hi, pass);
    }
    const size_t pbase = ((size_t)n * a.C + cb) * HW;
    const float *gp = a.gout + pbase, *vp = D.v + pbase + i;
    float *op = want_v ? D.gv + pbase + i : nullptr;
    float h = 0.0f, gx = 0.0f, gy = 0.0f;
    // U channels per pass, all their loads issued before the first use; channels past C in the last pass re-read channel C - 1
    for (int ch = 0; ch < C; ch += U) {
        float g4[U][4], v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t po = (size_t)min(ch + u, C - 1) * HW;
#pragma unroll
            for (int q = 0; q < 4; ++q) g4[u][q] = gp[po + t.o[q]];
            if (GH) v[u] = vp[po];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ch + u >= C) continue;
            const float g = corner_sum(t.k, g4[u], bw);
            if (GV && want_v) op[(size_t)(ch + u) * HW] = t.ok ? w * g : 0.0f;
            if (GH) {
                h += v[u] * g;
                disp_grad_add(gx, gy, t.k, v[u], g4[u], bdx, bdy);
            }
        }
    }
    if (GH && want_h) {
        float *pp = a.part + ((size_t)gz * 2 * a.N + n2) * 3 * HW + i;
        pp[0] = h; pp[HW] = gx; pp[2 * (size_t)HW] = gy;
    }
}

// grid (HW / 256, 2N)
__global__ __launch_bounds__(256) void blend_finish_kernel(BlendArgs a) {
    __shared__ double red[4];
    const int H = a.H, W = a.W, HW = H * W;
    const int n2 = blockIdx.y, second = n2 >= a.N, n = n2 - (second ? a.N : 0);
    const BlendDir D = a.dir[second];
    if (!D.gz && !D.gd) return;                                   // (workgroup-uniform)
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    const bool live = i0 < HW;
    const int i = live ? i0 : 0;
    float h = 0.0f, gx = 0.0f, gy = 0.0f;
    for (int g = 0; g < a.groups; ++g) {                          // the groups' sums, in group order
        const float *pp = a.part + ((size_t)g * 2 * a.N + n2) * 3 * HW + i;
        h += pp[0]; gx += pp[HW]; gy += pp[2 * (size_t)HW];
    }
    const int y = i / W, x = i - y * W;
    const float *f = D.d + (size_t)n * 2 * HW;
    const Foot t(f[i], f[HW + i], x, y, i, H, W);
    const float *rp = a.aux + (size_t)n * 2 * HW + HW;
    float rv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rv[k] = rp[t.o[k]];
    const float r = corner_sum(t.k, rv, t.w), rx = corner_sum(t.k, rv, t.dx), ry = corner_sum(t.k, rv, t.dy);
    bool pass;
    const float al = a.alpha[n];
    const size_t zi = (size_t)n * HW + i;
    const float w = blend_weight(D, zi, second ? 1.0f - al : al, a.lo, a.hi, pass);
    if (D.gd && live) {
        float *gd = D.gd + (size_t)n * 2 * HW + i;
        gd[0] = t.ok ? w * (gx + rx) : 0.0f;
        gd[HW] = t.ok ? w * (gy + ry) : 0.0f;
    }
    if (D.gz) {                                                   // (uniform; D.z is there: checked on the host)
        const float gzn = (live & t.ok & pass) ? (h + r) * w : 0.0f;
        if (live) D.gz[zi] = gzn;
        if (D.zmax) {
            // the maximum's correction: this workgroup's sum in float64, lanes then waves in a fixed order
            double s = (double)gzn;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
            __syncthreads();
            if (threadIdx.x == 0) a.bsum[((size_t)second * a.N + n) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
            if (live && D.z[zi] == D.zmax[0]) atomicMin(&a.maxidx[second], (int)zi);      // (an integer minimum: the same from run to run)
        }
    }
}

// grid (2): dZ_d[argmax] -= sum of the workgroups' partial sums
__global__ __launch_bounds__(256) void blend_max_fix_kernel(BlendArgs a, int nblocks) {
    __shared__ double red[256];
    const int second = blockIdx.x;
    const BlendDir D = a.dir[second];
    if (!D.gz || !D.zmax) return;
    const double *b = a.bsum + (size_t)second * nblocks;
    double s = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 256) s += b[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int j = a.maxidx[second];
        if (j != 0x7fffffff) D.gz[j] = (float)((double)D.gz[j] - red[0]);
    }
}

// Channel groups of the gather (grid.z): one group is 2N * ceil(HW / 256) workgroups; as many groups as keep the launch within 4096
// workgroups, at most 4, at least 8 channels each, each a multiple of the 4 channels of a pass -- [2,64,256,256]: 4 groups (4096
// workgroups instead of 1024), 768x1280: one.  The N of the grids' second dimension (N or 2N) is bounded by blend_sizes_ok.
static int blend_groups(int N, int C, int H, int W) {
    const long long wgs = 2LL * N * (((long long)H * W + 255) / 256);
    long long g = 4096 / (wgs > 0 ? wgs : 1);
    g = g > 4 ? 4 : g;
    const int byc = C / 8;
    g = g > byc ? byc : g;
    return g < 1 ? 1 : (int)g;
}

struct BlendLayout { size_t stack, plane, aux, part, bsum, idx, fwd, bwd; int groups, cper, blocks; };
static BlendLayout blend_layout(int N, int C, int H, int W) {
    BlendLayout L;
    const size_t hw = (size_t)H * W;
    const ChannelSplit cs = split_channels(C, blend_groups(N, C, H, W), SLR_BLEND_U);
    L.groups = cs.groups; L.cper = cs.cper;
    L.blocks = (int)((hw + 255) / 256);
    L.stack = al256((size_t)N * C * hw * 4);                       // the raw sums of one direction ...
    L.plane = al256((size_t)N * hw * 4);                           // ... and its raw normaliser
    L.fwd = 2 * L.stack + 2 * L.plane;
    L.aux = 0;
    L.part = L.aux + al256((size_t)N * 2 * hw * 4);
    L.bsum = L.part + al256((size_t)L.groups * 2 * N * 3 * hw * 4);
    L.idx = L.bsum + al256((size_t)2 * N * L.blocks * 8);
    L.bwd = L.idx + 256;
    return L;
}

static bool blend_sizes_ok(int N, int C, int H, int W) {
    return N > 0 && N <= 32767 && C > 0 && H > 0 && W > 0 && H < (1 << 24) && (long long)N * H * W < (1LL << 29) && (long long)H * W < (1LL << 26);
}

int splat_weighted_sum(const float *values, const float *logits, const float *zmax, const float *alpha, int second, float lo, float hi,
                       const float *flow, float *sum, float *norm, int N, int C, int H, int W, void *ws, size_t ws_bytes, int ws_flags,
                       bool det, hipStream_t st);                    // splat_op.hip

}  // namespace slr

using namespace slr;

SLR_EXPORT size_t slr_splat_blend_ws_bytes(int N, int C, int H, int W) {
    if (!blend_sizes_ok(N, C, H, W)) return 0;
    const BlendLayout L = blend_layout(N, C, H, W);
    return L.fwd > L.bwd ? L.fwd : L.bwd;
}

// flags & SLR_BLEND_DETERMINISTIC: the DET forms of the tile kernels (splat_op.hip) -- blend_normalize_kernel is a fixed order anyway.
SLR_EXPORT int slr_splat_blend_forward_ex(const float *values_f, const float *logits_f, const float *disp_f, const float *values_p,
                                          const float *logits_p, const float *disp_p, const float *alpha, const float *zmax_f,
                                          const float *zmax_p, float clamp_lo, float clamp_hi, float eps, float *out, float *norm,
                                          int N, int C, int H, int W, void *splat_ws, size_t splat_ws_bytes, int ws_flags, int flags,
                                          void *scratch, size_t scratch_bytes, void *stream) {
    SLR_CHECK_ARG(!(flags & ~SLR_BLEND_DETERMINISTIC), "flags: unknown bits (SLR_BLEND_DETERMINISTIC)");
    const bool det = (flags & SLR_BLEND_DETERMINISTIC) != 0;
    SLR_CHECK_ARG(values_f && disp_f && values_p && disp_p && alpha && out && norm, "null pointer");
    SLR_CHECK_ARG(blend_sizes_ok(N, C, H, W), "sizes (N, C, H, W > 0, N < 2^15, N*H*W < 2^29, H*W < 2^26)");
    SLR_CHECK_ARG(clamp_lo <= clamp_hi && eps > 0.0f, "clamp range / eps");
    SLR_CHECK_ARG(!(ws_flags & SLR_WS_PREBINNED), "the two directions share the splat workspace: it cannot be prebinned");
    const BlendLayout L = blend_layout(N, C, H, W);
    SLR_CHECK_ARG(scratch && !((uintptr_t)scratch & 15) && scratch_bytes >= L.fwd, "scratch: slr_splat_blend_ws_bytes bytes, 16-byte aligned");
    SLR_CHECK_ARG(splat_ws && !((uintptr_t)splat_ws & 15) && splat_ws_bytes >= slr_splat_workspace_bytes(N, H, W),
                  "splat workspace: slr_splat_workspace_bytes(N, H, W) bytes, 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float *sum_f = (float *)scratch, *sum_p = (float *)((char *)scratch + L.stack);
    float *nrm_f = (float *)((char *)scratch + 2 * L.stack), *nrm_p = (float *)((char *)scratch + 2 * L.stack + L.plane);
    if (int e = splat_weighted_sum(values_f, logits_f, logits_f ? zmax_f : nullptr, alpha, 0, clamp_lo, clamp_hi, disp_f, sum_f, nrm_f, N, C, H, W,
                                   splat_ws, splat_ws_bytes, ws_flags, det, st)) return e;
    if (int e = splat_weighted_sum(values_p, logits_p, logits_p ? zmax_p : nullptr, alpha, 1, clamp_lo, clamp_hi, disp_p, sum_p, nrm_p, N, C, H, W,
                                   splat_ws, splat_ws_bytes, ws_flags, det, st)) return e;
    hipLaunchKernelGGL(blend_normalize_kernel, dim3((unsigned)(N * L.blocks)), dim3(256), 0, st, (const float *)sum_f, (const float *)sum_p,
                       (const float *)nrm_f, (const float *)nrm_p, out, norm, eps, C, H * W);
    SLR_CHECK_LAUNCH();
    return 0;
}

SLR_EXPORT int slr_splat_blend_forward(const float *values_f, const float *logits_f, const float *disp_f, const float *values_p,
                                       const float *logits_p, const float *disp_p, const float *alpha, const float *zmax_f,
                                       const float *zmax_p, float clamp_lo, float clamp_hi, float eps, float *out, float *norm,
                                       int N, int C, int H, int W, void *splat_ws, size_t splat_ws_bytes, int ws_flags,
                                       void *scratch, size_t scratch_bytes, void *stream) {
    return slr_splat_blend_forward_ex(values_f, logits_f, disp_f, values_p, logits_p, disp_p, alpha, zmax_f, zmax_p, clamp_lo, clamp_hi, eps, out, norm,
                                      N, C, H, W, splat_ws, splat_ws_bytes, ws_flags, 0, scratch, scratch_bytes, stream);
}

SLR_EXPORT int slr_splat_blend_backward(const float *values_f, const float *logits_f, const float *disp_f, const float *values_p,
                                        const float *logits_p, const float *disp_p, const float *alpha, const float *zmax_f,
                                        const float *zmax_p, float clamp_lo, float clamp_hi, float eps, const float *out,
                                        const float *norm, const float *grad_out, float *grad_values_f, float *grad_logits_f,
                                        float *grad_disp_f, float *grad_values_p, float *grad_logits_p, float *grad_disp_p,
                                        int N, int C, int H, int W, void *scratch, size_t scratch_bytes, void *stream) {
    SLR_CHECK_ARG(values_f && disp_f && values_p && disp_p && alpha && out && norm && grad_out, "null pointer");
    SLR_CHECK_ARG((logits_f || !grad_logits_f) && (logits_p || !grad_logits_p), "a gradient of logits that were not given");
    SLR_CHECK_ARG(blend_sizes_ok(N, C, H, W), "sizes (N, C, H, W > 0, N < 2^15, N*H*W < 2^29, H*W < 2^26)");
    SLR_CHECK_ARG(clamp_lo <= clamp_hi && eps > 0.0f, "clamp range / eps");
    const BlendLayout L = blend_layout(N, C, H, W);
    SLR_CHECK_ARG(scratch && !((uintptr_t)scratch & 15) && scratch_bytes >= L.bwd, "scratch: slr_splat_blend_ws_bytes bytes, 16-byte aligned");
    const bool gv = grad_values_f || grad_values_p, gh = grad_logits_f || grad_disp_f || grad_logits_p || grad_disp_p;
    if (!gv && !gh) return 0;
    hipStream_t st = (hipStream_t)stream;
    BlendArgs a = {};
    a.dir[0] = {values_f, logits_f, disp_f, logits_f ? zmax_f : nullptr, grad_values_f, grad_logits_f, grad_disp_f};
    a.dir[1] = {values_p, logits_p, disp_p, logits_p ? zmax_p : nullptr, grad_values_p, grad_logits_p, grad_disp_p};
    a.alpha = alpha; a.out = out; a.norm = norm; a.gout = grad_out;
    char *b = (char *)scratch;
    a.aux = (float *)(b + L.aux); a.part = (float *)(b + L.part); a.bsum = (double *)(b + L.bsum); a.maxidx = (int *)(b + L.idx);
    a.lo = clamp_lo; a.hi = clamp_hi; a.eps = eps;
    a.N = N; a.C = C; a.H = H; a.W = W; a.cper = L.cper; a.groups = L.groups;
    const dim3 g1(L.blocks, N), g2(L.blocks, 2 * N), g3(L.blocks, 2 * N, L.groups);
    hipLaunchKernelGGL(blend_prepass_kernel, g1, dim3(256), 0, st, a);
    dispatch_bools(gv, gh, [&](auto v, auto h) { hipLaunchKernelGGL((blend_gather_kernel<decltype(v)::value, decltype(h)::value>), g3, dim3(256), 0, st, a); });
    if (gh) {
        hipLaunchKernelGGL(blend_finish_kernel, g2, dim3(256), 0, st, a);
        if ((grad_logits_f && a.dir[0].zmax) || (grad_logits_p && a.dir[1].zmax))
            hipLaunchKernelGGL(blend_max_fix_kernel, dim3(2), dim3(256), 0, st, a, N * L.blocks);
    }
    SLR_CHECK_LAUNCH();
    return 0;
}
