/*
 * slr_splat.h -- C ABI of libslrsplat.so: MI355X (gfx950) kernels for the SLR-SFS
 * frame-synthesis hot path (Euler-integrated feature warping + softmax splatting).
 *
 * The reference has no FFI for this path: models/softsplat.py hands raw data_ptr()s to
 * cupy-JIT-compiled CUDA kernels (softsplat.py:408-416) and euler_integration is a Python
 * loop of torch ops (models/projection/euler_integration_manipulator.py:36-55).  Each entry
 * point below names the reference code it replaces (file:line under the reference root).
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every tensor is fp32, NCHW, contiguous, resident in device (HBM) memory -- the same
 *     contract the reference asserts (softsplat.py:397-402);
 *   - `stream` is a hipStream_t (NULL = default stream) that belongs to the CURRENT device;
 *     all work is enqueued on it, nothing synchronises the host, nothing is allocated;
 *   - scratch memory is caller-owned: `ws` must hold slr_splat_workspace_bytes(N,H,W) bytes, 16-byte aligned (it depends on the
 *     flow's shape only, not on the planes splatted with it), and must not be shared by calls in flight on different streams;
 *   - sizes: H < 2^24, H*W < 2^26, N*H*W < 2^29; the plane count C is free -- a sample's plane stack of 2 GiB or more (the reference
 *     indexes up to 2^31 ELEMENTS per tensor, softsplat.py:163,408-416) is rendered by several launches over plane groups;
 *   - return value 0 = success; >0 = hipError_t; <0 = SLR_E_* argument error.
 *     slr_last_error() returns a thread-local description of the last failure.
 *   - a non-finite or |.| >= 2^30 target coordinate drops all four corners (reference: UB).
 */
#ifndef SLR_SPLAT_H
#define SLR_SPLAT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLR_ABI_VERSION 28

#define SLR_E_BADARG   (-1)   /* null pointer / non-positive size / unknown enum  */
#define SLR_E_WORKSPACE (-2)  /* workspace too small or misaligned                */

/* FunctionSoftsplat strType (softsplat.py:667) */
#define SLR_MODE_SUMMATION 0
#define SLR_MODE_AVERAGE   1
#define SLR_MODE_LINEAR    2
#define SLR_MODE_SOFTMAX   3

/* normaliser handling of slr_splat_normalize / slr_synth_group */
#define SLR_NORM_ZERO_TO_ONE 0   /* norm==0 -> 1      (softsplat.py:684)                       */
#define SLR_NORM_CLAMP_EPS   1   /* max(norm, eps)    (animating_softmax_splating.py:923)      */

int         slr_abi_version(void);
const char *slr_last_error(void);

/* Measurement hook: the NEXT splat call of this thread records hipEvent_t `ev_start` right
 * before and `ev_stop` right after its tile kernel (the dominant kernel; not the plan/combine
 * helpers) on the launch stream.  One-shot; NULLs disable.  Used by bench.py for the roofline. */
void slr_splat_time_next(void *ev_start, void *ev_stop);

/* ------------------------------------------------------------------ Euler integration */

/* euler_integration(motion, nsteps) for one sample.
 * Replaces models/projection/euler_integration_manipulator.py:7-56 (return_all_frames=False).
 *   motion  [2,H,W]  ch0 = x velocity, ch1 = y velocity (px/frame); multiplied by `sign`
 *                    (+1 / -1: the models call it with flow and -flow,
 *                    animating_softmax_splating.py:847-848; an exact sign flip)
 *   disp    [2,H,W]  out; invalid pixels = max(H,W)+1 in both channels (:55)
 *   visible [H,W]    out, 1.0/0.0 (:54); may be NULL
 * Bit-exact with the reference (fp32 adds, round-half-even gather index). */
int slr_euler_integrate(const float *motion, int H, int W, int nsteps, float sign,
                        float *disp, float *visible, void *stream);

/* All frames t = 0..nmax in ONE pass: disp_all[t] == euler_integration(sign*motion, t).
 * Replaces the per-frame re-integration of forward_flow (O(N^2) steps per clip,
 * animating_softmax_splating.py:847-848); the reference's own return_all_frames=True branch
 * is broken (euler_integration_manipulator.py:31,50).
 *   disp_all [nmax+1,2,H,W] out;  vis_all [nmax+1,H,W] out, may be NULL */
int slr_euler_integrate_all(const float *motion, int H, int W, int nmax, float sign,
                            float *disp_all, float *vis_all, void *stream);

/* Gradient of slr_euler_integrate w.r.t. the motion field: what torch autograd computes through the reference's
 * differentiable loop (euler_integration_manipulator.py:36-55; the training path feeds it the motion regressor's
 * output, animating_softmax_splating.py:515-580).  Each step of a still-valid pixel's path adds the pixel's
 * displacement gradient to the cell it gathered from (:37-38); pixels that left the image contribute nothing
 * (:45-46,55).
 *   grad_disp [2,H,W] in;  grad_motion [2,H,W] out (zeroed here, then accumulated with fp32 atomics) */
int slr_euler_backward(const float *motion, int H, int W, int nsteps, float sign, const float *grad_disp,
                       float *grad_motion, void *stream);

/* EulerIntegration(opt).forward(motion, destination_frame) -- the batch form the training step calls
 * (models/projection/euler_integration_manipulator.py:58-71, used at animating_softmax_splating.py:579-580): every sample
 * b integrated for its own steps[b] in ONE launch; the step counts stay on the device (the reference loops over b in
 * Python and reads destination_frame[b] on the host).
 *   motion [B,2,H,W];  steps [B] int64 ON THE DEVICE (what `index.long()` arithmetic yields; <= 0: no step, :36)
 *   disp [B,2,H,W] out;  visible [B,H,W] out, may be NULL.  Per sample bit-exact with slr_euler_integrate. */
int slr_euler_integrate_batch(const float *motion, const long long *steps, int B, int H, int W, float sign,
                              float *disp, float *visible, void *stream);

/* Gradient of slr_euler_integrate_batch w.r.t. the motion fields (per sample: slr_euler_backward).
 *   grad_disp [B,2,H,W] in;  grad_motion [B,2,H,W] out (zeroed here).  Sizes: B < 65536, H*W < 2^30, B*H*W < 2^38 - 128. */
int slr_euler_backward_batch(const float *motion, const long long *steps, int B, int H, int W, float sign,
                             const float *grad_disp, float *grad_motion, void *stream);

/* ABI 28.  Both integrations of the training step (animating_softmax_splating.py:579-580) as one operator.
 * Forward: ONE launch, the direction a grid dimension: disp_f = the integration of +motion for steps_f[b] steps, disp_p = that of
 * -motion for steps_p[b] steps; per sample and direction the bits of slr_euler_integrate_batch with sign = +1 / -1.
 *   motion [B,2,H,W];  steps_f, steps_p [B] int64 ON THE DEVICE;  disp_f, disp_p [B,2,H,W] out;  vis_f, vis_p [B,H,W] out, may be NULL. */
int slr_euler_pair_forward(const float *motion, const long long *steps_f, const long long *steps_p, int B, int H, int W,
                           float *disp_f, float *disp_p, float *vis_f, float *vis_p, void *stream);

/* Gradient of both displacements w.r.t. `motion` as one tensor: slr_euler_backward_batch(+1, gdisp_f) + slr_euler_backward_batch(-1,
 * gdisp_p) by definition, but summed in 64-bit fixed point with integer atomics, so grad_motion is the same bits whatever order the
 * contributions arrive in (run to run, alone or inside a batch).  Three launches: scale (zeroes the workspace, largest finite |g| per
 * sample), walk (one work-item per sample, direction and pixel; consecutive steps in one cell are one addition), finish (writes EVERY
 * element of grad_motion).  Per cell with K visits and exact sum s:  |out - s| <= Q + 2^-24 (|s| + Q),  Q = K 2^(e-F-1), where
 * 2^(e-1) <= largest finite |g| of the sample < 2^e and F = min(60, 63 - ceil(log2((steps_f[b] + steps_p[b]) H W))) (csrc/euler.hip has
 * the derivation).  A non-finite g goes to the cells of its pixel's path and nowhere else, as a canonical NaN or an infinity.
 *   workspace: slr_euler_pair_workspace_bytes(B, H, W) = B (1280 + 24 H W) bytes, 8-byte aligned, contents irrelevant on entry; on
 *   return sample b's first four ints (byte offset 1280 b) hold {e, F, bits of the largest finite |g|, 0}.
 * slr_euler_pair_workspace_bytes returns 0 for sizes the operator refuses (B outside 1..65535, H W >= 2^30). */
size_t slr_euler_pair_workspace_bytes(int B, int H, int W);
int slr_euler_pair_backward(const float *motion, const long long *steps_f, const long long *steps_p, int B, int H, int W,
                            const float *gdisp_f, const float *gdisp_p, float *grad_motion, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ------------------------------------------------------------------ splat: workspace, binning, front ends */

/* flags of the `prebinned` argument of the one-flow calls (0: a self-contained call on a workspace nothing is known about) */
#define SLR_WS_PREBINNED 1   /* `ws` was filled by slr_splat_bin / slr_splat_bin_pair with this flow */
#define SLR_WS_CLEAN     2   /* `ws` was zeroed by slr_splat_workspace_init and has only been used through this library since: the call
                                skips the kernel that zeroes the binning counters (the binning leaves them zero again) */

/* Bytes of scratch one flow field [N,2,H,W] needs: per-tile row-segment lists (256 records of 8 bytes per 8x64 output tile), work
 * plans, destination boxes, and for the scan front end's sink launch an entry array + slabs of partial sums -- 21 MB at 768x1280, 81 MB
 * on grids of up to 1024 tiles (where the scan front end runs by default: 16 MB of entries + 64 MB of slabs).  slr_splat_workspace_init
 * zeroes the counters of a fresh workspace (see SLR_WS_CLEAN). */
size_t slr_splat_workspace_bytes(int N, int H, int W);
int slr_splat_workspace_init(void *ws, size_t ws_bytes, int N, int H, int W, void *stream);

/* Sort `flow` [N,2,H,W] for splatting, inside `ws`: every 64-pixel row segment of the flow is appended to the few 8x64 OUTPUT
 * tiles its bilinear footprints touch (one 64-bit atomic per (segment, tile) = list slot + the tile's exact entry count), and the
 * work plan is written by the same launch (heavy tiles first; a tile of more than 1024 entries cut into ranges of its output
 * columns).  Depends on the flow only -- every tensor splatted with this flow reuses it (prebinned = SLR_WS_PREBINNED).
 * (No reference counterpart: the reference scatters with global atomics, softsplat.py:186-199; here each workgroup owns an output
 * tile -- or a range of its columns -- and gathers exactly the sources that land in it.) */
int slr_splat_bin(const float *flow, int N, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* slr_splat_bin for two flow fields of the same shape (the forward and the backward displacement map of a frame). */
int slr_splat_bin_pair(const float *flow_a, const float *flow_b, int N, int H, int W,
                       void *ws_a, void *ws_b, size_t ws_bytes, void *stream);

/* Front end of the self-contained one-flow calls below (slr_softsplat_forward, slr_softsplat_mode_forward, slr_maxsplat_forward,
 * slr_max_warp_norm without SLR_WS_PREBINNED).  Two exact front ends find an output tile's source pixels:
 *   rows : slr_splat_bin's binning + plan, then the tile kernel walks exactly the listed rows of the flow; pieces of heavy tiles
 *          run in parallel, each owning its output columns (no partial tiles, no combine).  3 launches (4 on a workspace that is not
 *          SLR_WS_CLEAN): rows + plan, tile kernel, and a normally empty pass-by-pass launch for pieces that still hold more than
 *          1024 entries;
 *   scan : one kernel writes the destination box of every 8x64 block of source pixels, then every output tile's workgroup lists the
 *          rows of the blocks whose box touches it and walks them with the same code (no plan: nothing to wait for on grids that fit
 *          the chip in one or two rounds).  3 launches: boxes, tile kernel, and a normally empty SINK launch for tiles of more than
 *          1024 entries (pile-ups of a contracting flow): their workgroups write the tile's entries out once, the sink launch
 *          renders them as tasks of exactly 1024 entries, up to 16 workgroups x 8 channel groups per tile at once, each into a slab
 *          of its own; the tile's last workgroup adds the slabs up in slot order (reproducible, no float atomics) and normalises.
 * A call takes `scan` when its grid has at most `max_tiles` output tiles (N * ceil(H/8) * ceil(W/64); default 1024, 0 = never,
 * INT_MAX = always) and `rows` above; slr_splat_set_front_end(1 | 2) forces scan | rows, anything else = automatic.  Process-wide;
 * both return the previous value (-1 = automatic).  Both are exact (floating-point summation order differs: results agree to
 * rounding, ~1e-6 relative). */
int slr_splat_set_scan_max_tiles(int max_tiles);
int slr_splat_set_front_end(int front_end);
/* Tuning of the scan front end (process-wide, 0 = the built-in choice by grid size): column pieces per output tile in the first launch
 * (1, 2, 4 or 8) x channel groups per piece; piece slots (default 33: the emergency slabs of pieces that find the slab pool empty; the sink
 * launch's task list takes min(32, slots) pieces per round) x channel groups (default 8) of the sink launch. */
void slr_splat_set_scan_shape(int pieces, int groups, int defer_wg, int defer_groups);

/* ------------------------------------------------------------------ splat: forward */

/* _FunctionSoftsplat.forward: summation splat.
 * Replaces kernel_Softsplat_updateOutput + its launcher, softsplat.py:157-202, 390-424.
 *   in [N,C,H,W], flow [N,2,H,W] -> out [N,C,H,W] (every element written; no pre-zeroing)
 * prebinned: 0 or SLR_WS_CLEAN = a self-contained call (front end: slr_splat_set_front_end / slr_splat_set_scan_max_tiles);
 * SLR_WS_PREBINNED: `ws` was filled by slr_splat_bin / slr_splat_bin_pair with this flow (one binning shared by several tensors
 * splatted with the same flow). */
int slr_softsplat_forward(const float *in, const float *flow, float *out,
                          int N, int C, int H, int W,
                          void *ws, size_t ws_bytes, int prebinned, void *stream);

/* FunctionSoftsplat(tenInput, tenFlow, tenMetric, strType) fused: weighting, splat and
 * normalisation in one pass.  Replaces softsplat.py:665-690.
 *   mode = SLR_MODE_*; metric [N,1,H,W] (ignored for SUMMATION/AVERAGE, may be NULL)
 *   out [N,C,H,W] = splat(in*m) / splat(m) with splat(m)==0 -> 1   (m = 1 | metric | exp(metric)) */
int slr_softsplat_mode_forward(const float *in, const float *metric, const float *flow, float *out,
                               int N, int C, int H, int W, int mode,
                               void *ws, size_t ws_bytes, int prebinned, void *stream);

/* Normalisation of a raw accumulation whose LAST channel is the normaliser:
 * accum [N,C+1,H,W] -> out [N,C,H,W].  Replaces softsplat.py:681-686 (ZERO_TO_ONE) and
 * animating_softmax_splating.py:923-924 (CLAMP_EPS, eps = 1e-8). */
int slr_splat_normalize(const float *accum, float *out, int N, int C, int H, int W,
                        int norm_mode, float eps, void *stream);

/* The frame-synthesis block of forward_flow for one group of planes sharing a weight plane:
 *   S   = splat(values*w*a, disp_f) + splat(values*w*(1-a), disp_p)
 *   nrm = splat(w*a, disp_f)        + splat(w*(1-a), disp_p)
 *   out = S / max(nrm, eps)                  (exact 0 where nothing lands)
 * with w = exp(wlogit - *wmax) if wmax != NULL else exp(wlogit) if exp_weights else wlogit.
 * Replaces animating_softmax_splating.py:849-862, 884-924 (values = start_fs, wlogit = Z,
 * a = 1 - t/N) and ..._2layers_alpha_seperate.py:950-1045 (second group: values = alpha_fluid,
 * wlogit = CompositeFluidAlpha_I0).  One sample (the models run bs = 1 at inference).
 *   values [C,H,W]; wlogit [H,W]; wmax: device pointer to 1 float or NULL
 *   disp_f, disp_p [2,H,W]; ws_f, ws_p: workspaces ALREADY binned with disp_f / disp_p (slr_splat_bin_pair); the call sorts copies
 *   of their lists, writes a two-flow plan into ws_f and runs the fused kernel of the clip path on that one frame
 *   out [C,H,W]; norm_out [H,W] or NULL (the clamped normaliser, for alpha_fluid_mask :1039) */
int slr_synth_group(const float *values, const float *wlogit, const float *wmax, int exp_weights,
                    const float *disp_f, const float *disp_p, float alpha,
                    float *out, float *norm_out, int C, int H, int W, float eps,
                    void *ws_f, void *ws_p, size_t ws_bytes, void *stream);

/* ---- clip plans: all frames of a clip binned and planned by one set of launches ----
 * forward_flow integrates and splats per frame (animating_softmax_splating.py:847-848,884-921); every displacement map of a clip
 * exists before its first frame (slr_euler_integrate_all), so the 2 x n maps of n frames are binned by ONE launch (row segments
 * per tile, exact column-octant histograms), their lists sorted by one, and one workgroup per frame writes the frame's work plan
 * (tiles of more than 1536 entries of the two directions together cut into column pieces): 4 launches per clip.
 * Frame i uses disp_f[idx_f[i]] and disp_p[idx_p[i]] (idx_*: DEVICE int arrays; for frame t of an N-frame clip idx_f = t,
 * idx_p = N - t).  At most 16384 frames per plan.
 * slr_clip_plan_totals: where the per-frame totals sit inside the plan buffer (stride_words uint32 per frame: [0] work items) --
 * read them back once per clip to pass exact grids to the synthesis calls (n_items; -1 or a NULL array = unknown: upper-bound grids,
 * surplus workgroups exit at once).
 * The synthesis calls WRITE into the plan (a frame's list of pieces that turned out to hold more than a segment, emptied again by the
 * same call): one synthesis call at a time per plan -- not from two streams at once -- and no frame twice in one batch. */
size_t slr_clip_plan_bytes(int nframes, int H, int W);
int slr_clip_plan_totals(int nframes, int H, int W, size_t *offset_bytes, int *stride_words);
int slr_clip_plan_build(const float *disp_f, const int *idx_f, const float *disp_p, const int *idx_p, int nframes,
                        int H, int W, void *plan, size_t plan_bytes, void *stream);
/* slr_synth_group for nb <= 16 frames of a built clip plan in ONE launch of the fused tile kernel (+ one normally empty launch for
 * pieces of more than a segment): consecutive kernels of a stream do not overlap, and the last round of a frame's ~2100 work items
 * runs on a half-empty chip; the frames' block groups are interleaved so that the same tile of consecutive frames runs side by
 * side on one XCD and shares its L2.  Per frame of work at 768x1280: 239 us with 1 frame per launch, 158 with 8, 151 with 16.
 * Arrays of nb entries: disp_f / disp_p / out / norm_out (device pointers per frame; norm_out may be NULL), alpha,
 * frame (index into the plan, every frame at most once); n_items = nb work-item counts (slr_clip_plan_totals) or NULL (all unknown). */
/* (ABI 8) exp_weights of the three clip calls below is a set of flags: bit 0 = exp weights (as before), SLR_SYNTH_VALUES_B4 = `values` is
 * plane-blocked by 4 in memory, [C/4][H][W][4] (C % 4 == 0, the stack below 2 GiB), as slr_pack_planes4 writes it: the 4 planes of a chunk
 * are then ONE 16-byte load per source pixel instead of four 4-byte loads.  The outputs stay [C,H,W]; same arithmetic in the same order. */
#define SLR_SYNTH_VALUES_B4 2
/* in [N,C,H,W] -> out [N,C/4,H,W,4] (C % 4 == 0; out 16-byte aligned, not in place): once per clip for its feature planes. */
int slr_pack_planes4(const float *in, float *out, int N, int C, int H, int W, void *stream);
int slr_synth_group_clip_batch(const float *values, const float *wlogit, const float *wmax, int exp_weights,
                               const float *const *disp_f, const float *const *disp_p, const float *alpha,
                               float *const *out, float *const *norm_out, int C, int H, int W, float eps,
                               void *plan, size_t plan_bytes, int nframes, const int *frame, int nb,
                               const int *n_items, void *stream);

/* slr_synth_group_clip_batch with a SECOND WEIGHT GROUP splatted by the same launch: ONE more value plane with its own
 * weight plane -- the alpha plane of the 2-layer model, which the reference splats with CompositeFluidAlpha_I0 as weights
 * next to the 64 feature planes weighted by Z (..._2layers_alpha_seperate.py:963-1045).  The two groups share the flow, so
 * they share the per-tile records: the records keep the pure bilinear weights, the first group's weight multiplies its values
 * when they are staged, and one extra chunk (the first group's weight | values2 * w2 | w2 per source pixel) yields both
 * normalisers and the second group's sum -- instead of a second launch that rebuilds every tile's records for one plane
 * (41 us per 768x1280 frame).
 *   values2 [H,W], wlogit2 [H,W]: w2 = exp(wlogit2) if exp_weights2 else wlogit2;  out2[k] [H,W] per frame:
 *   out2 = (splat(values2*w2*a, disp_f) + splat(values2*w2*(1-a), disp_p)) / max(same for w2, eps). */
int slr_synth_two_groups_clip_batch(const float *values, const float *wlogit, const float *wmax, int exp_weights,
                                    const float *values2, const float *wlogit2, int exp_weights2,
                                    const float *const *disp_f, const float *const *disp_p, const float *alpha,
                                    float *const *out, float *const *out2, int C, int H, int W, float eps,
                                    void *plan, size_t plan_bytes, int nframes, const int *frame, int nb,
                                    const int *n_items, void *stream);
/* slr_synth_group for frame `frame` of a built clip plan (disp_f / disp_p: that frame's two maps). */
int slr_synth_group_clip(const float *values, const float *wlogit, const float *wmax, int exp_weights,
                         const float *disp_f, const float *disp_p, float alpha, float *out, float *norm_out,
                         int C, int H, int W, float eps, void *plan, size_t plan_bytes, int nframes, int frame,
                         int n_items, void *stream);

/* Global max of a tensor (Z.max(), animating_softmax_splating.py:855) -> result[0].
 * scratch: 1024 floats of device memory. */
int slr_global_max(const float *x, size_t n, float *result, float *scratch, void *stream);

/* ------------------------------------------------------------------ splat: backward */

/* _FunctionSoftsplat.backward.  Replaces kernel_Softsplat_updateGradInput / updateGradFlow
 * and their launcher, softsplat.py:204-255, 257-326, 427-478.
 *   grad_in [N,C,H,W] and/or grad_flow [N,2,H,W]; either may be NULL (needs_input_grad).  With both requested ONE kernel
 *   gathers grad_out once for both; each result is bit-identical to the call that asks for it alone. */
int slr_softsplat_backward(const float *in, const float *flow, const float *grad_out,
                           float *grad_in, float *grad_flow,
                           int N, int C, int H, int W, void *stream);

/* The same with scratch for channel groups (round 6).  The kernel's channels are dealt to 2-4 workgroups per tile: 2-4 on grids
 * smaller than the chip -- the reference TRAINS at 256 x 256, batch 2 per GPU (train_animating_scripts/train_baseline2_pconv.sh:14):
 * 256 source tiles, one workgroup per CU walking all 65 channels --, 2 on larger ones (halves the life of the blocks a flow's sinks
 * make slow: 65 x 768 x 1280 at Euler t=59 230 -> 210 us).  gradInput is per channel (bit-identical); group 0 writes gradFlow itself,
 * the other groups' partial sums go to `ws` and a second small launch adds them on in group order (reproducible; the grouping of the
 * channel sum differs from the one-group kernel by rounding).  slr_softsplat_backward_ws_bytes: bytes of `ws` this shape wants
 * ((groups - 1) * N * 2 * H * W * 4; 0: fewer than 16 channels); a NULL / short `ws` = one group when grad_flow is asked for.
 * slr_softsplat_backward is this call without scratch. */
size_t slr_softsplat_backward_ws_bytes(int N, int C, int H, int W);
int slr_softsplat_backward_ws(const float *in, const float *flow, const float *grad_out, float *grad_in,
                              float *grad_flow, int N, int C, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ splat: the two-direction blend of the training step */

/* The splat half of the training step as one differentiable operator.  Replaces the weighting, the two `cat`, the two 65-plane
 * summation splats, the in-place adds, the clamp and the division of animating_softmax_splating.py:587-692 and autograd's mirror image
 * of them.  Per sample b and direction d (f: start features along disp_f, p: end features along disp_p):
 *   w_d = exp(clamp(logits_d - zmax_d[0], clamp_lo, clamp_hi)) * a_d,   a_f = alpha[b], a_p = 1 - alpha[b]
 *   out = (splat(values_f w_f, disp_f) + splat(values_p w_p, disp_p)) / max(norm, eps),   norm = splat(w_f, disp_f) + splat(w_p, disp_p)
 *   values_d [N,C,H,W];  logits_d [N,1,H,W] or NULL (w_d = a_d; "train_Z" off);  disp_d [N,2,H,W];  alpha [N] ON THE DEVICE;
 *   zmax_d: device scalar (slr_global_max of logits_d, :601 / :646) or NULL (nothing subtracted: use_softmax_splatter_v1);
 *   no clamp ("no_clamp_Z"): clamp_lo = -INFINITY, clamp_hi = INFINITY;  eps 1e-8 (:691).
 *   out [N,C,H,W], norm [N,1,H,W]: every element written here; a destination nobody reaches: norm 0, out exactly +0.0.
 *   splat_ws / ws_flags: the workspace of slr_softsplat_forward (16-byte aligned; the two directions use it one after the other; not SLR_WS_PREBINNED);
 *   scratch: slr_splat_blend_ws_bytes(N, C, H, W) bytes, 16-byte aligned -- the forward's raw sums per direction (two [N,C,H,W]
 *   stacks and two normaliser planes; the weights are applied inside the tile kernels: no weighted stack), the backward's partial sums (0 for a non-positive size: host arithmetic only).  Nothing in it outlives a call:
 *   what the backward needs is the inputs, `out` and `norm`. */
size_t slr_splat_blend_ws_bytes(int N, int C, int H, int W);
int slr_splat_blend_forward(const float *values_f, const float *logits_f, const float *disp_f, const float *values_p,
                            const float *logits_p, const float *disp_p, const float *alpha, const float *zmax_f,
                            const float *zmax_p, float clamp_lo, float clamp_hi, float eps, float *out, float *norm,
                            int N, int C, int H, int W, void *splat_ws, size_t splat_ws_bytes, int ws_flags,
                            void *scratch, size_t scratch_bytes, void *stream);

/* The same with `flags` (slr_splat_blend_forward is this call with flags 0; unknown bits: SLR_E_BADARG before the device is touched).
 * SLR_BLEND_DETERMINISTIC: tile kernels whose per-pixel record lists are ranked by source pixel instead of taking the order in which the
 * waves of a workgroup reached an LDS counter -- `out` and `norm` are then a function of the inputs, the shape and the front-end
 * settings (slr_splat_set_front_end, slr_splat_set_scan_max_tiles; NOT of slr_splat_set_scan_shape's channel groups) alone: the same bits
 * from run to run, under any load.  One exception, which is counted: a flow with so many pile-ups that a deferred piece of the scan front
 * end finds no room in the workspace's entry array or no slabs in its pool is rendered another way (still correct, another summation
 * tree), and WHICH pieces are refused depends on their arrival order.  Every such refusal of a deterministic call increments a 32-bit word
 * of the splat workspace that is zero after slr_splat_workspace_init and is never reset: the guarantee holds while it reads 0.
 * slr_splat_fallback_count_offset: the byte offset of that word in a workspace for this shape (0 for a non-positive size; host
 * arithmetic only) -- read it as a device value, no synchronisation needed to locate it. */
#define SLR_BLEND_DETERMINISTIC 1
int slr_splat_blend_forward_ex(const float *values_f, const float *logits_f, const float *disp_f, const float *values_p,
                               const float *logits_p, const float *disp_p, const float *alpha, const float *zmax_f,
                               const float *zmax_p, float clamp_lo, float clamp_hi, float eps, float *out, float *norm,
                               int N, int C, int H, int W, void *splat_ws, size_t splat_ws_bytes, int ws_flags, int flags,
                               void *scratch, size_t scratch_bytes, void *stream);
size_t slr_splat_fallback_count_offset(int N, int H, int W);

/* Its backward for grad_out = dL/dout [N,C,H,W], with `out` and `norm` as the forward wrote them.  Any of the six gradient pointers may
 * be NULL (needs_input_grad); the others are bit-identical to the call that asks for all six.  grad_logits_d needs logits_d; it is
 * zero where the clamp bites, and the element that holds the maximum (the first one in memory: ties are not split) also receives
 * minus the sum of all the others' -- reduced per workgroup in float64, then in a fixed order: no float atomics, the same bits from
 * run to run.  A source whose target coordinate is not representable has gradient exactly 0 everywhere. */
int slr_splat_blend_backward(const float *values_f, const float *logits_f, const float *disp_f, const float *values_p,
                             const float *logits_p, const float *disp_p, const float *alpha, const float *zmax_f,
                             const float *zmax_p, float clamp_lo, float clamp_hi, float eps, const float *out,
                             const float *norm, const float *grad_out, float *grad_values_f, float *grad_logits_f,
                             float *grad_disp_f, float *grad_values_p, float *grad_logits_p, float *grad_disp_p,
                             int N, int C, int H, int W, void *scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------ maximum-splat family */

/* _FunctionMaximumsplat.forward: out[corner] = max(init, max over sources of in*w).
 * Replaces kernel_Maximumsplat_updateOutput, softsplat.py:12-82, 482-518 (init 0.0, :497). */
int slr_maxsplat_forward(const float *in, const float *flow, float *out, float init,
                         int N, int C, int H, int W,
                         void *ws, size_t ws_bytes, int prebinned, void *stream);

/* _FunctionMaximumWarpNormsplat: max-splat seeded with -1000, then per source pixel the max
 * over its in-bounds corners and itself.  Replaces softsplat.py:84-155, 576-624.
 *   scratch [N,C,H,W] receives the intermediate max-warped tensor. */
int slr_max_warp_norm(const float *in, const float *flow, float *scratch, float *out,
                      int N, int C, int H, int W,
                      void *ws, size_t ws_bytes, int prebinned, void *stream);

/* ------------------------------------------------------------------ decoder elementwise stages (8 f3) */

/* y = relu(x*scale[c] - shift[c]) * mask: eval-mode noise-BN (zero noise), ReLU and the
 * input*mask of the following partial convolution in one pass.  Replaces
 * models/layers/normalization.py:219-231 + blocks.py:229-231 + partialconv2d.py:69.
 *   mask_channels = 1: mask [N,1,H,W];  = C: mask [N,C,H,W];  = 0: mask = (x != 0)
 *   (models/networks/architectures.py:369);  = -1: no mask (plain BN + ReLU of the encoder /
 *   background blocks, blocks.py:66-74).  `mask` is ignored for 0 and -1.
 *   Sizes: N, C <= 65535, H*W < 2^31 - 2^18 (a plane is walked in steps of up to 1024 workgroups of 256). */
int slr_bn_relu_mask(const float *x, const float *scale, const float *shift, const float *mask,
                     int mask_channels, float *y, int N, int C, int H, int W, void *stream);

/* Partial-convolution epilogue on the bias-free convolution output raw0:
 *   um_raw = mask_box*mask_scale  (= conv(mask, ones[out,in,k,k]), partialconv2d.py:61: the k x k box
 *            filter of a channel-uniform mask times Cin, or of the channel sum of the mask times 1)
 *   o = (raw0*ratio + b)*um,  um = clamp(um_raw,0,1),  ratio = winsize/(um_raw + 1e-8)*um
 * then optionally  o += residual            (blocks.py:248)
 * or               o  = relu(o*next_scale - next_shift)*um   (BN + ReLU + input*mask of the next
 *                       partial convolution of the block, blocks.py:233-236 / partialconv2d.py:69).
 * Replaces models/layers/partialconv2d.py:64-74.
 *   raw0 [N,C,H,W]; mask_box [N,1,H,W]; residual [N,C,H,W] or NULL; next_scale/next_shift [C] or
 *   NULL (exclusive with residual); um_out [N,1,H,W] or NULL receives um; winsize = Cin*k*k.
 *   Sizes: N, C <= 65535, H*W < 2^31 - 2^18. */
int slr_pconv_epilogue(const float *raw0, const float *bias, const float *mask_box, float mask_scale,
                       const float *residual, const float *next_scale, const float *next_shift,
                       float *out, float *um_out, float winsize, int N, int C, int H, int W, void *stream);

/* The split-f16 convolution kernels below represent an activation x as two f16 halves of x * xscale (`xscale` of the
 * forward calls: a power of two in (0, 64]; 64 = the default): exact-domain for |x| < 65472 / xscale -- 1023 at 64
 * (post-BN activations are O(1 .. 10^2)), 65472 at 1 (the low halves of values below 2^-3 are then f16 subnormals:
 * absolute error <= 2^-25 per value).  The LOWER edge: the lo half is a normal f16 number only for |x| * xscale >= 2^-2; below that
 * it is a subnormal (absolute resolution 2^-25 / xscale per value), below |x| * xscale = 2^-14 the hi half is one too and below
 * 2^-25 the value is 0.  gfx950 keeps f16 subnormals in the conversion and in the A / B inputs of v_mfma_f32_32x32x16_f16
 * (measured, tests/test_gpu_conv_range.py: bit-exact probes), so the error grows smoothly, 16 x per 2^-4 of input magnitude.
 * Measured E = max|out - fp64| / max|fp64| of a layer by the standard deviation of its input (19 kernel / shape cases each):
 *     input std        >= 2^-4    2^-8      2^-12     2^-16     2^-20        (a plain fp32 convolution: 0.9 - 3e-7 throughout)
 *     xscale 64 (E <=)  5.9e-7    6.3e-7    1.4e-6    2.1e-5    3.5e-4
 *     xscale 1  (E <=)  7.5e-7    4.9e-6    8.7e-5    1.4e-3    2.4e-2       (5.9e-7 at std >= 1)
 * i.e. worse than 10 x plain fp32 below an input std of about 2^-13 at xscale 64 and about 2^-7 at xscale 1.  Nothing counts or
 * reports this underflow: it loses precision gradually, it does not make a frame wrong.  A larger activation is CLAMPED at the upper edge (no inf / NaN), which makes the frame wrong
 * rather than inexact -- the reference's fp32 convolution has no such limit -- so every wave that had to clamp adds to
 * a counter.  The counter is ONE PER DEVICE (shared by all streams and host threads using that device).
 *   slr_conv_saturation_count: *count = the counter of the current device after everything enqueued on `stream` so far
 *       (synchronises that stream with the host); reset != 0 zeroes it.
 *   slr_conv_saturation_record: asynchronous -- the current value is copied into *host_slot (PINNED host memory) in
 *       stream order; read it after synchronising.  Differences of consecutive records tell which piece of work clamped.
 * The Python networks react to a non-zero count (smaller xscale, then fp32 convolutions, or an exception: nets.py). */
int slr_conv_saturation_count(unsigned long long *count, int reset, void *stream);
int slr_conv_saturation_record(unsigned *host_slot, void *stream);

/* ------------------------------------------------------------------ decoder convolution on the matrix cores (8 f3) */

/* 3x3 / stride 1 / zero-pad 1 convolution, fp32 in / fp32 out: implicit GEMM on
 * v_mfma_f32_32x32x16_f16 with split operands (x = hi + lo in f16, three MFMAs per product, fp32
 * accumulation; csrc/conv.hip): fp32-class accuracy (2-5e-6 abs on outputs of magnitude 4, like
 * MIOpen's fp32 Winograd) at several times the rate of the fp32 matrix pipe.  Any Cin / Cout
 * (channels are zero-padded to multiples of 16 / 32 inside the weight buffer).
 *   Weights are prepared once per layer with slr_conv3x3_split_weights into a buffer of
 *   slr_conv3x3_weight_bytes(Cout, Cin) bytes; `wscale` is a power of two that brings max|w|
 *   near 2^12 (f16 range) and must be passed unchanged to the forward calls.  A weight buffer (3x3, 1x1, Winograd) holds fewer than
 *   2^30 - 256 padded elements. */
/* `layout` flags of the forward calls: the activation BETWEEN two of these kernels may be kept channel-blocked,
 * [N, C/8, H, W, 8] instead of [N, C, H, W] (C % 8 == 0): the consumer then stages an item's 8 channels with two
 * 16-byte loads instead of eight 4-byte loads, the producer stores 16 bytes per lane without a transpose.
 * Same values, same arithmetic; only the memory order of that one tensor differs. */
#define SLR_CONV_IN_B8  1      /* `in` / `x` is channel-blocked */
#define SLR_CONV_OUT_B8 2      /* `out` is written channel-blocked */
#define SLR_CONV_RES_B8 4      /* `residual` is channel-blocked (only together with SLR_CONV_OUT_B8) */
/* The fp32 rung (ABI 6): with SLR_CONV_F32 in `layout` the same entry points run the convolution on v_mfma_f32_32x32x2_f32 --
 * fp32 operands, fp32 products, fp32 accumulation: the arithmetic of the reference's own convolutions
 * (models/layers/partialconv2d.py:61-74, models/layers/blocks.py:173-248), no pre-scale, no clamp, no limit on the magnitude of the
 * activations -- at the rate of the fp32 matrix pipe (157 TFLOP/s, 1/16 of the f16 rate).  `wsplit` must then come from
 * slr_conv3x3_f32_weights / slr_conv1x1_f32_weights (same byte counts as the split-f16 buffers), wscale = xscale = 1. */
#define SLR_CONV_F32    8
/* Together with SLR_CONV_F32 on the 3x3 entry points (Cout > 4): the convolution as Winograd F(2x2, 3x3) on the same fp32 matrix
 * instructions -- 16 multiplications per (input channel, output channel, 2x2 output tile) instead of 36, the transforms are additions
 * (csrc/conv_wino.hpp).  fp32 operands, products and accumulation as on the plain fp32 rung; the rounding error of the transform
 * domain is within a small factor of the direct fp32 convolution's (tests/test_gpu_conv_f32.py: both against fp64).  `wsplit` must then
 * come from slr_conv3x3_wino_weights (slr_conv3x3_wino_weight_bytes: 16 transformed values per weight instead of 9). */
#define SLR_CONV_WINO   16
#define SLR_CONV_SKIP_B8 32    /* slr_conv3x3_forward_skip / slr_pconv3x3_forward_skip: `skip_in` is channel-blocked */
#define SLR_CONV_POOL_OUT 64   /* ... and `out` is avgpool3x3s2 of the result, [N,Cout,(H-1)/2+1,(W-1)/2+1] channel-blocked (needs pool_ws) */
#define SLR_CONV_UP_OUT 128    /* ... or `out` is the x2 bilinear up-sampling of the result, [N,Cout,2H,2W] channel-blocked (needs pool_ws) */
/* Cout <= 4 (the 128 -> 3 end of the decoders): the 3x3 entry points run a kernel of their own on EITHER rung -- fp32 FMAs on the vector
 * ALUs (csrc/conv_few.hpp; the narrowest matrix-core tile would compute 32 channels for 3), i.e. the reference's arithmetic: both
 * weight-preparation calls then write plain fp32 weights into the buffer, wscale / xscale are accepted and unused, nothing saturates. */

size_t slr_conv3x3_weight_bytes(int Cout, int Cin);
int slr_conv3x3_split_weights(const float *w /* [Cout,Cin,3,3] */, void *wsplit, int Cout, int Cin,
                              float wscale, void *stream);
int slr_conv3x3_f32_weights(const float *w /* [Cout,Cin,3,3] */, void *wfrag /* slr_conv3x3_weight_bytes */, int Cout, int Cin,
                            void *stream);
size_t slr_conv3x3_wino_weight_bytes(int Cout, int Cin);
int slr_conv3x3_wino_weights(const float *w /* [Cout,Cin,3,3] */, void *wfrag /* slr_conv3x3_wino_weight_bytes */, int Cout, int Cin,
                             void *stream);

/* out = conv3x3(pre(in)) + bias + residual, pre(x) = relu(x*pre_scale[c] - pre_shift[c]) when pre_scale
 * is given (eval-mode noise-BN + ReLU in front of the convolution, models/layers/blocks.py:66-74 +
 * normalization.py:219-231), identity otherwise.  bias [Cout] or NULL; residual [N,Cout,H,W] or NULL
 * (the x_a + x_b of ResNet_Block, blocks.py:87).
 * Sizes of every 3x3 entry point: N < 65536, Cout < 2^20, Cin*H*W < 2^31 (a sample's input is indexed with 32 bits), H*W < 2^31 - 1024,
 * N*Cout*H*W < 2^40 (offsets of samples and of output planes are 64-bit); a batch may hold more than 2^31 elements. */
int slr_conv3x3_forward(const float *in, const void *wsplit, const float *bias, const float *residual, float *out,
                        int N, int Cin, int Cout, int H, int W, float wscale, float xscale,
                        const float *pre_scale, const float *pre_shift, int layout, void *stream);

/* One partial convolution of ResNet_Block_Pconv2 in a single kernel
 * (models/layers/partialconv2d.py:41-81 with blocks.py:229-239,248):
 *   xin = relu(x*pre_scale - pre_shift) * mask     (prologue; skipped when pre_scale is NULL: x is
 *         then the already activated and masked input, i.e. the output of a previous call with
 *         next_scale / next_shift)
 *         mask [N,1,H,W]: channel-uniform mask;  mask = NULL: the per-element mask (x != 0) of
 *         models/networks/architectures.py:369 (needs pre_scale: x must be the raw input)
 *   raw0 = conv3x3(xin)                             (bias-free)
 *   um_raw = conv(mask, ones[Cout,Cin,3,3]) (:61) = box3x3(mask)*Cin, resp. box3x3(sum_c (x != 0));
 *            computed inside the kernel from the mask plane of the block's halo (exact integers)
 *   out  = epilogue(raw0) exactly as slr_pconv_epilogue: (raw0*ratio + b)*um, then `+ residual`
 *          or relu(.*next_scale - next_shift)*um;  um = clamp(um_raw, 0, 1) -> um_out.
 * Same operations in the same order as slr_bn_relu_mask -> convolution -> slr_pconv_epilogue. */
int slr_pconv3x3_forward(const float *x, const float *pre_scale, const float *pre_shift, const float *mask,
                         const void *wsplit, float wscale, float xscale, const float *bias, const float *residual,
                         const float *next_scale, const float *next_shift, float *out, float *um_out,
                         int N, int Cin, int Cout, int H, int W, int layout, void *stream);

/* ABI 10.  The same two convolutions with the residual block's 1x1 skip branch INSIDE the kernel (models/layers/blocks.py:83-87 and
 * :243-248: x_a + x_b with x_b = conv1x1(block input)):
 *   out = [3x3 convolution with its whole epilogue, as above, without residual / next-BN] + conv1x1(skip_in) (+ skip_bias)
 * The accumulators take the 3x3 epilogue, change to the skip operands' scale (a power of two: exact) and go on as the accumulators of
 * the skip convolution over skip_cin more input channels (one tap): no separate 1x1 kernel, no write and re-read of its result.
 * Against the two-kernel form (slr_conv1x1_forward -> residual) the result differs by the order of the last additions only (fp32
 * rounding; tests/test_gpu_parity.py).  skip_wsplit: slr_conv1x1_split_weights(Cout, skip_cin, skip_wscale); the skip input shares
 * `xscale`.  No SLR_CONV_WINO; with SLR_CONV_F32 only Cout > 64 and skip_wscale = 1; main input and skip input channel-blocked (SLR_CONV_IN_B8 and
 * SLR_CONV_SKIP_B8 both set, skip_cin % 8 == 0), Cout > 4; anything else is SLR_E_BADARG -- callers keep the two-kernel form there
 * (the networks' 3-channel first blocks and 65- / 3-channel ends).
 * With SLR_CONV_POOL_OUT (and SLR_CONV_OUT_B8, Cout > 64) the "Down" block's nn.AvgPool2d(3, stride=2, padding=1) (blocks.py:196-199)
 * happens in the epilogue: the full-resolution result -- whose only reader is the pool -- is never written; `out` is the pooled tensor,
 * um_out stays full resolution.  A wave pools the 4 x 16 pixels of its tile in registers; the pooled pixels that need the row above /
 * the column left of the tile are completed by a small second launch from side buffers in pool_ws (slr_conv_pool_ws_bytes: the last row
 * of every tile row and the last column of every tile column, ~16 % of the full-resolution tensor).  Same 9 terms per pooled pixel as
 * slr_avgpool3x3s2, summed rows first: equal to the two-kernel form to fp32 rounding.  pool_ws = NULL otherwise.
 * Both resampling epilogues: N * Cout / 8 <= 65535 (the second launch has one grid row per sample and 8-channel group). */
size_t slr_conv_pool_ws_bytes(int N, int Cout, int H, int W);
/* With SLR_CONV_UP_OUT (same conditions) the "Up" block's nn.Upsample(scale_factor=2, mode='bilinear') (blocks.py:200-203) happens in the
 * epilogue: a tile's 8 x 32 pixels give the 16 x 64 output pixels below them; all but the first / last row and column of that block come
 * from the wave's registers and neighbouring lanes, those borders are written by a second launch from side buffers (pool_ws of
 * slr_conv_up_ws_bytes: first and last row / column of every tile).  Expression and order of slr_upsample_bilinear2x: bit-identical to
 * the two-kernel form.  The low-resolution result is never written; um_out stays at the convolution's resolution. */
size_t slr_conv_up_ws_bytes(int N, int Cout, int H, int W);
int slr_conv3x3_forward_skip(const float *in, const void *wsplit, const float *bias, float *out,
                             int N, int Cin, int Cout, int H, int W, float wscale, float xscale,
                             const float *pre_scale, const float *pre_shift,
                             const float *skip_in, const void *skip_wsplit, const float *skip_bias /* [Cout] or NULL */, int skip_cin,
                             float skip_wscale, void *pool_ws, size_t pool_ws_bytes, int layout, void *stream);
int slr_pconv3x3_forward_skip(const float *x, const float *pre_scale, const float *pre_shift, const float *mask,
                              const void *wsplit, float wscale, float xscale, const float *bias, float *out, float *um_out,
                              int N, int Cin, int Cout, int H, int W,
                              const float *skip_in, const void *skip_wsplit, int skip_cin, float skip_wscale,
                              void *pool_ws, size_t pool_ws_bytes, int layout, void *stream);

/* Cout <= 4 (the 128 -> 3 end of the decoders), channel-blocked input: the first convolution of the block as slr_conv3x3_forward /
 * slr_pconv3x3_forward, and next to it skip_out [N,Cout,H,W] = conv1x1(in) + skip_bias -- the block's skip branch on the SAME (raw) input
 * (blocks.py:192-193, 243-247), which the caller hands to the block's second convolution as its residual.  The 128 input planes are read
 * from HBM once instead of twice.  skip_w4: plain fp32 weights [Cin][4] (row ci = w[0..3][ci], zero padded), 16-byte aligned.  Either rung
 * (the <= 4-channel kernel is fp32 FMAs on both).  Bit-identical to slr_conv1x1_small on the same input. */
int slr_conv3x3_forward_skipout(const float *in, const void *wsplit, const float *bias, const float *residual, float *out,
                                int N, int Cin, int Cout, int H, int W, float wscale, float xscale,
                                const float *pre_scale, const float *pre_shift,
                                const float *skip_w4, const float *skip_bias /* [Cout] or NULL */, float *skip_out, int layout, void *stream);
int slr_pconv3x3_forward_skipout(const float *x, const float *pre_scale, const float *pre_shift, const float *mask,
                                 const void *wsplit, float wscale, float xscale, const float *bias, const float *residual,
                                 const float *next_scale, const float *next_shift, float *out, float *um_out,
                                 int N, int Cin, int Cout, int H, int W,
                                 const float *skip_w4, float *skip_out, int layout, void *stream);

/* ABI 27.  The narrow end without its widest tensor.  A 128-channel block's second partial convolution whose result has ONE pair of
 * readers -- the next block's 128 -> 3 first convolution and its 1x1 skip -- never writes that result: a 3x3 convolution onto 3 channels
 * is a per-pixel linear map onto 27 columns (tap * 3 + co) followed by a gather of nine shifted columns, the map needs no halo, and its
 * operand is what the wide kernel holds in its accumulators when it finishes.
 *   slr_pconv3x3_forward_tail: slr_pconv3x3_forward (no prologue; x, residual channel-blocked; split-f16 rung; Cout = 128) up to and
 *     including the residual add, o; then per pixel  Z[tap * 3 + co] = sum_ci relu(o * tail_scale - tail_shift)[ci] * um * w_aa[co, ci, tap]
 *     (the next block's first BN, the update mask just computed) and  Z[27 + co] = sum_ci o[ci] * w_b[co, ci],  both operands scaled by
 *     xscale, clamped, counted (slr_conv_saturation_count) and split like every staged activation, products in the kernels' order.
 *     z_out [N,32,H,W] fp32 planar, in the operands' scale (x xscale x the branch's wscale), planes 30-31 zero; um_out as always.
 *   slr_conv_tail_weights: w_aa [3,Cin,3,3] and w_b [3,Cin,1,1] -> the split column weights, slr_conv_tail_weight_bytes(Cin) bytes
 *     (Cin: the wide convolution's OUTPUT channels, a multiple of 32), [tile of 32 channels][activated | raw][chunk of 16][hi | lo][lane 64][8];
 *     each branch has its own power-of-two wscale.  slr_conv_tail_weight_source: (operand, half, row of the tile, input channel) of one
 *     element of that buffer -- the layout, on the host.
 *   slr_narrow_gather: raw[co] = sum over the nine taps, ascending, of plane tap * 3 + co shifted by the tap (zero outside the image),
 *     then the partial epilogue of the <= 4-channel kernel operation for operation with `mask` [N,1,H,W] (the wide kernel's um_out) and
 *     Cin input channels behind every mask value: out [N,3,H,W] = relu(((raw * ratio + bias) * um) * next_scale - next_shift) * um
 *     (next_scale = NULL: without), um_out [N,1,H,W], skip_out [N,3,H,W] = Z[27 + co] (+ skip_bias): what slr_pconv3x3_forward_skipout
 *     returns, to the rounding of a different order of the same sums.  Sizes: N < 65536, H*W < 2^31 - 64, H <= 262140. */
size_t slr_conv_tail_weight_bytes(int Cin);
int slr_conv_tail_weight_source(int Cin, int element, int *operand, int *half, int *row, int *ci);
int slr_conv_tail_weights(const float *w_aa, const float *w_b, void *wtail, int Cin, float wscale_aa, float wscale_b, void *stream);
int slr_pconv3x3_forward_tail(const float *x, const float *mask, const void *wsplit, float wscale, float xscale, const float *bias,
                              const float *residual /* [N,Cout,H,W] channel-blocked, or NULL */, const float *tail_scale, const float *tail_shift,
                              const void *wtail, float *z_out, float *um_out, int N, int Cin, int Cout, int H, int W, void *stream);
int slr_narrow_gather(const float *z, const float *mask, const float *bias, const float *next_scale, const float *next_shift,
                      const float *skip_bias /* [3] or NULL */, float *out, float *um_out, float *skip_out, int N, int Cin, int H, int W,
                      float wscale, float skip_wscale, float xscale, void *stream);

/* 1x1 convolution (skip branch of the residual blocks, models/layers/blocks.py:192-193,243-247) on the same
 * split-f16 arithmetic: out = conv1x1(in) + bias.  HBM-bound, no LDS.  Weights prepared once per layer with
 * slr_conv1x1_split_weights into slr_conv1x1_weight_bytes(Cout, Cin) bytes; wscale as for the 3x3 kernel.
 * Sizes: N < 65536, Cout < 2^20, H*W < 2^31 - 128, Cin*H*W < 2^40: one sample may hold more than 2^31 elements. */
size_t slr_conv1x1_weight_bytes(int Cout, int Cin);
int slr_conv1x1_split_weights(const float *w /* [Cout,Cin,1,1] */, void *wsplit, int Cout, int Cin,
                              float wscale, void *stream);
int slr_conv1x1_f32_weights(const float *w /* [Cout,Cin,1,1] */, void *wfrag /* slr_conv1x1_weight_bytes */, int Cout, int Cin,
                            void *stream);
int slr_conv1x1_forward(const float *in, const void *wsplit, const float *bias /* [Cout] or NULL */, float *out,
                        int N, int Cin, int Cout, int H, int W, float wscale, float xscale, int layout, void *stream);

/* ------------------------------------------------------------------ decoder resampling stages (8 f3) */

/* nn.AvgPool2d(3, stride=2, padding=1) (count_include_pad): "Down" of models/layers/blocks.py:196-199.
 *   in [N,C,H,W] -> out [N,C,(H-1)/2+1,(W-1)/2+1].  Sizes: N*C < 65536, H*W < 2^30. */
int slr_avgpool3x3s2(const float *in, float *out, int N, int C, int H, int W, int b8 /* both tensors channel-blocked */,
                     void *stream);

/* nn.Upsample(scale_factor=2, mode='bilinear') (align_corners=False): "Up" of blocks.py:200-203.
 *   in [N,C,H,W] -> out [N,C,2H,2W].  Sizes: N*C < 65536, H*W < 2^28 (the output plane is indexed with an int). */
int slr_upsample_bilinear2x(const float *in, float *out, int N, int C, int H, int W, int b8 /* both tensors channel-blocked */,
                            void *stream);

/* 1x1 convolution onto 1..4 output channels (the skip branch of the decoder's last block,
 * blocks.py:192-193,243-247 with configs.py:117-137): out = bias + w . in;  w [Cout,Cin], bias [Cout] or NULL.
 *   NCHW input requires H*W % 4 == 0 and 16-byte aligned tensors.  Sizes: N < 65536, H*W < 2^31 - 256, Cout*Cin < 2^31. */
int slr_conv1x1_small(const float *in, const float *w, const float *bias, float *out,
                      int N, int Cin, int Cout, int H, int W, int in_b8 /* `in` channel-blocked; `out` is always NCHW */,
                      void *stream);

/* ------------------------------------------------------------------ motion U-Nets (ABI 11; csrc/motion.hip, csrc/conv4x4.hip)
 * The networks that predict the motion field from a still image: Unet4Motion (models/networks/architectures.py:382-493, used by
 * models/unet_motion.py:30-109) and SPADEUnet4MaskMotion (architectures.py:602-743 with SPADE, models/networks/networks.py:422-463, used by
 * unet_motion.py:111-191).  All their convolutions run on the fp32 rung (v_mfma_f32_32x32x2_f32): the 3x3 ones through
 * slr_conv3x3_forward with SLR_CONV_F32, the encoder's 4x4 / stride 2 ones through the entry points below.  All tensors NCHW fp32. */

/* Conv2d(Cin, Cout, 4, stride 2, padding 1) (architectures.py:389-396, 612-619):
 *   out = post(conv4x4s2(pre(in)) + bias),  pre(x) = leaky_relu(x, slope) when `leaky` (the LeakyReLU(0.2) in front of conv2..conv8,
 *   :448-462), identity otherwise;  post(y) = y * post_scale[c] + post_shift[c] when given (an eval-mode BatchNorm folded to an affine,
 *   :449-460), identity when both are NULL.  in [N,Cin,H,W], H, W >= 2 -> out [N,Cout,(H-2)/2+1,(W-2)/2+1].  bias [Cout] or NULL.
 *   Weights are prepared once per layer into fragment order with slr_conv4x4s2_f32_weights (slr_conv4x4s2_weight_bytes bytes). */
size_t slr_conv4x4s2_weight_bytes(int Cout, int Cin);
int slr_conv4x4s2_f32_weights(const float *w /* [Cout,Cin,4,4] */, void *wfrag, int Cout, int Cin, void *stream);
int slr_conv4x4s2_forward(const float *in, const void *wfrag, const float *bias, const float *post_scale, const float *post_shift,
                          float *out, int N, int Cin, int Cout, int H, int W, int leaky, float slope, void *stream);

/* SPADE with nn.InstanceNorm2d (affine=False, biased variance; networks.py:441-463):
 *   out = (x - mean) * rsqrt(var + eps) * (1 + gamma) + beta, mean / var per (n, c) plane of x [N,C,H,W];
 *   gamma_beta [N,2C,H,W]: gamma = channels 0..C-1, beta = channels C..2C-1 (mlp_gamma and mlp_beta as ONE 3x3 convolution). */
int slr_instnorm_spade(const float *x, const float *gamma_beta, float *out, int N, int C, int H, int W, float eps, void *stream);

/* The segmap of a SPADE layer (networks.py:446-457): F.interpolate(in, size=(H >> k, W >> k)) per channel, bilinear
 * (align_corners=False) for every channel but `nearest_channel` (the mask: mode='nearest'; -1 = none).  in [N,C,H,W] ->
 * out [N,C,H>>k,W>>k]; H and W multiples of 2^k, k < 16.  Sizes: N*C < 65536, H*W < 2^31 - 256. */
int slr_resize_segmap(const float *in, float *out, int N, int C, int H, int W, int k, int nearest_channel, void *stream);

/* The decoders' x2 up-sampling + skip concatenation: out[n] = cat(up(a[n]), up(b[n])) [N,Ca+Cb,2H,2W] with a [N,Ca,H,W], b [N,Cb,H,W]
 * (Cb = 0: a alone).  up = nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False) (the expression of
 * slr_upsample_bilinear2x) except channel `nearest_channel` of EACH source, which is nearest (architectures.py:712-740; -1 = none).
 * relu = 1: ReLU of the inputs (up(relu(cat)), architectures.py:463-489 and e8 at :710); 2: ReLU of the output (:715-741); 0: none.
 * Sizes: N*(Ca+Cb) < 65536, 4*H*W < 2^31 - 256 (the output plane is indexed with an int). */
int slr_upsample2x_concat(const float *a, int Ca, const float *b, int Cb, float *out, int N, int H, int W, int nearest_channel, int relu,
                          void *stream);

/* ------------------------------------------------------------------ clip-evaluation metrics (ABI 12; csrc/metrics.hip)
 * The reference scores clips with evaluation/animation/metrics.py (psnr, ssim_metric, perceptual_sim) on models/losses/ssim.py and
 * models/networks/pretrained_networks.py (PNet "vgg").  Images are float [N,C,H,W] in [0,1] (u8 = 0) or uint8 [N,H,W,C] frames as
 * decoders give them (u8 = 1; the value is v / 255.0f, i.e. ToTensor).  Reductions are deterministic (fixed order, no atomics) and a
 * result depends on its own image only.  The VGG16 convolutions run on slr_conv3x3_forward with SLR_CONV_F32 (channel-blocked
 * features, the ReLU between them as the prologue with scale 1 / shift 0). */

/* models/losses/ssim.py:_ssim (window_size odd, 1 .. 15, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2) and the squared error of
 * evaluation/animation/metrics.py:psnr in ONE pass: out [N,2] = per image (ssim, mse).  mask [N,1,H,W] or NULL: with a mask
 * ssim = sum(mask * mean_c(ssim_map)) / max(sum(mask), 1) (ssim.py:61-67) and mse = sum(mask * err^2) / (3 max(sum(mask), 1))
 * (metrics.py:12-17); without, both are means over C, H, W (ssim.py:76, metrics.py:20).  ws: slr_ssim_ws_bytes(N, H, W) bytes,
 * 8-byte aligned (per-tile partial sums).  Sizes: N < 65536, C <= 64, H*W < 2^31 - 128, N*C*H*W < 2^40. */
size_t slr_ssim_ws_bytes(int N, int H, int W);
int slr_ssim_mse(const void *img1, const void *img2, int u8, const float *mask, float *out, int N, int C, int H, int W,
                 int window_size, void *ws, size_t ws_bytes, void *stream);

/* The input of PNet's VGG16 (metrics.py:29 + pretrained_networks.py:45-46, 73-74): out [N,3,H,W] NCHW = ((x * 2 - 1) - shift) / scale
 * with from01 = 1 (images in [0,1]; uint8 frames need it), (x - shift) / scale with from01 = 0 (PNet.forward's own [-1,1] input). */
int slr_vgg_prep(const void *img, int u8, int from01, float *out, int N, int H, int W, void *stream);

/* nn.ReLU + nn.MaxPool2d(2, stride 2) of torchvision's vgg16.features (floor mode: 45 x 80 -> 22 x 40):
 * in [N,C,H,W] -> out [N,C,H/2,W/2], both channel-blocked [N,C/8,.,.,8], C % 8 == 0, 16-byte aligned.  A window that holds a NaN
 * gives NaN, as torch's does (the training loss runs this kernel too). */
int slr_relu_maxpool2x2_b8(const float *in, float *out, int N, int C, int H, int W, void *stream);

/* 1 - cos_sim(relu(f0), relu(f1)) of pretrained_networks.py:11-31 and :82 (normalize_tensor eps 1e-10; mean over H, W):
 * f0, f1 [N,C,H,W] channel-blocked (C % 8 == 0), out [N].  ws: slr_feature_cos_ws_bytes(N, H, W) bytes, 8-byte aligned. */
size_t slr_feature_cos_ws_bytes(int N, int H, int W);
int slr_feature_cos_distance(const float *f0, const float *f1, float *out, int N, int C, int H, int W, void *ws, size_t ws_bytes,
                             void *stream);

/* ------------------------------------------------------------------ training loss (ABI 14; csrc/loss.hip)
 * The generator loss of the reference, models/losses/synthesis.py:61-109 (SynthesisLoss, --losses 1.0_l1 10.0_content): nn.L1Loss and the
 * VGG19 PerceptualLoss (:166-185; models/networks/architectures.py:82-115), each with its gradient to the predicted image.  The VGG19 is
 * frozen: its 13 convolutions run on slr_conv3x3_forward with SLR_CONV_F32 and channel-blocked features, and so do their backward-data
 * convolutions (3x3 / stride 1 / pad 1: the same convolution with the weights flipped and transposed).  The entry points below are the
 * device code around them.  None synchronises; sums are deterministic (per-workgroup partial sums in double, added in a fixed order by a
 * second launch -- no atomics).  `gscale` is a DEVICE scalar: the gradient arriving at the loss value (autograd's grad_output). */

/* Partial sums of slr_l1_loss_grad / slr_feature_l1_gate_b8 for a tensor of N*C*H*W elements. */
size_t slr_loss_ws_bytes(int N, int C, int H, int W);

/* nn.L1Loss() (synthesis.py:134-140): loss[0] = mean |pred - gt| over all elements of [N,C,H,W] (any count, any 4-byte alignment);
 * with grad: grad = sign(pred - gt) * (coef * gscale[0]), sign(0) = 0, the product formed in fp32 in that order (coef = 1 / count for
 * the mean).  loss or grad may be NULL (not both); ws (slr_loss_ws_bytes, 8-byte aligned) is needed with loss. */
int slr_l1_loss_grad(const float *pred, const float *gt, float *loss, float *grad, float coef, const float *gscale,
                     int N, int C, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* One pass over a VGG19 slice's features (PerceptualLoss.forward, synthesis.py:176-185: criterion(pred_fs[i], gt_fs[i]) and its backward,
 * with the nn.ReLU in front of it): a, b raw (pre-ReLU) features of prediction / ground truth, g_in the gradient arriving at relu(a)
 * from the layers above, all [N,C,H,W] channel-blocked, C % 8 == 0, 16-byte aligned.
 *   sum[0] = sum |relu(a) - relu(b)|                                           (needs b and ws; the caller divides by the count)
 *   g_out  = a <= 0 ? 0 : g_in + sign(relu(a) - relu(b)) * (coef * gscale[0])  (g_in = NULL counts as 0)
 *   b = NULL: g_out = a <= 0 ? 0 : g_in, the ReLU backward of a layer that ends no slice.
 * sum or g_out may be NULL (not both).  fp32 operations in the order written: bit-equal to the same expression in torch.  relu is
 * torch.relu: a NaN in a or b makes the sum NaN; sign(NaN) = 0 and the gate closes on `<= 0` only (torch's ReLU backward), so a NaN a passes
 * g_in and g_out holds no NaN of theirs. */
int slr_feature_l1_gate_b8(const float *a, const float *b, const float *g_in, float *sum, float *g_out, float coef,
                           const float *gscale, int N, int C, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* Backward of slr_relu_maxpool2x2_b8 (nn.ReLU + nn.MaxPool2d(2, 2) of torchvision's vgg19.features): x [N,C,H,W] the raw activation,
 * g [N,C,H/2,W/2] the pooled gradient, out [N,C,H,W], all channel-blocked.  g goes to the first maximum of its window in row-major
 * order (torch's choice) if that maximum is > 0; every other element, the last row / column of an odd H / W included, gets 0.
 * A window with NaNs: torch's max_pool2d replaces on `>` or on a NaN, so g goes to the window's LAST NaN, and torch's ReLU backward
 * closes on `<= 0` only, so it arrives there.  Every element of out is written exactly once. */
int slr_relu_maxpool2x2_backward_b8(const float *x, const float *g, float *out, int N, int C, int H, int W, void *stream);

/* ------------------------------------------------------------------ trainable 3x3 convolutions (ABI 15; csrc/conv_grad.hip)
 * What torch autograd computes for the learning 3x3 / stride 1 / pad 1 convolutions of the reference's decoder: nn.Conv2d
 * (models/layers/blocks.py:66-87) and PartialConv2d (models/layers/partialconv2d.py:61-74).  The gradient to the input is the forward
 * kernel with flipped, transposed weights (SLR_CONV_F32); the entry points below are the rest.  None synchronises, none uses atomics:
 * the same inputs and the same split count give the same bits from run to run. */
#define SLR_GRAD_X_B8 1        /* `x` is channel-blocked, [N,Cin/8,H,W,8] (Cin % 8 == 0, 16-byte aligned) */
#define SLR_GRAD_G_B8 2        /* `g` (and `gr`) is channel-blocked, [N,C/8,H,W,8] (C % 8 == 0, 16-byte aligned) */

/* Workspace of the two calls below, in bytes:
 *   al256(N * Cout * ceil(H * W / 256) * 8)          the bias gradient's partial sums (double)
 * + al256(S * 9 * Cout * Cin * 4)                    the weight gradient's partial sums of S slabs (float); nothing for Cin = 0
 * S = min(splits, chunks) for splits > 0; for splits = 0 the library's choice min(ceil(512 / channel tiles), chunks, 32 MiB / (36 Cout Cin))
 * with chunks = N * ceil(H / 2) * ceil(W / 32) and channel tiles = ceil(Cin / 64) * ceil(Cout / 64) (csrc/slr_tuning.hpp): at most
 * 32 MiB + the bias part.  Cin = 0: the bias part alone, what the scale / bias pass needs.  0 for sizes the calls refuse. */
size_t slr_conv3x3_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int splits);

/* Weight and bias gradient of out = conv3x3(x, w) + b (what autograd's backward of F.conv2d, blocks.py:66-87, returns for weight and bias):
 *   dw[co][ci][ky][kx] = sum_{n,y,x} g[n,co,y,x] * x[n,ci,y+ky-1,x+kx-1] (zero padding), plain [Cout,Cin,3,3];  db[co] = sum g[n,co,y,x].
 * x [N,Cin,H,W], g [N,Cout,H,W]; any Cin, Cout, H, W >= 1.  fp32 products and sums on v_mfma_f32_32x32x2_f32 inside a slab of pixels, the
 * slabs added in double in a fixed order; db in double throughout.  splits: 0 = the library's choice, > 0 = that many slabs (at most one
 * per chunk).  layout: SLR_GRAD_X_B8 | SLR_GRAD_G_B8.  db may be NULL.  ws: 256-byte aligned, else SLR_E_WORKSPACE.
 * Sizes of both calls: N * max(Cin, Cout) * H * W < 2^31 - 1024, N * Cout <= 65535, channels <= 65535 * 64, 9 * Cout * Cin < 2^31 - 64. */
int slr_conv3x3_weight_grad(const float *x, const float *g, float *dw, float *db, int N, int Cin, int Cout, int H, int W,
                            int splits, int layout, void *ws, size_t ws_bytes, void *stream);

/* One pass over the gradient g [N,C,H,W] arriving at a partial convolution's output (the backward of partialconv2d.py:64-74,
 * out = (raw * ratio + b) * um):  gr = g * r with r = ratio * um [N,1,H,W] -- the gradient at raw, input of the backward-data convolution
 * and of the weight gradient, in g's layout (SLR_GRAD_G_B8), bit-equal to the fp32 product -- and db[c] = sum g * um (um [N,1,H,W];
 * NULL = 1: the plain convolution's bias gradient).  gr or db may be NULL (not both); gr needs r; ws is needed with db. */
int slr_conv_grad_scale_bias(const float *g, const float *r, const float *um, float *gr, float *db, int N, int C, int H, int W,
                             int layout, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ trainable decoder block (ABI 16; csrc/block_grad.hip)
 * What ResNet_Block_Pconv2 (models/layers/blocks.py:218-248) needs in training mode beyond its 3x3 convolutions: the partial batch-norm
 * with noise-conditioned gain and bias (models/layers/normalization.py:19-52, 256-354) forward and backward, the weight gradient of the
 * 1x1 skip convolution, and the adjoints of the two resampling stages.  b8 = 1: the [N,C,H,W] tensors are channel-blocked, [N,C/8,H,W,8]
 * (C % 8 == 0, 16-byte aligned); masks are [N,1,H,W] (or NULL), tables [N,C] or [C] plain.  N * C <= 65535, N * C * H * W < 2^31 - 1024.  None
 * synchronises, none uses atomics: every sum is taken in double in a fixed order, the same inputs give the same bits. */

/* Workspace of slr_bn_batch_stats and slr_bn_relu_mask_backward in bytes (256-byte aligned, else SLR_E_WORKSPACE); 0 for sizes they refuse. */
size_t slr_bn_train_ws_bytes(int N, int C, int H, int W);

/* Batch statistics (normalization.py:319-335): per channel sum x and sum x^2 over ALL N H W elements, divided by
 * count = N H W (mask NULL: manual_bn) or sum(mask) + eps (mask [N,1,H,W]: partial_manual_bn);
 * mean[C] = sum x / count, var[C] = sum x^2 / count - mean^2, formed from the double sums and rounded once; count[1]. */
int slr_bn_batch_stats(const float *x, const float *mask, float eps, float *mean, float *var, float *count,
                       int N, int C, int H, int W, int b8, void *ws, size_t ws_bytes, void *stream);

/* scale[n,c] = rsqrt(var[c] + eps) * gain[n,c], shift[n,c] = mean[c] * scale[n,c] - bias[n,c] (normalization.py:342-354), one fp32
 * rounding per operation; gain / bias [N,C] or NULL (1 / 0). */
int slr_bn_train_tables(const float *mean, const float *var, const float *gain, const float *bias, float eps,
                        float *scale, float *shift, int N, int C, void *stream);

/* a = relu(x * scale[n,c] - shift[n,c]) * mask (blocks.py:225-231 with partialconv2d.py:69), bit-equal to that fp32 expression,
 * torch.relu's NaN included (a NaN pre-activation gives NaN, not 0); mask [N,1,H,W] or NULL (no mask).  slr_bn_relu_mask is the per-channel-table form of the inference path. */
int slr_bn_relu_mask_train(const float *x, const float *scale, const float *shift, const float *mask, float *a,
                           int N, int C, int H, int W, int b8, void *stream);

/* Backward of the two calls above for the gradient ga at a.  gy = ga * mask * [not x * scale - shift <= 0] (the gate is recomputed from x and closes
 * on `<= 0` only, as torch's ReLU backward: a NaN pre-activation passes the gradient on);
 * s0[n,c] = sum gy, s1[n,c] = sum gy * x;  dbias = s0, dgain = rs (s1 - m s0) with rs = (var + eps)^-1/2, both [N,C];
 * dx = gy * scale + A + B (x - m) + addend, A = -rs P / count, B = -rs^3 (Q - m P) / count, P = sum_n gain s0, Q = sum_n gain s1
 * (the gradient through mean and var = m2 - m^2 of slr_bn_batch_stats).  stored = 1: mean / var are stored statistics, A = B = 0 and
 * `count` is not read.  addend [N,C,H,W] in x's layout or NULL; dx, dgain, dbias may each be NULL (not all); gain NULL = 1.
 * ws is needed unless stored = 1 and dgain = dbias = NULL. */
int slr_bn_relu_mask_backward(const float *x, const float *ga, const float *mask, const float *scale, const float *shift,
                              const float *mean, const float *var, const float *gain, const float *count, float eps,
                              const float *addend, float *dx, float *dgain, float *dbias, int stored,
                              int N, int C, int H, int W, int b8, void *ws, size_t ws_bytes, void *stream);

/* Weight gradient of out = conv1x1(x, w): dw[co][ci] = sum_{n,p} g[n,co,p] * x[n,ci,p], plain [Cout,Cin]; any Cin, Cout, H, W >= 1.
 * fp32 products and sums on v_mfma_f32_32x32x2_f32 inside a slab of pixels, the S slabs added in double in slab order.  splits: 0 = the
 * library's choice min(ceil(256 / channel tiles), chunks, 8 MiB / (4 Cout Cin)) with chunks = N * ceil(H W / 32) and channel tiles =
 * ceil(Cin / 64) * ceil(Cout / 128) (csrc/slr_tuning.hpp), > 0 = that many (at most one per chunk, at most 65535).
 * layout: SLR_GRAD_X_B8 | SLR_GRAD_G_B8.  ws: al256(S * Cout * Cin * 4) bytes, 256-byte aligned.  The bias gradient is
 * slr_conv_grad_scale_bias; the gradient to x is slr_conv1x1_forward with the transposed weight (SLR_CONV_F32). */
size_t slr_conv1x1_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int splits);
int slr_conv1x1_weight_grad(const float *x, const float *g, float *dw, int N, int Cin, int Cout, int H, int W,
                            int splits, int layout, void *ws, size_t ws_bytes, void *stream);

/* The exact adjoints of slr_avgpool3x3s2 and slr_upsample_bilinear2x in gather form: g is the gradient at the resampled tensor
 * ([N,C,(H-1)/2+1,(W-1)/2+1] / [N,C,2H,2W]), gin [N,C,H,W] the gradient at its input; every element of gin sums its own (at most 2 x 2 /
 * 4 x 4) contributions in a fixed order, the border clamping of align_corners = False folded into the weights. */
int slr_avgpool3x3s2_backward(const float *g, float *gin, int N, int C, int H, int W, int b8, void *stream);
int slr_upsample_bilinear2x_backward(const float *g, float *gin, int N, int C, int H, int W, int b8, void *stream);

/* ------------------------------------------------------------------ the decoder's first block, trainable (ABI 17; csrc/decoder_grad.hip)
 * ResNetDecoderPconv2 calls its first ResNet_Block_Pconv2 with the per-element mask (x != 0).float() [N,C,H,W]
 * (models/networks/architectures.py:369).  The entry points below are that block's batch-norm and the epilogue of its first partial
 * convolution with k = [x != 0] recomputed from x wherever it is needed: the mask is never a tensor.  From the update mask of that
 * convolution on, the mask is channel-uniform and the ABI 16 entry points apply.  Layouts, size limits (N * C <= 65535,
 * N * C * H * W < 2^31 - 1024) and rules as there: no atomics, every sum in double in a fixed order, nothing synchronises.  The two
 * reduction passes take 8 items per thread before their one workgroup sum. */

/* Workspace of the statistics and the backward below in bytes (256-byte aligned, else SLR_E_WORKSPACE); 0 for sizes they refuse. */
size_t slr_bn_nonzero_ws_bytes(int N, int C, int H, int W);

/* Batch statistics of partial_manual_bn with a [N,C,H,W] mask (models/layers/normalization.py:319-335): per channel
 * count[c] = #{x != 0} + eps (the number is an integer sum, eps is added in double), mean[c] = sum x / count[c],
 * var[c] = sum x^2 / count[c] - mean^2; the sums over ALL elements equal those over the kept ones.  mean, var, count: [C]. */
int slr_bn_nonzero_stats(const float *x, float eps, float *mean, float *var, float *count,
                         int N, int C, int H, int W, int b8, void *ws, size_t ws_bytes, void *stream);

/* msum [N,1,H,W] = sum_c [x != 0]: all a partial convolution needs of the per-element mask (models/layers/partialconv2d.py:61-67,
 * conv2d(mask, ones) = box3x3(msum)).  Exact integers in fp32; msum is plain in either layout of x. */
int slr_nonzero_count_plane(const float *x, float *msum, int N, int C, int H, int W, int b8, void *stream);

/* a = relu(x * scale[n,c] - shift[n,c]) * [x != 0] (models/layers/blocks.py:225-231 with partialconv2d.py:69; torch.relu: NaN stays NaN), bit-equal to that fp32
 * expression; scale, shift [N,C] from slr_bn_train_tables. */
int slr_bn_relu_nonzero_train(const float *x, const float *scale, const float *shift, float *a,
                              int N, int C, int H, int W, int b8, void *stream);

/* Backward of the calls above: slr_bn_relu_mask_backward with gy = ga * [x != 0] * [not x * scale - shift <= 0] (torch's ReLU backward: a
 * NaN pre-activation leaves the gate open) and the per-channel
 * count [C] of slr_bn_nonzero_stats.  The term A + B (x - m) of dx reaches the zero elements too, as the reference's autograd gives it.
 * NULL outputs, `stored`, addend, gain and ws as there (ws: slr_bn_nonzero_ws_bytes). */
int slr_bn_relu_nonzero_backward(const float *x, const float *ga, const float *scale, const float *shift,
                                 const float *mean, const float *var, const float *gain, const float *count, float eps,
                                 const float *addend, float *dx, float *dgain, float *dbias, int stored,
                                 int N, int C, int H, int W, int b8, void *ws, size_t ws_bytes, void *stream);

/* The epilogue of a partial convolution whose factors are given as planes (partialconv2d.py:72-74, blocks.py:248):
 * out = (raw0 * ratio + bias[c]) * um (+ residual), fp32 in that order; ratio, um [N,1,H,W] plain, bias [C], raw0 / residual / out
 * [N,C,H,W] in one layout (b8); residual may be NULL, out may be raw0.  For the first block ratio = 9 Cin / (box3x3(msum) + 1e-8) * um,
 * um = clamp(box3x3(msum), 0, 1) around a bias-free slr_conv3x3_forward. */
int slr_pconv_train_epilogue(const float *raw0, const float *ratio, const float *um, const float *bias, const float *residual,
                             float *out, int N, int C, int H, int W, int b8, void *stream);

/* ------------------------------------------------------------------ adversarial loss: the PatchGAN discriminator (ABI 18; csrc/disc.hip, csrc/conv4x4.hip)
 * What the reference's trainer (models/base_model.py:15-30, 118-151, --discriminator_losses pix2pixHD --norm_D spectralinstance) runs
 * through models/networks/discriminators.py:78-139 (NLayerDiscriminator) in both directions.  Everything is NCHW fp32.  None of the
 * entry points synchronises, none uses atomics: every long sum runs in a fixed order in double, the same inputs (and the same split
 * count) give the same bits.  H, W are the sizes of the convolution's INPUT everywhere; its output is OH = H / stride + 1,
 * OW = W / stride + 1 (kernel 4, padding 2).  Limits: stride 1 or 2, N < 65536, channels < 65536, N * H * W and N * OH * OW < 2^31. */

/* Bytes of a prepared weight buffer: ceil(Cout / 32) * Cin * 2048 for the forward, ceil(Cin / 32) * Cout * 2048 for backward != 0;
 * 0 for sizes the calls refuse. */
size_t slr_conv4x4_weight_bytes(int Cout, int Cin, int backward);

/* w [Cout,Cin,4,4] (nn.Conv2d's layout) -> MFMA fragments, each weight multiplied by scale[0] if `scale` (a DEVICE scalar: the 1 / sigma
 * of torch.nn.utils.spectral_norm, normalization.py:105-106) is not NULL.  backward = 0: the order slr_conv4x4_forward reads;
 * backward != 0: the order slr_conv4x4_backward_data reads for this `stride` (the forward's order does not depend on it). */
int slr_conv4x4_f32_weights(const float *w, const float *scale, void *wfrag, int Cout, int Cin, int stride, int backward, void *stream);

/* nn.Conv2d(Cin, Cout, kernel_size=4, stride, padding=2) (discriminators.py:92, 104-110, 116): in [N,Cin,H,W] -> out [N,Cout,OH,OW],
 * bias [Cout] or NULL, leaky != 0: nn.LeakyReLU(slope) of the result (discriminators.py:93).  Any Cin, Cout, H, W >= 1.  An implicit
 * GEMM on v_mfma_f32_32x32x2_f32: fp32 operands, products and accumulation. */
int slr_conv4x4_forward(const float *in, const void *wfrag, const float *bias, float *out, int N, int Cin, int Cout, int H, int W,
                        int stride, int leaky, float slope, void *stream);

/* The gradient to the input of the convolution above (what autograd's backward of F.conv2d returns for its input):
 *   gin[n,ci,iy,ix] = sum_co sum_{ky,kx} g'[n,co,(iy+2-ky)/stride,(ix+2-kx)/stride] * w[co,ci,ky,kx] over the taps whose division is
 * exact and in range, a gather: every element of gin [N,Cin,H,W] is stored once.  g [N,Cout,OH,OW]; g' = g, or with gate [N,Cout,OH,OW]
 * (the LeakyReLU'd output of the forward) g' = g * (gate > 0 ? 1 : slope).  wfrag: prepared with backward = 1 and this stride. */
int slr_conv4x4_backward_data(const float *g, const float *gate, const void *wfrag, float *gin, int N, int Cin, int Cout, int H, int W,
                              int stride, float slope, void *stream);

/* Workspace of slr_conv4x4_weight_grad in bytes: al256(S * 16 * Cout * Cin * 4), the partial sums of S slabs.  S = min(splits, chunks,
 * 65535) for splits > 0; for splits = 0 the library's choice min(ceil(512 / channel tiles), chunks, 32 MiB / (64 Cout Cin)) (at least 1)
 * with chunks = N * OH * ceil(OW / 32) and channel tiles = ceil(Cin / 32) * ceil(Cout / 32) (csrc/slr_tuning.hpp).  0 for sizes the
 * call refuses. */
size_t slr_conv4x4_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int stride, int splits);

/* Weight and bias gradient of the convolution above: dw[co][ci][ky][kx] = sum_{n,oy,ox} g'[n,co,oy,ox] * x[n,ci,s*oy+ky-2,s*ox+kx-2]
 * (zero padding), plain [Cout,Cin,4,4]; db[co] = sum g' (NULL: not wanted).  x [N,Cin,H,W], g and gate as in slr_conv4x4_backward_data.
 * fp32 products and sums on v_mfma_f32_32x32x2_f32 inside a slab of pixels, the slabs added in double in slab order; db in double
 * throughout.  ws: 256-byte aligned, slr_conv4x4_grad_ws_bytes bytes, else SLR_E_WORKSPACE. */
int slr_conv4x4_weight_grad(const float *x, const float *g, const float *gate, float *dw, float *db, int N, int Cin, int Cout, int H, int W,
                            int stride, float slope, int splits, void *ws, size_t ws_bytes, void *stream);

/* nn.InstanceNorm2d(C, affine=False) + nn.LeakyReLU(slope) (normalization.py:121-128, discriminators.py:112): per (n, c) plane
 * m = mean(x), rstd = 1 / sqrt(mean((x - m)^2) + eps), y = leaky((x - m) * rstd); mean, rstd [N*C] are kept for the backward.  Planes
 * of at least 4 elements; the sums in double.  One workgroup per plane. */
int slr_instnorm_lrelu_forward(const float *x, float *y, float *mean, float *rstd, int N, int C, int H, int W, float eps, float slope,
                               void *stream);

/* Its backward: xh = (x - m) * rstd, gh = gy * (xh > 0 ? 1 : slope), gx = rstd * (gh - mean(gh) - xh * mean(gh * xh)). */
int slr_instnorm_lrelu_backward(const float *x, const float *gy, const float *mean, const float *rstd, float *gx, int N, int C, int H,
                                int W, float slope, void *stream);

/* ------------------------------------------------------------------ optimiser step: multi-tensor Adam (ABI 19; csrc/adam.hip)
 * torch.optim.Adam(params, lr, betas, eps) with no weight decay and no amsgrad -- the two optimisers of the reference's trainer
 * (models/base_model.py:21-37) -- over any number of fp32 tensors in at most two launches.  A PLAN in device memory describes the
 * tensors; it is built on the host (the two entry points below touch no device) and uploaded by the caller with one copy.
 *
 * Plan layout (little endian; offsets in bytes from the plan's start, which is 16-byte aligned):
 *   header, 64 bytes:   uint32 magic = SLR_ADAM_PLAN_MAGIC, uint32 chunk = SLR_ADAM_CHUNK, uint32 n_tensors, uint32 n_work,
 *                       uint64 tensors_off = 64, uint64 work_off, uint64 scratch_off, uint64 bytes, 16 bytes of zeros
 *   tensors_off:        n_tensors records of 48 bytes: uint64 p, g, m, v, step (device addresses; step: the tensor's fp32 step counter),
 *                       int64 numel
 *   work_off:           n_work records of 16 bytes: int32 tensor, int32 count, int64 start -- elements [start, start + count) of that
 *                       tensor, start a multiple of SLR_ADAM_CHUNK, 1 <= count <= SLR_ADAM_CHUNK; the records of a tensor follow each
 *                       other in order of start and cover [0, numel) exactly once; a tensor with numel = 0 has none
 *   scratch_off:        n_tensors pairs of fp32, written by every step: 1 - beta1^step and sqrt(1 - beta2^step)
 *   work_off = align16(64 + 48 n_tensors), scratch_off = align16(work_off + 16 n_work), bytes = align256(scratch_off + 8 n_tensors).
 * The update kernel takes one work item per workgroup and loop trip: the plan is data, never kernel arguments, so n_tensors has no limit. */
#define SLR_ADAM_CHUNK      4096
#define SLR_ADAM_PLAN_MAGIC 0x4d414441u   /* "ADAM" */
#define SLR_ADAM_ZERO_GRADS 1             /* flags bit 0: write zeros to g after reading it (zero_grad with fixed gradient pointers) */

/* Bytes of the plan of n tensors with numel[t] elements (host arithmetic only); 0 for n <= 0, a negative numel or 2^31 work items. */
size_t slr_adam_plan_bytes(int n, const long long *numel);

/* Writes the plan into CALLER memory `host_buf` of `bytes` >= slr_adam_plan_bytes(n, numel) bytes (host only; nothing touches a device).
 * p, g, m, v, step: n device addresses each, as integers, 4-byte aligned; numel[t] = 0 is legal and costs nothing (its step still
 * advances).  The header's n_work is the value slr_adam_step wants. */
int slr_adam_plan_fill(void *host_buf, size_t bytes, int n, const unsigned long long *p, const unsigned long long *g,
                       const unsigned long long *m, const unsigned long long *v, const unsigned long long *step, const long long *numel);

/* One Adam step of every tensor of the plan (a copy of a filled plan in device memory, 16-byte aligned), in torch's arithmetic and order,
 * fp32 with single roundings:
 *     step += 1;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),  bc = 1 - beta^step
 * Launch (a), one workgroup: per tensor the step counter and the two corrections, evaluated in double, into the plan's scratch table.
 * Launch (b): the update -- 16-byte accesses of all four streams where a tensor's four pointers are 16-byte aligned, scalar ones
 * otherwise; a capped grid strides over the work items; no atomics; every element is read and written by exactly one thread, so the bits
 * depend neither on the grid nor on how tensors are grouped into plans.
 *   lr_dev   a DEVICE fp32 scalar: a new learning rate needs no new plan and cannot break a captured graph
 *   betas    HOST, two doubles (beta1, beta2), each in [0, 1): read before the call returns.  Doubles because 1 - beta is: the fp32
 *            nearest to 0.999 is 0.99900001287, and 1 - that is off by 1.3e-5 of itself -- in v and in the second correction alike
 *   eps      > 0
 *   flags    SLR_ADAM_ZERO_GRADS or 0; any other bit is refused
 * Argument errors return SLR_E_BADARG before anything is launched. */
int slr_adam_step(void *plan_dev, int n_tensors, int n_work, const float *lr_dev, const double *betas, float eps, int flags, void *stream);

/* ------------------------------------------------------------------ spectral normalisation of the generator (ABI 20; csrc/spectral.hip, csrc/conv.hip)
 * torch.nn.utils.spectral_norm as the reference wraps it around every 3x3, partial 3x3 and 1x1 convolution of the generator
 * (models/layers/blocks.py:5-35, models/networks/architectures.py:18-66) and around the bias-free nn.Linear maps of the noise layers
 * (models/layers/normalization.py:6-16) under --norm_G sync:spectral_batch, the option of every training script it ships: the parameter is
 * weight_orig, the buffers weight_u / weight_v, the effective weight weight_orig / sigma.  None of the entry points synchronises, none uses
 * atomics; every long sum is accumulated in double in an order the matrix's own shape fixes: the same bits from run to run and whatever
 * else is in the list.
 *
 * Plan of slr_spectral_sigma (little endian; offsets in bytes from the plan's start, which is 16-byte aligned):
 *   header, 64 bytes:   uint32 magic = SLR_SPECTRAL_PLAN_MAGIC, uint32 max_dim = SLR_SPECTRAL_MAX_DIM, uint32 n_tensors, uint32 n_work,
 *                       uint64 tensors_off = 64, uint64 bytes, uint64 total_u (sum of rows), uint64 total_v (sum of cols),
 *                       uint64 work_off, uint64 scratch_off
 *   tensors_off:        n_tensors records of 64 bytes: uint64 w, u, v (device addresses), int32 rows, int32 cols, int32 slot (= the
 *                       record's index: its element of inv_sigma), int32 bands, int64 u_off, int64 v_off (elements into the saved
 *                       arrays: the running sums of rows / cols), int64 scratch (bytes from the plan's start; 0 where bands = 0)
 *   work_off:           n_work records of 8 bytes: int32 tensor, int32 band -- one per band of every banded matrix, in order
 *   scratch_off:        per banded matrix align256(8 (bands cols + rows)) bytes, written by every call: the bands' partial W^T u
 *                       [bands][cols] and W v [rows] in double
 *   A matrix is BANDED when rows cols >= SLR_SPECTRAL_SPLIT_ELEMENTS and rows >= 2 SLR_SPECTRAL_BAND_ROWS: bands =
 *   ceil(rows / SLR_SPECTRAL_BAND_ROWS), band b holds rows [b, b + 1) SLR_SPECTRAL_BAND_ROWS; bands = 0 otherwise.
 *   work_off = align16(64 + 64 n_tensors), scratch_off = align256(work_off + 8 n_work), bytes = align256(scratch_off + scratch).
 * The plan is data, never kernel arguments, so n_tensors has no limit.  The scratch belongs to the plan: calls that share a plan run
 * on one stream. */
#define SLR_SPECTRAL_PLAN_MAGIC 0x43455053u   /* "SPEC" */
#define SLR_SPECTRAL_MAX_DIM    3072          /* rows and cols of one matrix (the generator's largest: 256 x 2304) */
#define SLR_SPECTRAL_GRAD_CHUNK 4096          /* elements per workgroup of slr_spectral_weight_grad */
#define SLR_SPECTRAL_BAND_ROWS  16            /* rows per band of a banded matrix */
#define SLR_SPECTRAL_SPLIT_ELEMENTS 32768     /* matrices of at least this many elements are banded */

/* Bytes of the plan of n matrices of rows[t] x cols[t] (host arithmetic only); 0 for n <= 0 or a size outside 1 .. SLR_SPECTRAL_MAX_DIM. */
size_t slr_spectral_plan_bytes(int n, const int *rows, const int *cols);

/* Writes the plan into CALLER memory `host_buf` of `bytes` >= slr_spectral_plan_bytes(n, rows, cols) bytes (host only; nothing touches a device).
 * w, u, v: n device addresses each, as integers, 4-byte aligned (16-byte alignment of w is used where it is there): w [rows, cols] is
 * weight_orig viewed as [Cout, Cin k k] (spectral_norm's weight_mat, dim 0) or the [C, noise_sz] weight of a linear; u [rows], v [cols]. */
int slr_spectral_plan_fill(void *host_buf, size_t bytes, int n, const unsigned long long *w, const unsigned long long *u,
                           const unsigned long long *v, const int *rows, const int *cols);

/* SpectralNorm.compute_weight (torch/nn/utils/spectral_norm.py, n_power_iterations = 1, eps = 1e-12) of every matrix of the plan (a copy
 * of a filled plan in device memory; n_work: the header's), a workgroup per matrix in one launch, preceded by two launches (one in eval
 * mode) over the bands of the banded matrices where there are any -- at most three launches, whatever the list:
 *   training != 0:  v <- W^T u / max(|W^T u|, eps);  u <- W v / max(|W v|, eps), written in place into the buffers;
 *   training == 0:  u and v are read only;
 *   both:           inv_sigma[slot] = 1 / (u^T W v);  saved_u [total_u] and saved_v [total_v] receive copies of u and v at u_off / v_off:
 *                   the constants the backward of THIS forward needs (slr_spectral_weight_grad) -- per call, not per module.
 * Banded matrices: every band's partial W^T u over its rows in order, the partials added in band order, W v per row as elsewhere: the
 * order of every sum is fixed by (rows, cols) alone.  A zero matrix gives a non-finite inv_sigma, as torch does. */
int slr_spectral_sigma(void *plan_dev, int n_tensors, int n_work, float *inv_sigma, float *saved_u, float *saved_v, int training, void *stream);

/* slr_conv3x3_f32_weights / slr_conv1x1_f32_weights of w * scale[0] (scale: a DEVICE scalar, the inv_sigma above; one fp32 product per
 * weight), w [Cout,Cin,k,k] = weight_orig.  backward = 0: the buffer of the forward convolution (slr_conv*_weight_bytes(Cout, Cin) bytes),
 * bit-equal to the unscaled entry applied to w * scale.  backward != 0: the buffer of the backward-data convolution, Cout -> Cin channels
 * (slr_conv*_weight_bytes(Cin, Cout) bytes), read straight from weight_orig: bit-equal to the unscaled entry applied to
 * (w * scale).flip(2, 3).transpose(0, 1).contiguous(). */
int slr_conv3x3_f32_weights_scaled(const float *w, const float *scale, void *wfrag, int Cout, int Cin, int backward, void *stream);
int slr_conv1x1_f32_weights_scaled(const float *w, const float *scale, void *wfrag, int Cout, int Cin, int backward, void *stream);

/* The same for every convolution of a network in ONE launch, from a plan in device memory:
 *   header, 64 bytes:   uint32 magic = SLR_CONV_PREP_PLAN_MAGIC, uint32 chunk = SLR_CONV_PREP_CHUNK, uint32 n_tensors, uint32 n_work,
 *                       uint64 tensors_off = 64, uint64 work_off, uint64 bytes, 24 bytes of zeros
 *   tensors_off:        n_tensors records of 48 bytes: uint64 w, uint64 wfrag, int32 slot (the element of `scales` that multiplies it),
 *                       int32 Cout', Cin' (of the convolution the buffer serves: swapped for backward), int32 Cin' padded to 16,
 *                       int32 taps (9 or 1), int32 backward, int32 few (the plain layout of 3x3 layers with Cout' <= 4), int32 elements
 *   work_off:           n_work records of 8 bytes: int32 tensor, int32 start -- buffer elements [start, start + chunk) of that tensor
 *   work_off = align16(64 + 48 n_tensors), bytes = align256(work_off + 8 n_work).
 * cout, cin, taps, backward: n ints each, cout / cin the shape of weight_orig as in the single-tensor entries. */
#define SLR_CONV_PREP_PLAN_MAGIC 0x50455250u   /* "PREP" */
#define SLR_CONV_PREP_CHUNK      4096
size_t slr_conv_prep_plan_bytes(int n, const int *cout, const int *cin, const int *taps, const int *backward);
int slr_conv_prep_plan_fill(void *host_buf, size_t bytes, int n, const unsigned long long *w, const unsigned long long *wfrag,
                            const int *slot, const int *cout, const int *cin, const int *taps, const int *backward);
int slr_conv_prep_scaled_multi(const void *plan_dev, int n_tensors, int n_work, const float *scales, void *stream);

/* Workspace of slr_spectral_weight_grad in bytes: align256(8 * ceil(rows * cols / SLR_SPECTRAL_GRAD_CHUNK)); 0 for sizes it refuses. */
size_t slr_spectral_grad_ws_bytes(int rows, int cols);

/* The gradient to weight_orig that autograd returns through spectral_norm's weight = weight_orig / sigma, sigma = u^T W v with u and v
 * constants (spectral_norm.py: they are detached):
 *     out = (dw - <dw, W_eff> u v^T) * inv_sigma,   W_eff = w * inv_sigma
 * dw [rows, cols]: the gradient at the effective weight (what the weight-gradient kernels produce); w = weight_orig; u [rows], v [cols],
 * inv_sigma [1]: the saved values of that forward.  Two launches: partial sums of <dw, w> per chunk of SLR_SPECTRAL_GRAD_CHUNK elements
 * in double, then the update, every workgroup adding the partials in chunk order.  The same entry serves the [C, noise_sz] linears.
 * out may be dw.  ws: 16-byte aligned, slr_spectral_grad_ws_bytes bytes, else SLR_E_WORKSPACE. */
int slr_spectral_weight_grad(const float *dw, const float *w, const float *u, const float *v, const float *inv_sigma, float *out,
                             int rows, int cols, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ the same gradient for every tensor of a list (ABI 21; csrc/spectral.hip)
 * slr_spectral_weight_grad over ANY number of tensors in TWO launches: what a network's backward needs once for all its weight_orig,
 * instead of two launch-bound launches per tensor.  Built like slr_adam_step and slr_spectral_sigma: a plan in device memory, never
 * kernel arguments.  Work items are (tensor, chunk) pairs, chunk c of a tensor its elements [c, c + 1) SLR_SPECTRAL_GRAD_CHUNK.
 *
 * Plan (little endian; offsets in bytes from the plan's start, which is 16-byte aligned):
 *   header, 64 bytes:   uint32 magic = SLR_SPECTRAL_GRAD_PLAN_MAGIC, uint32 chunk = SLR_SPECTRAL_GRAD_CHUNK, uint32 n_tensors, uint32 n_work,
 *                       uint64 tensors_off = 64, uint64 bytes, uint64 work_off, uint64 scratch_off, 16 bytes of zeros
 *   tensors_off:        n_tensors records of 64 bytes: uint64 dw, w, out (device addresses), int32 rows, int32 cols, int32 slot (its
 *                       element of inv_sigma), int32 chunks = ceil(rows cols / chunk), int64 u_off, int64 v_off (elements into saved_u /
 *                       saved_v: where slr_spectral_sigma of that forward put its u and v), int64 first (its first work item: the running
 *                       sum of chunks; its partial sums are doubles [first, first + chunks) of the scratch)
 *   work_off:           n_work records of 8 bytes: int32 tensor, int32 chunk -- every tensor's chunks in order, the tensors in order
 *   scratch_off:        n_work doubles, one per work item, written by every call before it reads them
 *   work_off = align16(64 + 64 n_tensors), scratch_off = align256(work_off + 8 n_work), bytes = scratch_off + align256(8 n_work).
 * The scratch belongs to the plan: calls that share a plan run on one stream. */
#define SLR_SPECTRAL_GRAD_PLAN_MAGIC 0x44475053u   /* "SPGD" */

/* Bytes of the plan of n tensors of rows[t] x cols[t] (host arithmetic only); 0 for n <= 0 or a size outside 1 .. SLR_SPECTRAL_MAX_DIM. */
size_t slr_spectral_grad_plan_bytes(int n, const int *rows, const int *cols);

/* Writes the plan into CALLER memory `host_buf` of `bytes` >= slr_spectral_grad_plan_bytes(n, rows, cols) bytes (host only; nothing
 * touches a device).  dw, w, out: n device addresses each, as integers, 4-byte aligned; out[t] may be dw[t].  u_off, v_off, slot: where
 * tensor t's u, v and inv_sigma lie in the arrays of its forward (the layout slr_spectral_sigma wrote; any subset of that list, in any
 * order, is a legal list here).  SLR_E_BADARG for n <= 0, a null or misaligned address, a size outside 1 .. SLR_SPECTRAL_MAX_DIM, a
 * negative offset or slot, or too few bytes. */
int slr_spectral_grad_plan_fill(void *host_buf, size_t bytes, int n, const unsigned long long *dw, const unsigned long long *w,
                                const unsigned long long *out, const int *rows, const int *cols, const long long *u_off,
                                const long long *v_off, const int *slot);

/* out_t = (dw_t - <dw_t, w_t inv_sigma_t> u_t v_t^T) inv_sigma_t for every tensor of the plan (a copy of a filled plan in device memory;
 * n_tensors, n_work: the header's).  Launch 1: a workgroup per work item writes its chunk's sum of dw w, in double, into the scratch.
 * Launch 2: a workgroup per work item adds its own tensor's partials in chunk order and writes its chunk of out.  Per tensor the
 * chunking, the order of every sum and the arithmetic are slr_spectral_weight_grad's: the result is BIT-EQUAL to it, alone or in any
 * list.  No atomics, nothing synchronises. */
int slr_spectral_weight_grad_multi(void *plan_dev, int n_tensors, int n_work, const float *inv_sigma, const float *saved_u,
                                   const float *saved_v, void *stream);

/* ------------------------------------------------------------------ training the SPADE motion U-Net (ABI 23; csrc/motion_grad.hip, csrc/conv4x4.hip, csrc/disc.hip)
 * The backward of the motion U-Nets' kernels above and the motion losses (models/losses/synthesis.py:11-58, 142-160), as the reference's
 * train_motion_unet.py needs them.  All tensors NCHW fp32; nothing synchronises; no atomics: every long sum is accumulated in double in a
 * fixed order, the same bits from run to run. */

/* The encoder convolution Conv2d(Cin, Cout, 4, stride 2, padding 1) with leaky_relu(., slope) of its input (slr_conv4x4s2_forward).
 * Forward in training: slr_conv4x4s2_forward on the fragments of slr_conv4x4_f32_weights(w, scale, ., Cout, Cin, 2, 0) (the layout of
 * slr_conv4x4s2_f32_weights, every weight times the device scalar `scale`).
 *
 * slr_conv4x4s2_backward_data: gin [N,Cin,H,W] from g [N,Cout,(H-2)/2+1,(W-2)/2+1] as a gather, every element stored once.  Pixel
 * (2a + py, 2b + px) gets the taps ky = (1 - py) + 2 ty, kx = (1 - px) + 2 tx reading g[a + py - ty][b + px - tx]: the taps of parity
 * class (1 - py, 1 - px) of the padding-2 convolution, so `wfrag` is what slr_conv4x4_f32_weights(w, scale, ., Cout, Cin, 2, 1) prepares
 * (slr_conv4x4_weight_bytes(Cout, Cin, 1) bytes) and the kernel reads it with the class bits flipped.  xin: the convolution's RAW input
 * [N,Cin,H,W] when the layer has the LeakyReLU in front (the result is multiplied by xin > 0 ? 1 : slope), NULL when it has none (conv1).
 * H, W >= 2, odd sizes included. */
int slr_conv4x4s2_backward_data(const float *g, const float *xin, const void *wfrag, float *gin, int N, int Cin, int Cout, int H, int W,
                                float slope, void *stream);

/* dw[co][ci][ky][kx] = sum over (n, oy, ox) of g[n,co,oy,ox] * pre(x)[n,ci,2oy+ky-1,2ox+kx-1] (zero outside), pre = leaky_relu(., slope)
 * when `leaky`, applied while staging; db[co] = sum of g in double (db NULL: not computed).  The slab scheme of slr_conv4x4_weight_grad:
 * `splits` slabs of output pixels (0: chosen by the library), partial sums per slab in ws, a second launch adds them in double in slab
 * order.  ws: 256-byte aligned, slr_conv4x4s2_grad_ws_bytes bytes (0 for sizes it refuses), else SLR_E_WORKSPACE. */
size_t slr_conv4x4s2_grad_ws_bytes(int N, int Cin, int Cout, int H, int W, int splits);
int slr_conv4x4s2_weight_grad(const float *x, const float *g, float *dw, float *db, int N, int Cin, int Cout, int H, int W, int leaky,
                              float slope, int splits, void *ws, size_t ws_bytes, void *stream);

/* slr_instnorm_spade that also keeps mean and rstd [N*C] of every plane for the backward: the same kernel code, so `out` is BIT-EQUAL to
 * slr_instnorm_spade's (an eval() forward of the trainable network is the inference network's).  Planes of at least 2 x 2. */
int slr_instnorm_spade_train_forward(const float *x, const float *gamma_beta, float *out, float *mean, float *rstd, int N, int C, int H,
                                     int W, float eps, void *stream);

/* From g = d out, with xh = (x - mean) rstd:  d beta = g,  d gamma = g xh,  gh = g (1 + gamma),
 *   gx = rstd (gh - mean(gh) - xh mean(gh xh)),  the two means per plane from double sums;
 * dgamma_beta [N,2C,H,W] = d gamma | d beta in gamma_beta's layout.  One workgroup per (n, c) plane. */
int slr_instnorm_spade_backward(const float *x, const float *gamma_beta, const float *g, const float *mean, const float *rstd, float *gx,
                                float *dgamma_beta, int N, int C, int H, int W, void *stream);

/* The gradient of slr_upsample2x_concat: g [N,Ca+Cb,2H,2W] -> ga [N,Ca,H,W], gb [N,Cb,H,W] (Cb = 0: b, gb unused).  Every source pixel
 * sums the <= 4 x 4 output pixels it feeds with the bilinear weights .25 / .75 and the edge clamping folded in (channel `nearest_channel`
 * of each source: its 2 x 2 block).  relu = 1: the sum is gated by the source, a / b > 0 (a, b required); relu = 2: every g is gated by
 * fwd > 0, fwd [N,Ca+Cb,2H,2W] the forward's result (required); relu'(0) = 0 as in torch.  relu = 0: a, b and fwd may be NULL. */
int slr_upsample2x_concat_backward(const float *g, const float *fwd, const float *a, int Ca, const float *b, int Cb, float *ga, float *gb,
                                   int N, int H, int W, int nearest_channel, int relu, void *stream);

/* The motion losses in one pass over pred, gt [N,2,H,W], d = pred - gt:  sums [N][3] (DOUBLE, device) per image =
 *   sum |d|_2  (EndPointError = its total / (N H W)),  sum |d_0| + |d_1|  (MotionL1 = total / (2 N H W)),  sum |d|_2^2  (PSNR's mse_err =
 *   per image / (H W)).  Workgroups of 4096 pixels write partial sums to ws, a second launch adds them in order.
 * ws: 256-byte aligned, slr_motion_loss_ws_bytes bytes (0 for sizes it refuses), else SLR_E_WORKSPACE. */
size_t slr_motion_loss_ws_bytes(int N, int H, int W);
int slr_motion_loss(const float *pred, const float *gt, double *sums, int N, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* gpred [N,2,H,W] = w_epe[0] d / |d|_2 / (N H W)  (exactly 0 where |d|_2 = 0: torch's norm backward)  +  w_l1[0] sign(d) / (2 N H W);
 * w_epe, w_l1: DEVICE scalars (the gradients reaching the two means), either may be NULL (that term is absent). */
int slr_motion_loss_grad(const float *pred, const float *gt, const float *w_epe, const float *w_l1, float *gpred, int N, int H, int W,
                         void *stream);

/* ------------------------------------------------------------------ the head of the two-layer model (ABI 24; csrc/layers.hip)
 * What models/animating_softmax_splating_2layers_alpha_seperate.py computes between its networks' raw outputs and its loss dictionary.
 * All planes contiguous NCHW fp32.  Nothing synchronises; no atomics: every sum is a per-workgroup partial sum in double, added by a
 * second launch in a fixed order, the same bits from run to run.  Per element every operation is the fp32 one torch does, products with
 * masks included (0 * NaN = NaN); sign(0) = sign(NaN) = 0 (torch.sign).  16-byte accesses where H W (the composite) or W (the losses) is
 * a multiple of 4 and every tensor is 16-byte aligned, scalar accesses elsewhere. */

/* fluid_raw, bg_raw [N,3,H,W], fluid_alpha_raw, bg_alpha_raw [N,1,H,W] ->
 *   fluid = tanh(fluid_raw), bg = tanh(bg_raw)   (:598, :372)
 *   af = sigmoid(fluid_alpha_raw), ab = sigmoid(bg_alpha_raw), n = max(af + ab, 1e-8)   (:608, :616-617; a NaN sum stays NaN)
 *   pred = (af fluid + ab bg) / n  [N,3,H,W]   (:652),   composite_alpha = af / n  [N,1,H,W]   (:775, :789). */
int slr_layer_composite_forward(const float *fluid_raw, const float *bg_raw, const float *fluid_alpha_raw, const float *bg_alpha_raw,
                                float *pred, float *fluid, float *bg, float *composite_alpha, int N, int H, int W, void *stream);

/* The four input gradients in one pass from g_pred, g_fluid, g_bg [N,3,H,W], the gradients reaching pred, fluid and bg (each may be NULL:
 * absent).  The chain is autograd's: the gradient reaching n passes on to af and ab only where af + ab >= 1e-8 (where the clamp bites,
 * nothing flows through n).  Each output may be NULL (not wanted), not all four. */
int slr_layer_composite_backward(const float *fluid_raw, const float *bg_raw, const float *fluid_alpha_raw, const float *bg_alpha_raw,
                                 const float *g_pred, const float *g_fluid, const float *g_bg, float *d_fluid_raw, float *d_bg_raw,
                                 float *d_fluid_alpha_raw, float *d_bg_alpha_raw, int N, int H, int W, void *stream);

/* Workspace of slr_alpha_losses_forward in bytes (8-byte aligned, else SLR_E_WORKSPACE); 0 for sizes it refuses (H or W < 2). */
size_t slr_alpha_losses_ws_bytes(int N, int H, int W);

/* a_start [N,2,H,W] (channel 0 the background logit a0, channel 1 the fluid logit a1); mask_rock r, small_motion_alpha, warped_alpha,
 * norm, fluid_alpha_raw f [N,1,H,W].  With m = 1 - small_motion_alpha, sf = sigmoid(a1), sb = sigmoid(a0):
 *   c0 = sf / max(sf + sb, 1e-8)   (:420-421),   gt_alpha = 0.25 r m + (1 - r) m + 0.5 small_motion_alpha   (:619-621),   both [N,1,H,W]
 *   err = (c0 m - gt_alpha m)^2
 *   losses[0]  AlphaMSEloss: reweight != 0:  0.5 (sum r m err / (1 + sum r m) + sum (1 - r) m err / (1 + sum (1 - r) m))   (:660-666)
 *                            reweight == 0:  mean err   (:694-697)
 *   losses[1]  AlphaTV = TV(a1) + TV(sb), TV(x) = mean |x[..., :-1] - x[..., 1:]| + mean |x[..., :-1, :] - x[..., 1:, :]|   (:67-71, :728:
 *              the fluid plane as the raw logit, the background plane after its sigmoid)
 *   losses[2]  Alpha Decoder Consistency Loss = mean S(warped_alpha k - f k), k = norm > 1e-8, S(d) = |d| + 0.1 (2 sigmoid(5 |d|) - 1)
 *              (:63-65, :758-759)
 *   losses[3]  its moving-region form, mean S(.) m   (:763-764)
 *   losses[4], [5]  0.5 / (1 + sum r m) and 0.5 / (1 + sum (1 - r) m), which the backward reads;  losses[6], [7] = 0.
 * losses: 8 floats in device memory.  H, W >= 2. */
int slr_alpha_losses_forward(const float *a_start, const float *mask_rock, const float *small_motion_alpha, const float *warped_alpha,
                             const float *norm, const float *fluid_alpha_raw, float *losses, float *gt_alpha, float *c0, int reweight,
                             int N, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* d_a_start [N,2,H,W] and d_fluid_alpha_raw [N,1,H,W] (either may be NULL) from g_losses [4], the gradients reaching losses[0 .. 3]
 * (device), and `losses`, the forward's vector.  The TV term is a five-point stencil; warped_alpha receives no gradient. */
int slr_alpha_losses_backward(const float *a_start, const float *mask_rock, const float *small_motion_alpha, const float *warped_alpha,
                              const float *norm, const float *fluid_alpha_raw, const float *losses, const float *g_losses,
                              float *d_a_start, float *d_fluid_alpha_raw, int reweight, int N, int H, int W, void *stream);

/* ------------------------------------------------------------------ the alpha-0 blending weight (ABI 25; csrc/layers.hip)
 * train_alpha_finetuneBG_finetuneFluid_v1.sh (--use_alpha0_as_blending_weight): the alpha logit plane is splatted under exp(c0), c0 the
 * composite fluid alpha of the START image, so c0 carries a gradient; and two more loss terms on c0 (:741-755).  Conventions as above;
 * 16-byte accesses where H W is a multiple of 4 and every tensor is 16-byte aligned. */

/* Workspace of slr_blend_alpha0_forward in bytes (8-byte aligned, else SLR_E_WORKSPACE); 0 for sizes it refuses. */
size_t slr_blend_alpha0_ws_bytes(int N, int H, int W);

/* a_start [N,2,H,W] (channel 0 the background logit a0, channel 1 the fluid logit a1); mask_rock r, small_motion_alpha [N,1,H,W].
 * With m = 1 - small_motion_alpha, sf = sigmoid(a1), sb = sigmoid(a0), S(d) = |d| + 0.1 (2 sigmoid(5 |d|) - 1)   (:63-65):
 *   c0 = sf / max(sf + sb, 1e-8)  [N,1,H,W]   (:420-421)
 *   values[0]  FluidRegionLoss = mean S(c0 (1 - r) m - (1 - r) m)   (:742-744)
 *   values[1]  RockRegionLoss  = mean S(c0 r m - rock_target r m)   (:750-753)
 * values: 2 floats in device memory.  N, H, W >= 1. */
int slr_blend_alpha0_forward(const float *a_start, const float *mask_rock, const float *small_motion_alpha, float *c0, float *values,
                             float rock_target, int N, int H, int W, void *ws, size_t ws_bytes, void *stream);

/* d_a_start [N,2,H,W] in one pass from g_c0 [N,1,H,W], the gradient reaching c0, and g_values [2], the gradients reaching the two losses
 * (device); either may be NULL (absent), not both.  The sigmoids are recomputed.  The chain is autograd's: where sf + sb < 1e-8 nothing
 * flows through the clamped sum (the convention of slr_layer_composite_backward). */
int slr_blend_alpha0_backward(const float *a_start, const float *mask_rock, const float *small_motion_alpha, const float *g_c0,
                              const float *g_values, float *d_a_start, float rock_target, int N, int H, int W, void *stream);

/* ------------------------------------------------------------------ LPIPS of the clip evaluation (ABI 26; csrc/lpips.hip)
 * The reference's tables are LPIPS: evaluation/animation/eval_CLAW.py:24,37 calls lpips.LPIPS(net='alex', version='0.1') on every frame
 * pair.  Trunk and scaling constants: models/networks/pretrained_networks.py:45-46 and :154-196 (torchvision's alexnet.features cut
 * after each ReLU); the linear heads are those of the lpips package.  Everything here is fp32 (the convolutions on
 * v_mfma_f32_32x32x2_f32: fp32 operands, products and accumulation), deterministic (fixed order, no atomics), and a result depends on
 * its own image only.  The three 3x3 convolutions of the trunk run on slr_conv3x3_forward with SLR_CONV_F32. */

/* The input of the trunk (lpips' ScalingLayer = pretrained_networks.py:45-46, 73-74): out [N,3,H,W] NCHW = (x - shift) / scale, with
 * normalize = 1 ((2 x - 1) - shift) / scale (lpips' normalize=True: images in [0,1]).  img: float [N,3,H,W] (u8 = 0) or uint8 [N,H,W,3]
 * (u8 = 1; x = v / 255.0f first, in either mode). */
int slr_lpips_prep(const void *img, int u8, int normalize, float *out, int N, int H, int W, void *stream);

/* nn.Conv2d(Cin, Cout, K, stride, padding) + bias for (K, stride, padding) = (11, 4, 2) and (5, 1, 2): features.0 and features.3 of
 * torchvision's alexnet (pretrained_networks.py:161-166).  Weights w [Cout,Cin,K,K] are prepared once into fragment order
 * (slr_convkxk_f32_weights into slr_convkxk_weight_bytes(Cout, Cin, K) bytes; 0 for sizes it refuses).  in [N,Cin,H,W] NCHW
 * (in_b8 = 0) or channel-blocked [N,Cin/8,H,W,8] (in_b8 = 1, Cin % 8 == 0); out [N,Cout,OH,OW], O. = (. + 2 padding - K) / stride + 1,
 * channel-blocked [N,Cout/8,OH,OW,8], Cout % 8 == 0, RAW: the ReLU belongs to the consumer.  Any H, W >= 1 with OH, OW >= 1;
 * N H W < 2^31; channel-blocked tensors are 16-byte aligned. */
size_t slr_convkxk_weight_bytes(int Cout, int Cin, int K);
int slr_convkxk_f32_weights(const float *w, void *wfrag, int Cout, int Cin, int K, void *stream);
int slr_convkxk_forward(const float *in, const void *wfrag, const float *bias, float *out, int N, int Cin, int Cout, int H, int W, int K,
                        int stride, int pad, int in_b8, void *stream);

/* nn.ReLU + nn.MaxPool2d(3, stride 2) of torchvision's alexnet.features (floor mode, no padding: 179 x 319 -> 89 x 159):
 * in [N,C,H,W] -> out [N,C,(H-3)/2+1,(W-3)/2+1], both channel-blocked, C % 8 == 0, H, W >= 3, 16-byte aligned.  A window that holds a
 * NaN gives NaN, as slr_relu_maxpool2x2_b8 does. */
int slr_relu_maxpool3x3s2_b8(const float *in, float *out, int N, int C, int H, int W, void *stream);

/* One layer of LPIPS: with f = relu(raw features) and n(f) = f / (sqrt(sum_c f_c^2) + 1e-10),
 *   out[n] = mean_hw sum_c w[c] (n(f0)_c - n(f1)_c)^2        (lpips: normalize_tensor, NetLinLayer without bias, spatial_average)
 * f0, f1 [N,C,H,W] raw, channel-blocked (C % 8 == 0); w [C] (any sign), 16-byte aligned; out [N].  Two all-zero feature vectors at a
 * pixel contribute exactly 0; equal features give exactly 0.  ws: slr_lpips_distance_ws_bytes(N, H, W) bytes, 8-byte aligned. */
size_t slr_lpips_distance_ws_bytes(int N, int H, int W);
int slr_lpips_distance(const float *f0, const float *f1, const float *w, float *out, int N, int C, int H, int W, void *ws,
                       size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SLR_SPLAT_H */
