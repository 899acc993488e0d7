// splat_gather.hpp -- what the backward gather kernels share (grad.hip, blend.hip): a source pixel's footprint, the arithmetic of one
// channel of a pass, and the host helpers of their launches.
#pragma once
#include <type_traits>

#include "slr_common.hpp"

namespace slr {

// ---- the footprint as the backward gathers see it (grad.hip, blend.hip) -------------------
// What source pixel i = (x, y) knows about its four corners NW, NE, SW, SE; `live` false (a work-item outside the image) clears
// every flag.  An out-of-image corner reads the pixel ITSELF (a valid address) and its PRODUCT is replaced by +0.0 in the sums
// below: they keep the reference's terms in the reference's order (adding +0.0 changes nothing but the sign of a -0.0), the loop
// over the channels has no branch and the loads of several channels overlap.
struct Foot {
    bool ok, k[4];     // coordinate representable; corner in the image
    int x0, y0, nw;    // NW corner and its offset y0 * W + x0 (valid where k[0])
    int o[4];          // offset each corner reads
    float w[4], dx[4], dy[4];   // weights, d/dX and d/dY of them (softsplat.py:289-299: d/dx uses the y weights and vice versa)

    __device__ __forceinline__ Foot(float fx, float fy, int x, int y, int i, int H, int W, bool live = true) {
        const Corners c = make_corners(fx, fy, x, y);
        ok = c.ok; x0 = c.x0; y0 = c.y0; nw = c.y0 * W + c.x0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            k[q] = live & c.ok & in_image(c.x0 + (q & 1), c.y0 + (q >> 1), H, W);
            o[q] = k[q] ? nw + (q >> 1) * W + (q & 1) : i;
            w[q] = c.w[q];
        }
        const float X = (float)x + fx, Y = (float)y + fy;
        const float ax = (float)(c.x0 + 1) - X, bx = X - (float)c.x0;
        const float ay = (float)(c.y0 + 1) - Y, by = Y - (float)c.y0;
        dx[0] = (-1.0f) * ay; dx[1] = (+1.0f) * ay; dx[2] = (-1.0f) * by; dx[3] = (+1.0f) * by;
        dy[0] = ax * (-1.0f); dy[1] = bx * (-1.0f); dy[2] = ax * (+1.0f); dy[3] = bx * (+1.0f);
    }
};

// One channel of a backward pass, a[q] = the value gathered at corner q.  The weights are arguments: blend.hip passes them
// multiplied by the corners' inverse normaliser.  Bit-exactness with the oracle rests on these terms in this order
// (and on -ffp-contract=off).
__device__ __forceinline__ float corner_sum(const bool (&k)[4], const float (&a)[4], const float (&w)[4]) {
    float g = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) g += k[q] ? a[q] * w[q] : 0.0f;
    return g;
}

// (gx, gy) += the channel's part of the displacement gradient, v = the source value: (v * a) * d, corners inner
__device__ __forceinline__ void disp_grad_add(float &gx, float &gy, const bool (&k)[4], float v, const float (&a)[4],
                                              const float (&dx)[4], const float (&dy)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float t = v * a[q], px = t * dx[q], py = t * dy[q];   // (products first: the two selects on one flag stay selects,
        gx += k[q] ? px : 0.0f;                                     //  with the products inside them the compiler branches)
        gy += k[q] ? py : 0.0f;
    }
}

// ---- host helpers of the backward launches -------------------------------------------------
// C channels dealt to `want` groups (grid.z), each a multiple of the kernel's `per_pass` channels: channels per group and the
// groups that are left
struct ChannelSplit { int cper, groups; };
inline ChannelSplit split_channels(int C, int want, int per_pass) {
    const int cper = want > 1 ? ((C + want - 1) / want + per_pass - 1) / per_pass * per_pass : C;
    return {cper, (C + cper - 1) / cper};
}

// two run-time switches -> f(std::bool_constant<A>, std::bool_constant<B>); neither set: nothing to launch, no <false, false> is built
template <class F>
inline void dispatch_bools(bool a, bool b, F &&f) {
    if (a && b) f(std::true_type{}, std::true_type{});
    else if (a) f(std::true_type{}, std::false_type{});
    else if (b) f(std::false_type{}, std::true_type{});
}

}  // namespace slr
