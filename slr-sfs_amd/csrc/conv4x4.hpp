// conv4x4.hpp -- sizes of the 4x4 / padding 2 convolution of the discriminator, shared by its forward and data gradient
// (csrc/conv4x4.hip) and its weight gradient (csrc/disc.hip).
#pragma once

namespace slr {

inline int c4_tiles(int C) { return (C + 31) / 32; }
inline int c4_out(int H, int stride) { return H / stride + 1; }     // (H + 2 * 2 - 4) / stride + 1
inline bool c4_sizes_ok(int N, int Cin, int Cout, int H, int W, int stride) {
    if (!(N > 0 && N < 65536 && Cin > 0 && Cin < (1 << 16) && Cout > 0 && Cout < (1 << 16) && H > 0 && W > 0 && H < (1 << 20) && W < (1 << 20)))
        return false;
    if (stride != 1 && stride != 2) return false;
    const long long OH = c4_out(H, stride), OW = c4_out(W, stride);
    return (long long)H * W < (1LL << 31) && OH * OW < (1LL << 31) && (long long)N * H * W < (1LL << 31) && (long long)N * OH * OW < (1LL << 31) &&
           (long long)N * Cin * H * W < (1LL << 40) && (long long)N * Cout * OH * OW < (1LL << 40);
}

}  // namespace slr
