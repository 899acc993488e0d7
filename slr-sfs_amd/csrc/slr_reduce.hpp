// slr_reduce.hpp -- the deterministic reductions of csrc/metrics.hip and csrc/loss.hip: sums in double over a wave and over a workgroup,
// the same order on every run (no atomics).  A kernel writes its workgroups' sums to a caller-owned workspace; a second launch adds them
// in a fixed order.
#pragma once
#include "slr_common.hpp"

namespace slr {

// Sum of v over the 64 lanes of a wave: a butterfly, the same order on every lane and every run.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over a workgroup of NW waves of K values per thread; thread 0 returns the sums, added in wave order.  Every thread calls it.
template <int K, int NW>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[NW]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[k][wave] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) s += red[k][w];
            v[k] = s;
        }
}

}  // namespace slr
