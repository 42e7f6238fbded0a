// The half norm of a row of fp16, stated once: smi_l2_prepare computes it of the rows it writes (l2.hip), the
// Euclidean k-means finalise of the centroid rows it writes (kmeans.hip).
#pragma once
#include "common.hpp"

namespace smi {

// 1/2 sum_c row[c]^2 of a row of d fp16 (d a multiple of 8), the order of the header: the row is d / 8 chunks of 8 consecutive
// columns, `load(c)` gives chunk c; lane l adds, from 0 in fp64, the squares of chunks l, l + 64, l + 128, ... in that order,
// the 8 columns of a chunk in ascending order; the 64 lane sums are joined in six steps, off = 32, 16, 8, 4, 2, 1: every lane
// takes p[l] + p[l ^ off] (an fp64 add commutes: all lanes hold the same bits after each step).  A product of two fp16 is
// exact in fp64 (22 significant bits), fused into the add or not.  The result, fl32(0.5 * sum), is in every lane.
template <class Load>
__device__ __forceinline__ float l2_half_norm(int d, int lane, Load&& load) {
  double s = 0.0;
  for (int c = lane; c < d / 8; c += 64) {
    const half8 h = load(c);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += (double)h[e] * (double)h[e];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return (float)(0.5 * s);
}

}  // namespace smi
