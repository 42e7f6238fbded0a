// The half norm of a row of fp16, stated once: smi_l2_prepare computes it of the rows it writes (l2.hip), the
// Euclidean k-means finalise of the centroid rows it writes (kmeans.hip), the bias of the L2 product-quantised lists of the rows
// the codes decode to (ivf_pq_l2.hpp, which also sums its residual terms in the same order).
#pragma once
#include "common.hpp"

namespace smi {

// A sum over a row of d columns (d a multiple of 8) in THE order of the header, in every lane: the row is d / 8 chunks of 8
// consecutive columns; lane l adds, from 0 in fp64, the terms of chunks l, l + 64, l + 128, ... in that order -- `terms(c, s)`
// adds the 8 terms of chunk c to s, the columns ascending; the 64 lane sums are joined in six steps, off = 32, 16, 8, 4, 2, 1:
// every lane takes p[l] + p[l ^ off] (an fp64 add commutes: all lanes hold the same bits after each step).
template <class Terms>
__device__ __forceinline__ double l2_ordered_sum(int d, int lane, Terms&& terms) {
  double s = 0.0;
  for (int c = lane; c < d / 8; c += 64) terms(c, s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// 1/2 sum_c row[c]^2 of a row of d fp16, `load(c)` its chunk c: the squares in the order above.  A product of two fp16 is
// exact in fp64 (22 significant bits), fused into the add or not.  The result, fl32(0.5 * sum), is in every lane.
template <class Load>
__device__ __forceinline__ float l2_half_norm(int d, int lane, Load&& load) {
  const double s = l2_ordered_sum(d, lane, [&](int c, double& acc) {
    const half8 h = load(c);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += (double)h[e] * (double)h[e];
  });
  return (float)(0.5 * s);
}

}  // namespace smi
