// The LayerNorm arithmetic of the row kernels (rowops.hip, decoder.hip, speech.hip), once.  A row of width d is spread
// over the lanes of a wave (or of half a wave: the row-pair maps); a lane holds its share as A vectors of B floats,
// `float v[A][B]` or `f32x4 v[A]`.  Everything is fp32, in this order:
//   sum  = plain sum of the row (lane-local part by the caller while it loads, joined by row_sum)
//   mean = sum / d;  v -= mean in place;  var = sum(v * v) / d  (biased, of the CENTRED values: two passes over registers)
//   rstd = 1 / sqrt(var + eps);  y = v * rstd * w + b
// row_sum is the cross-lane sum of the lanes that share a row: wave_sum, half_sum (common.hpp) or pair_sum (rowops.hip).
// Accuracy: the fp32 mean is off by a few ulp of mean_i |x_i|, and that offset shifts EVERY centred value, so
//   |y - exact| <~ 2^-20 (|w| (|x - mean| + mean_i |x_i|) rstd + |b|)
// -- not 2^-20 (|w| |x - mean| rstd + |b|): where x ~ mean and b ~ 0 the offset of the mean is all there is.  Under an fp16
// rounding of y the difference does not show (tests/test_gpu_row_kernels.py: rule T, and the fp32 stream of ln2).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace smi {

// centre the lane's share v[A][B] of one row in place (sum = its plain lane-local sum); returns 1 / std of the row
template <int B, typename V, int A, typename Sum>
__device__ __forceinline__ float ln_center(V (&v)[A], float sum, float inv_d, float eps, Sum row_sum) {
  const float mean = row_sum(sum) * inv_d;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < A; ++k)
#pragma unroll
    for (int i = 0; i < B; ++i) {
      v[k][i] -= mean;
      q += v[k][i] * v[k][i];
    }
  return 1.0f / sqrtf(row_sum(q) * inv_d + eps);
}

// A loaded 16-B chunks of an fp16 row widened to fp32; returns their lane-local sum (element by element, in order)
template <int A>
__device__ __forceinline__ float ln_widen8(const half8 (&raw)[A], float (&v)[A][8]) {
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < A; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[k][i] = (float)raw[k][i];
      sum += v[k][i];
    }
  return sum;
}

// Host side: the row kernels exist for d = NV * 256, NV in {1, 2, 3, 4, 8}.  Calls f(std::integral_constant<int, NV>{}) for
// the NV of d and returns true; any other d: calls nothing and returns false (the launcher answers hipErrorInvalidValue).
template <typename F>
inline bool dispatch_nv(int d, F&& f) {
  switch (d) {
    case 1 * 256: f(std::integral_constant<int, 1>{}); return true;
    case 2 * 256: f(std::integral_constant<int, 2>{}); return true;
    case 3 * 256: f(std::integral_constant<int, 3>{}); return true;
    case 4 * 256: f(std::integral_constant<int, 4>{}); return true;
    case 8 * 256: f(std::integral_constant<int, 8>{}); return true;
    default: return false;
  }
}
// ... and for an fp16 or an fp32 stream: calls f(f16{}) or f(float{})
template <typename F>
inline void dispatch_f16(bool is_f16, F&& f) {
  if (is_f16) f(f16{}); else f(float{});
}

}  // namespace smi
