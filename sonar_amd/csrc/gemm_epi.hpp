// Activations, fp16 packing and the read-out pieces shared by the GEMM epilogues (gemm.hip, gemm_v2.hip).
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace smi {

// Activations of the fp16 epilogues.  v_rcp_f32 (1 ulp) instead of an IEEE division: `/` expands to a
// ~10-instruction div_scale / fma / div_fixup sequence per element, 128 elements per lane and tile,
// for a result that is rounded to fp16 right after.
__device__ __forceinline__ float sigmoid_f(float v) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
}
__device__ __forceinline__ float silu_f(float v) { return v * sigmoid_f(v); }
// tanh(v) = 1 - 2 / (exp(2v) + 1); exact limits at +-inf (exp -> inf gives 1, exp -> 0 gives -1)
__device__ __forceinline__ float tanh_f(float v) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(2.8853900817779268f * v) + 1.0f);
}

template <int EPI>
__device__ __forceinline__ f32x4 epi_act(f32x4 v) {
  if constexpr (EPI == EPI_RELU_F16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  } else if constexpr (EPI == EPI_SILU_F16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
  } else if constexpr (EPI == EPI_TANH_F16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = tanh_f(v[e]);
  }
  return v;
}

// Activation + rounding of 4 accumulator values to fp16.  relu runs on the rounded halves as a packed
// signed 16-bit integer max with 0 (a negative fp16 is a negative int16): one v_pk_max_i16 per two
// values instead of the canonicalise + v_max_f32 pair per value that fmaxf compiles to (MFMA results
// are not known-canonical), and relu(round(x)) == round(relu(x)).
template <int EPI>
__device__ __forceinline__ half4 epi_act_pack(f32x4 v) {
  typedef short short2v __attribute__((ext_vector_type(2)));
  if constexpr (EPI != EPI_RELU_F16) v = epi_act<EPI>(v);
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  half2v lo = __builtin_convertvector(f32x2{v[0], v[1]}, half2v);  // v_cvt_pk_f16_f32
  half2v hi = __builtin_convertvector(f32x2{v[2], v[3]}, half2v);
  if constexpr (EPI == EPI_RELU_F16) {
    const short2v z = {0, 0};
    lo = __builtin_bit_cast(half2v, __builtin_elementwise_max(__builtin_bit_cast(short2v, lo), z));
    hi = __builtin_bit_cast(half2v, __builtin_elementwise_max(__builtin_bit_cast(short2v, hi), z));
  }
  return half4{lo[0], lo[1], hi[0], hi[1]};
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// LayerNorm fold: a row's (sum, sum of squares) over K -> (rstd, -rstd * mean)
__device__ __forceinline__ float2 fold_row_affine(float sum, float sumsq, float inv_k, float eps) {
  const float mean = sum * inv_k;
  const float var = fmaxf(sumsq * inv_k - mean * mean, 0.f);
  const float rs = __builtin_amdgcn_rsqf(var + eps);  // 1 ulp; the result is rounded to fp16 a few steps later
  return float2{rs, -rs * mean};
}

// The affine in front of the activation, on one accumulator block.  MODE 0: v + c2 (c2 = the bias);  1: LayerNorm fold with
// the exact mean term, rs * v + (nm * c1 + c2);  2: fold with centred weights, rs * v + c2.
// v_pk_fma_f32: two values per instruction (a wave64 VALU instruction takes 4 cycles)
template <int MODE>
__device__ __forceinline__ f32x4 fold_apply(f32x4 v, const f32x4& c1, const f32x4& c2, float rs, float nm) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 rs2 = {rs, rs}, nm2 = {nm, nm};
#pragma unroll
  for (int hp2 = 0; hp2 < 2; ++hp2) {
    const f32x2 c2p = {c2[2 * hp2], c2[2 * hp2 + 1]};
    f32x2 vp = {v[2 * hp2], v[2 * hp2 + 1]};
    if constexpr (MODE == 1) {
      const f32x2 c1p = {c1[2 * hp2], c1[2 * hp2 + 1]};
      vp = __builtin_elementwise_fma(rs2, vp, __builtin_elementwise_fma(nm2, c1p, c2p));
    } else if constexpr (MODE == 2) {
      vp = __builtin_elementwise_fma(rs2, vp, c2p);
    } else {
      vp = vp + c2p;
    }
    v[2 * hp2] = vp[0];
    v[2 * hp2 + 1] = vp[1];
  }
  return v;
}

// A row's maximum / sum over its four lane groups (lanes 16 and 32 apart), joined by v_permlane16/32_swap (VALU rate;
// __shfl_xor is an LDS round trip per step)
__device__ __forceinline__ float quad_max(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float quad_sum(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Tile-major store of a 32-column k-block = the accumulator-block pair A, B: v_permlane16_swap moves lane group 1's piece of
// A against group 0's piece of B (and 3 against 2) -- rows 16..31 / 48..63 of h0 <-> rows 0..15 / 32..47 of h1 -- after which
// every lane holds one whole 16-B chunk: group kg owns chunk (kg&1)*2 + (kg>>1) of the k-block.
__device__ __forceinline__ u32x4 tm_chunk(uint2 h0, uint2 h1) {
  const auto s0 = __builtin_amdgcn_permlane16_swap(h0.x, h1.x, false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(h0.y, h1.y, false, false);
  return u32x4{s0[0], s1[0], s0[1], s1[1]};
}

}  // namespace smi
