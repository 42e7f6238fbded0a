// The total order of the mining kernels and its packed form, shared by xsim.hip (brute force) and ivf.hip (the IVF scan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smi {

// total order: higher score first, ties -> lower index first (deterministic
// regardless of the order candidates are met).
__device__ __forceinline__ bool better(float s, int i, float s2, int i2) {
  return s > s2 || (s == s2 && i < i2);
}

// The same order as ONE unsigned compare (the running top-k lists in LDS, xsim.hip): key = order-preserving(score) << 32 |
// (0xffffffff - index); a larger key is a better candidate.
constexpr unsigned long long XS_EMPTY = (0x007fffffull << 32) | 0x80000000ull;  // (-inf, index 0x7fffffff)
__device__ __forceinline__ uint32_t xs_ord(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float xs_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
template <int K>
__device__ __forceinline__ void xs_insert(unsigned long long* list, float v, int n) {
  unsigned long long key = ((unsigned long long)xs_ord(v) << 32) | (uint32_t)(0xffffffffu - (uint32_t)n);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const unsigned long long old = __hip_atomic_fetch_max(list + j, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    key = old < key ? old : key;
    if (key == XS_EMPTY) break;
  }
}

}  // namespace smi
