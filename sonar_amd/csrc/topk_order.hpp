// The total order "value descending, index ascending" and its packed form, stated once.  Users: xsim_walk.hpp (the brute-force
// top-k lists of xsim.hip and xsim_i8.hip, and TopK, the sorted register list over `better`), ivf.hip / ivf_scan.hpp (the IVF
// scans and the self-join), mining.hip (the max-strategy walk), decoder.hip (tile and token selection, the beam step) and
// sampling.hip (the radix descent and the most-probable-token draw).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smi {

// total order: higher score first, ties -> lower index first (deterministic
// regardless of the order candidates are met).
__device__ __forceinline__ bool better(float s, int i, float s2, int i2) {
  return s > s2 || (s == s2 && i < i2);
}

// The same order as ONE unsigned compare (the running top-k lists in LDS, xsim_walk.hpp): key = order-preserving(score) << 32 |
// (0xffffffff - index); a larger key is a better candidate.  A key built from a value other than NaN is never 0.
constexpr unsigned long long XS_EMPTY = (0x007fffffull << 32) | 0x80000000ull;  // (-inf, index 0x7fffffff)
__device__ __forceinline__ uint32_t xs_ord(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float xs_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// key of (ordered value bits, index) -- for a caller that keeps xs_ord(v) -- and of (value, index); the two halves of a key
__device__ __forceinline__ unsigned long long xs_key_ord(uint32_t o, int n) {
  return ((unsigned long long)o << 32) | (uint32_t)(0xffffffffu - (uint32_t)n);
}
__device__ __forceinline__ unsigned long long xs_key(float v, int n) { return xs_key_ord(xs_ord(v), n); }
__device__ __forceinline__ float xs_key_value(unsigned long long key) { return xs_unord((uint32_t)(key >> 32)); }
__device__ __forceinline__ int xs_key_index(unsigned long long key) { return (int)(0xffffffffu - (uint32_t)key); }

template <int K>
__device__ __forceinline__ void xs_insert(unsigned long long* list, float v, int n) {
  unsigned long long key = xs_key(v, n);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const unsigned long long old = __hip_atomic_fetch_max(list + j, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    key = old < key ? old : key;
    if (key == XS_EMPTY) break;
  }
}

// xs_insert for the lists of a page (K = 16), the cascade as a LOOP: unrolled, the 16 x 16 x 16 atomics of a
// lane's insertion path made hipcc index the walk's accumulators through scratch (528 bytes a lane).  The same list for the
// same keys: slot j keeps the larger, the smaller travels on, and an empty key has nowhere to go.
template <int K>
__device__ __forceinline__ void xs_insert_rolled(unsigned long long* list, float v, int n) {
  unsigned long long key = xs_key(v, n);
#pragma unroll 1
  for (int j = 0; j < K && key != XS_EMPTY; ++j) {
    const unsigned long long old = __hip_atomic_fetch_max(list + j, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    key = old < key ? old : key;
  }
}
template <int K>
__device__ __forceinline__ void xs_list_insert(unsigned long long* list, float v, int n) {
  if constexpr (K > 8) xs_insert_rolled<K>(list, v, n);
  else xs_insert<K>(list, v, n);
}

}  // namespace smi
