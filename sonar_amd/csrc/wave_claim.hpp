// Wave-aggregated bucketing by label, shared by kmeans.hip (the centroid update) and ivf.hip (the inverted lists and the
// inverted probe table): one atomic per distinct label of a wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smi {

// Every lane with `valid` adds 1 to ctr[c]; returns the value the lane's own add would have returned had the lanes gone one
// by one.  One atomic per distinct c of the wave.  Every lane of the wave must call it.
__device__ __forceinline__ int km_wave_claim(int32_t* __restrict__ ctr, int c, bool valid, int lane) {
  int rank = 0;
  bool pending = valid;
  for (;;) {
    const unsigned long long act = __ballot(pending);
    if (!act) break;
    const int leader = __ffsll((long long)act) - 1;
    const int lc = __shfl(c, leader, 64);
    const bool same = pending && c == lc;
    const unsigned long long grp = __ballot(same);
    int base = 0;
    if (lane == leader) base = atomicAdd(ctr + lc, (int)__popcll(grp));
    base = __shfl(base, leader, 64);
    if (same) {
      rank = base + (int)__popcll(grp & ((1ull << lane) - 1));
      pending = false;
    }
  }
  return rank;
}

__device__ __forceinline__ bool km_label_ok(int c, int K) { return (unsigned)c < (unsigned)K; }

}  // namespace smi
