// Bucketing of int32 keys in three passes -- histogram, one-block exclusive scan, cursor scatter -- shared by kmeans.hip (the
// rows of the centroid update by label), ivf.hip (the rows of a build by list, the (query, probe slot) pairs of a search by
// list, the de-duplication's unit prefix sum) and mining.hip (the scan alone, over its block counts).  The histogram and the
// scatter are wave-aggregated: one atomic per distinct key of a wave, so one huge bucket costs n / 64 of them.  The kernels
// are templates over their block size: a file gets the ones it launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smi {

// Every lane with `valid` adds 1 to ctr[c]; returns the value the lane's own add would have returned had the lanes gone one
// by one.  One atomic per distinct c of the wave.  Every lane of the wave must call it.
__device__ __forceinline__ int wave_claim(int32_t* __restrict__ ctr, int c, bool valid, int lane) {
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

__device__ __forceinline__ bool key_ok(int c, int K) { return (unsigned)c < (unsigned)K; }

// One-block exclusive scan of NV sums at once over K entries, in a block of TB threads: thread t owns a contiguous run of
// ceil(K / TB) entries and sums it, thread 0 scans the TB partial sums serially, and a second pass over the run hands out
// the prefixes.
//   get(i, v)      v[0 .. NV) = what entry i adds (called in both passes);
//   put(i, run)    run[0 .. NV) = the sums over the entries below i.  It is called after get(i), so it may overwrite what get
//                  read: the scan can run in place;
//   total(run)     the sums over all K entries, thread 0 only.
// Every thread of the block must call it (two barriers); K > 0x7fffff00 is the callers' to refuse.
template <int TB, int NV, class Get, class Put, class Total>
__device__ __forceinline__ void bucket_scan(int K, Get get, Put put, Total total) {
  __shared__ int part[NV][TB];
  const int per = (K + TB - 1) / TB;
  const int64_t lo64 = (int64_t)per * threadIdx.x;
  const int lo = lo64 < K ? (int)lo64 : K, hi = lo64 + per < K ? (int)(lo64 + per) : K;
  int run[NV] = {}, v[NV];
  for (int i = lo; i < hi; ++i) {
    get(i, v);
    for (int j = 0; j < NV; ++j) run[j] += v[j];
  }
  for (int j = 0; j < NV; ++j) part[j][threadIdx.x] = run[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 0; j < NV; ++j) run[j] = 0;
#pragma unroll 8  // what hipcc chose for the three scans this replaces; left alone it takes 16 and half as many registers again
    for (int t = 0; t < TB; ++t)
      for (int j = 0; j < NV; ++j) {
        const int p = part[j][t];
        part[j][t] = run[j];
        run[j] += p;
      }
    total(run);
  }
  __syncthreads();
  for (int j = 0; j < NV; ++j) run[j] = part[j][threadIdx.x];
#pragma unroll 2  // two loads in flight, as in the scans this replaces: at K = 16 384 a run is 64 entries, a chain of latencies
  for (int i = lo; i < hi; ++i) {
    get(i, v);
    put(i, run);
    for (int j = 0; j < NV; ++j) run[j] += v[j];
  }
}

namespace {

// counts[c] += the number of i < n with keys[i] == c, for the keys in [0, K); any other key is skipped by all three passes
template <int TB>
__global__ __launch_bounds__(TB) void bucket_hist_kernel(const int32_t* __restrict__ keys, int n, int K,
                                                         int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int c = i < n ? keys[i] : -1;
  wave_claim(counts, c, key_ok(c, K), threadIdx.x & 63);
}

// out[p] = i for every i with a key in [0, K), the i of one key at consecutive p from cursor[key] (the scan's offset of the
// key) on; okey (nullable) [p] = that key.  Which i lands where inside its run depends on the atomics' arrival order.
template <int TB>
__global__ __launch_bounds__(TB) void bucket_scatter_kernel(const int32_t* __restrict__ keys, int n, int K,
                                                            int32_t* __restrict__ cursor, int32_t* __restrict__ out,
                                                            int32_t* __restrict__ okey) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  const int c = i < n ? keys[i] : -1;
  const bool ok = key_ok(c, K);
  const int pos = wave_claim(cursor, c, ok, threadIdx.x & 63);
  if (ok) {  // pos is below the next key's offset: the histogram counted this key with the same test
    out[pos] = (int32_t)i;
    if (okey) okey[pos] = c;
  }
}

}  // namespace

}  // namespace smi
