// LASER-style bitext mining on top of the xsim kernels: the retrieval rules of LASER's
// mine_bitexts.py (fwd / bwd / intersect / max) over the best candidates smi_xsim_margin_select returns, the
// deterministic compaction of the kept pairs, and the margin score of arbitrary given pairs.
//
// Candidates.  c < nx is (c, fwd_best[c], fwd_score[c]); c >= nx is (bwd_best[c - nx], c - nx, bwd_score[c - nx]).
// A candidate whose score is NaN or whose source / target is outside [0, nx) / [0, ny) is EXCLUDED: it is never kept,
// never blocks another candidate and nothing is read or written at its index.
//
// `max` is LASER's greedy walk over the candidates sorted by score -- here in the total order (score descending, -0 = +0,
// candidate number ascending) -- accepting a candidate iff neither its source nor its target is taken.  It runs without a
// sort, as parallel rounds over 64-bit keys (ordered score bits : ~candidate number):
//   (a) every live candidate atomicMax-es its key into the slot of its source and the slot of its target;
//   (b) a live candidate that holds both maxima is accepted and marks its source and target taken;
//   (c) a live candidate whose source or target is taken dies; the survivors clear their slots and are counted.
// The best live candidate of all wins both of its slots, so every round accepts at least one and the loop ends; a candidate
// that wins both slots has no live competitor ahead of it in the order, and every dead one ahead of it was (by induction
// over the rounds) rejected by the sequential walk too: the result is exactly the sequential one.  The host reads the live
// count after every round.  Live candidates are NOT compacted between rounds: every round passes over all nx + ny states
// (one byte each); at the 3-4 rounds real data takes that is a few hundred KB of traffic.
#include <algorithm>

#include "api_common.hpp"
#include "bucket.hpp"
#include "common.hpp"
#include "topk_order.hpp"

namespace smi {

namespace {

constexpr int MB = 256;  // threads per block of every kernel here

struct MineArgs {
  const int32_t* fwd_best;
  const float* fwd_score;
  const int32_t* bwd_best;
  const float* bwd_score;
  int64_t nx, ny;
  int64_t ncand;  // fwd / intersect: nx; bwd: ny; max: nx + ny
  int first_bwd;  // the candidate number of the first backward candidate (bwd: 0; max: nx; fwd / intersect: none = ncand)
  int retrieval;
  int use_thr;
  float thr;
};

// candidate c -> (source, target, score); false if the candidate is excluded.  Reads only its own entry.
__device__ __forceinline__ bool load_candidate(const MineArgs& a, int64_t c, int32_t& s, int32_t& t, float& v) {
  if (c < a.first_bwd) {
    s = (int32_t)c;
    t = a.fwd_best[c];
    v = a.fwd_score[c];
  } else {
    const int64_t j = c - a.first_bwd;
    s = a.bwd_best[j];
    t = (int32_t)j;
    v = a.bwd_score[j];
  }
  return v == v && s >= 0 && s < a.nx && t >= 0 && t < a.ny;
}

__device__ __forceinline__ bool over_threshold(const MineArgs& a, float v) { return !a.use_thr || v > a.thr; }

// order-preserving bits of the score (-0 counts as +0) above the complement of the candidate number: a larger key is
// earlier in the walk.  Never 0, so 0 marks an empty slot.
__device__ __forceinline__ unsigned long long cand_key(float v, int64_t c) {
  if (v == 0.f) v = 0.f;
  return xs_key(v, (int)c);
}

enum : unsigned char { DEAD = 0, LIVE = 1, ACCEPTED = 2 };

__global__ __launch_bounds__(MB) void max_init_kernel(MineArgs a, unsigned char* __restrict__ state) {
  const int64_t c = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (c >= a.ncand) return;
  int32_t s, t;
  float v;
  state[c] = load_candidate(a, c, s, t, v) ? LIVE : DEAD;
}

__global__ __launch_bounds__(MB) void max_bid_kernel(MineArgs a, const unsigned char* __restrict__ state,
                                                     unsigned long long* __restrict__ src_slot,
                                                     unsigned long long* __restrict__ trg_slot,
                                                     int32_t* __restrict__ live_count) {
  const int64_t c = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (c == 0) *live_count = 0;  // read by the host after the previous round, accumulated by this round's step (c)
  if (c >= a.ncand || state[c] != LIVE) return;
  int32_t s, t;
  float v;
  load_candidate(a, c, s, t, v);
  const unsigned long long key = cand_key(v, c);
  atomicMax(src_slot + s, key);
  atomicMax(trg_slot + t, key);
}

__global__ __launch_bounds__(MB) void max_accept_kernel(MineArgs a, unsigned char* __restrict__ state,
                                                        const unsigned long long* __restrict__ src_slot,
                                                        const unsigned long long* __restrict__ trg_slot,
                                                        unsigned char* __restrict__ src_taken,
                                                        unsigned char* __restrict__ trg_taken) {
  const int64_t c = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (c >= a.ncand || state[c] != LIVE) return;
  int32_t s, t;
  float v;
  load_candidate(a, c, s, t, v);
  const unsigned long long key = cand_key(v, c);
  if (src_slot[s] == key && trg_slot[t] == key) {
    state[c] = ACCEPTED;
    src_taken[s] = 1;
    trg_taken[t] = 1;
  }
}

__global__ __launch_bounds__(MB) void max_retire_kernel(MineArgs a, unsigned char* __restrict__ state,
                                                        unsigned long long* __restrict__ src_slot,
                                                        unsigned long long* __restrict__ trg_slot,
                                                        const unsigned char* __restrict__ src_taken,
                                                        const unsigned char* __restrict__ trg_taken,
                                                        int32_t* __restrict__ live_count) {
  const int64_t c = (int64_t)blockIdx.x * MB + threadIdx.x;
  int live = 0;
  if (c < a.ncand && state[c] == LIVE) {
    int32_t s, t;
    float v;
    load_candidate(a, c, s, t, v);
    if (src_taken[s] || trg_taken[t]) {
      state[c] = DEAD;
    } else {
      // nobody bids in this kernel: plain stores.  A slot no survivor clears belongs to no survivor.
      src_slot[s] = 0;
      trg_slot[t] = 0;
      live = 1;
    }
  }
  const unsigned long long bal = __ballot(live);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(live_count, (int)__popcll(bal));
}

// is candidate c one of the returned pairs?
__device__ __forceinline__ bool kept(const MineArgs& a, const unsigned char* __restrict__ state, int64_t c, int32_t& s,
                                     int32_t& t, float& v) {
  if (c >= a.ncand) return false;
  if (a.retrieval == 3) {  // SMI_MINE_MAX: what the rounds accepted (acceptance does not depend on the threshold)
    if (state[c] != ACCEPTED) return false;
    load_candidate(a, c, s, t, v);
    return over_threshold(a, v);
  }
  if (!load_candidate(a, c, s, t, v) || !over_threshold(a, v)) return false;
  return a.retrieval != 2 || (int64_t)a.bwd_best[t] == c;  // SMI_MINE_INTERSECT: t is in [0, ny) here
}

__global__ __launch_bounds__(MB) void mine_count_kernel(MineArgs a, const unsigned char* __restrict__ state,
                                                        int32_t* __restrict__ block_count) {
  __shared__ int wave_n[MB / 64];
  const int64_t c = (int64_t)blockIdx.x * MB + threadIdx.x;
  int32_t s, t;
  float v;
  const unsigned long long bal = __ballot(kept(a, state, c, s, t, v));
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (int)__popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < MB / 64; ++w) n += wave_n[w];
    block_count[blockIdx.x] = n;
  }
}

// block_count[0 .. nb) -> its exclusive prefix sums in place (one pointer reads and writes the counts: its __restrict__ says
// nothing about them), the total to *out_count: bucket.hpp's one-block scan (nb is ncand / 256: 2048 at 262 144 x 262 144).
__global__ __launch_bounds__(MB) void mine_scan_kernel(int32_t* __restrict__ block_count, int nb,
                                                       int32_t* __restrict__ out_count) {
  bucket_scan<MB, 1>(
      nb, [&](int i, int(&v)[1]) { v[0] = block_count[i]; }, [&](int i, const int(&run)[1]) { block_count[i] = run[0]; },
      [&](const int(&run)[1]) { *out_count = run[0]; });
}

__global__ __launch_bounds__(MB) void mine_scatter_kernel(MineArgs a, const unsigned char* __restrict__ state,
                                                          const int32_t* __restrict__ block_off,
                                                          int32_t* __restrict__ out_src, int32_t* __restrict__ out_trg,
                                                          float* __restrict__ out_score) {
  __shared__ int wave_n[MB / 64];
  const int64_t c = (int64_t)blockIdx.x * MB + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t s = 0, t = 0;
  float v = 0.f;
  const bool keep = kept(a, state, c, s, t, v);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) wave_n[wave] = (int)__popcll(bal);
  __syncthreads();
  if (!keep) return;
  int64_t pos = block_off[blockIdx.x] + (int)__popcll(bal & ((1ull << lane) - 1));
  for (int w = 0; w < wave; ++w) pos += wave_n[w];
  out_src[pos] = s;
  out_trg[pos] = t;
  out_score[pos] = v;
}

// ------------------------------------------------------------------------------------------- pair scores
// One wave per pair: the fp32 dot product of row s of Xn and row t of Yn (fp16, 16 B per lane per access; d % 64 == 0 keeps
// every row 16-byte aligned), then the margin in margin_select_kernel's arithmetic: the neighbour sums in list order, / k,
// 0.5f * (xm + ym).  An index outside its matrix: NaN, nothing read.
__global__ __launch_bounds__(MB) void pair_scores_kernel(const f16* __restrict__ xn, int64_t nx, const f16* __restrict__ yn,
                                                         int64_t ny, int d, const int64_t* __restrict__ src_idx,
                                                         const int64_t* __restrict__ trg_idx, int64_t m,
                                                         const float* __restrict__ fs, const float* __restrict__ bs, int k,
                                                         int kind, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * (MB / 64);
  for (int64_t p = (int64_t)blockIdx.x * (MB / 64) + (threadIdx.x >> 6); p < m; p += stride) {
    const int64_t s = src_idx[p], t = trg_idx[p];
    if (s < 0 || s >= nx || t < 0 || t >= ny) {  // wave-uniform
      if (lane == 0) out[p] = __uint_as_float(0x7fc00000u);
      continue;
    }
    const half8* xr = (const half8*)(xn + s * d);
    const half8* yr = (const half8*)(yn + t * d);
    float acc = 0.f;
    for (int c = lane; c < d / 8; c += 64) {
      const half8 xv = xr[c], yv = yr[c];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += (float)xv[e] * (float)yv[e];
    }
    const float a = wave_sum(acc);
    if (lane != 0) continue;
    float score = a;
    if (kind != 2) {
      float xm = 0.f, ym = 0.f;
      for (int j = 0; j < k; ++j) xm += fs[s * k + j];
      xm /= (float)k;
      for (int j = 0; j < k; ++j) ym += bs[t * k + j];
      ym /= (float)k;
      const float b = 0.5f * (xm + ym);
      score = kind == 0 ? a / b : a - b;
    }
    out[p] = score;
  }
}

int64_t mine_candidates(int64_t nx, int64_t ny, int retrieval) {
  return retrieval == 1 ? ny : (retrieval == 3 ? nx + ny : nx);
}

// workspace: [max only: source slots u64 [nx] | target slots u64 [ny]] block counts int32 [nb] | live count int32
//            [max only: candidate states u8 [nx + ny] | source taken u8 [nx] | target taken u8 [ny]]; the max-only regions
//            are empty for the other retrievals
struct MineWs : smi_host::WsLayout {
  unsigned long long *src_slot, *trg_slot;
  int32_t *block_count, *live_count;
  unsigned char *state, *src_taken, *trg_taken;
  MineWs(void* ws, int64_t nx, int64_t ny, int retrieval) : smi_host::WsLayout(ws) {
    const int64_t mx = retrieval == 3 ? nx : 0, my = retrieval == 3 ? ny : 0;
    src_slot = take<unsigned long long>(mx);
    trg_slot = take<unsigned long long>(my);
    block_count = take<int32_t>((mine_candidates(nx, ny, retrieval) + MB - 1) / MB);
    live_count = take<int32_t>(1);
    state = take<unsigned char>(mx + my);
    src_taken = take<unsigned char>(mx);
    trg_taken = take<unsigned char>(my);
  }
};

}  // namespace

size_t mine_workspace_bytes(int64_t nx, int64_t ny, int retrieval) { return MineWs(nullptr, nx, ny, retrieval).bytes(); }

hipError_t launch_mine(const int32_t* fwd_best, const float* fwd_score, int64_t nx, const int32_t* bwd_best,
                       const float* bwd_score, int64_t ny, int retrieval, float threshold, int32_t* out_src,
                       int32_t* out_trg, float* out_score, int32_t* out_count, void* ws, hipStream_t stream) {
  if (nx <= 0 || ny <= 0 || retrieval < 0 || retrieval > 3 || nx + ny > 0x7fffffffLL || threshold != threshold)
    return hipErrorInvalidValue;
  MineArgs a;
  a.fwd_best = fwd_best;
  a.fwd_score = fwd_score;
  a.bwd_best = bwd_best;
  a.bwd_score = bwd_score;
  a.nx = nx;
  a.ny = ny;
  a.ncand = mine_candidates(nx, ny, retrieval);
  a.first_bwd = (int)(retrieval == 1 ? 0 : (retrieval == 3 ? nx : a.ncand));
  a.retrieval = retrieval;
  a.use_thr = threshold > -INFINITY;
  a.thr = threshold;
  const int64_t nb = (a.ncand + MB - 1) / MB;
  const dim3 grid((unsigned)nb), block(MB);
  const MineWs w(ws, nx, ny, retrieval);
  hipError_t e;
  if (retrieval == 3) {
    // the slots of both sides, then the taken flags of both sides: each pair is one contiguous run
    if ((e = hipMemsetAsync(w.src_slot, 0, (size_t)(nx + ny) * 8, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.src_taken, 0, (size_t)(nx + ny), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(max_init_kernel, grid, block, 0, stream, a, w.state);
    int32_t live = 0;
    do {
      hipLaunchKernelGGL(max_bid_kernel, grid, block, 0, stream, a, w.state, w.src_slot, w.trg_slot, w.live_count);
      hipLaunchKernelGGL(max_accept_kernel, grid, block, 0, stream, a, w.state, w.src_slot, w.trg_slot, w.src_taken, w.trg_taken);
      hipLaunchKernelGGL(max_retire_kernel, grid, block, 0, stream, a, w.state, w.src_slot, w.trg_slot, w.src_taken, w.trg_taken,
                         w.live_count);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = hipMemcpyAsync(&live, w.live_count, sizeof(live), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
      if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    } while (live > 0);
  }
  hipLaunchKernelGGL(mine_count_kernel, grid, block, 0, stream, a, w.state, w.block_count);
  hipLaunchKernelGGL(mine_scan_kernel, dim3(1), block, 0, stream, w.block_count, (int)nb, out_count);
  hipLaunchKernelGGL(mine_scatter_kernel, grid, block, 0, stream, a, w.state, w.block_count, out_src, out_trg, out_score);
  return hipGetLastError();
}

hipError_t launch_pair_scores(const f16* xn, int64_t nx, const f16* yn, int64_t ny, int d, const int64_t* src_idx,
                              const int64_t* trg_idx, int64_t m, const float* fwd_scores, const float* bwd_scores, int k,
                              int kind, float* out, hipStream_t stream) {
  if (nx <= 0 || ny <= 0 || m <= 0 || d <= 0 || d % 64 || k < 1 || k > 8 || kind < 0 || kind > 2 ||
      (kind != 2 && (!fwd_scores || !bwd_scores)))
    return hipErrorInvalidValue;
  const int64_t blocks = std::min<int64_t>((m + MB / 64 - 1) / (MB / 64), 1 << 20);
  hipLaunchKernelGGL(pair_scores_kernel, dim3((unsigned)blocks), dim3(MB), 0, stream, xn, nx, yn, ny, d, src_idx, trg_idx,
                     m, fwd_scores, bwd_scores, k, kind, out);
  return hipGetLastError();
}

}  // namespace smi
