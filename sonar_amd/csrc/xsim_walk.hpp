// The tile walk of the brute-force top-k mining kernels, stated once: xsim_tile256_kernel (xsim.hip, fp16 rows),
// xsim_i8_tile256_kernel (xsim_i8.hip, int8 codes) and l2_tile256_kernel (l2.hip, fp16 rows and one additive fp32 per y row) are
// wrappers of xsim_walk over an operand policy, and the host side of the passes (workspace layout, packing, launches, the K
// dispatch) is xsim_run below.
//
// The walk runs on the 256x256 ping-pong tile engine (gemm_tile256.hpp).  The K slices of ALL y tiles of a chunk form one
// continuous DMA stream through the 4-slot LDS ring: the pipeline is filled once per workgroup, not once per y tile; at every
// tile boundary the accumulators are folded into the running top-k and the next tile starts from C = 0.
//
// One byte geometry serves both operand types: a K slice of the engine is 64 B of a row, 32 fp16 or 64 int8, and a lane of
// v_mfma_i32_16x16x64_i8 feeds the 16 consecutive bytes at 16 * kg of its row, of BOTH operands -- exactly the chunk
// v_mfma_f32_16x16x32_f16 reads.  The tile-major layout, the tm_swz swizzle, the ring, the glds16 stream and every ds_read_b128
// offset are therefore the same, launch_pack_tile_major packs an int8 [rows, d] matrix when it is told fp16 [rows, d / 2], and
// the C/D layout is the 16x16 fp16 one.
//
// An operand policy P (one object per lane, built by the kernel wrapper) supplies what differs:
//   elem_t, frag_t, acc_t, mfma(w, x, c)   an operand element, the 16-byte fragment, the accumulator vector and the MFMA
//   BK                             elements in the 64 bytes of a row that a K slice holds: nt = d / BK slices per tile
//   LDS_ABOVE                      bytes of LDS above the ring: the row lists or thresholds, then whatever P keeps there
//   init(L, above, m0, t_begin)    before the lists are published and the stream starts
//   issue_tile(above, wave)        FIRST in the DMA group of a tile's first slice (below: the counted waits)
//   LISTS                          the running top-k are the key lists in LDS (xs_fold_lists), with
//     tile_t, fold_begin(n0f, ts), row_max(acc, mi, ts), score(acc, ni, mi, r, ts)   how a lane turns its sums into scores;
//                                  or P keeps them itself: top1_fold(acc, L, above, n0f, ny), top1_write(L, smem, o0, ps, pi)
//   TRACED                         a -DSMI_XSIM_TRACE build records this kernel's folds into P::trace_buf()
#pragma once
#include <algorithm>
#include <type_traits>

#include "api_common.hpp"
#include "gemm_tile256.hpp"
#include "kernels.hpp"
#include "topk_order.hpp"

namespace smi {

constexpr int XS_ROW_BYTES = G2_BK * (int)sizeof(f16);  // of a row in a K slice
constexpr int XS_BLOCK = G2_BM * XS_ROW_BYTES;          // bytes of one operand's K slice: a tile-major block
static_assert(XS_ROW_BYTES == 64 && XS_BLOCK == TM_BLOCK * (int)sizeof(f16), "the byte geometry of the fp16 engine");

// a sorted list of the K best (score, index) in registers: the chunk merge, and the walk's lists at fp16 top-1
template <int K>
struct TopK {
  float s[K];
  int i[K];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      s[j] = -INFINITY;
      i[j] = 0x7fffffff;
    }
  }
  __device__ __forceinline__ void push(float v, int idx) {
    if (better(v, idx, s[K - 1], i[K - 1])) {
      s[K - 1] = v;
      i[K - 1] = idx;
#pragma unroll
      for (int j = K - 1; j > 0; --j) {
        if (better(s[j], i[j], s[j - 1], i[j - 1])) {
          const float ts = s[j];
          s[j] = s[j - 1];
          s[j - 1] = ts;
          const int ti = i[j];
          i[j] = i[j - 1];
          i[j - 1] = ti;
        }
      }
    }
  }
};

// 16x16 MFMA blocks (gemm_tile256.hpp): a lane holds x rows row(mi), mi < 8, against y columns col(ni, r), ni < 4, r < 4, of
// the tile (from row m0 / column n0 on) -- accumulator element acc[ni][mi][r].  The sums start from the uniform term: hipcc then
// keeps no per-lane column number alive across the walk.
struct XsLane {
  int tid, lane, wave, l15, kg, wr, wc;  // wr doubles as the ping-pong group
  __device__ __forceinline__ XsLane()
      : tid(threadIdx.x), lane(tid & 63), wave(__builtin_amdgcn_readfirstlane(tid >> 6)), l15(lane & 15), kg(lane >> 4),
        wr(wave >> 2), wc(wave & 3) {}
  __device__ __forceinline__ int row(int mi, int m0 = 0) const { return m0 + wr * 128 + mi * 16 + l15; }
  __device__ __forceinline__ int col(int ni, int r, int n0 = 0) const { return n0 + wc * 64 + ni * 16 + 4 * kg + r; }
};

// ---- running top-k lists in LDS ---------------------------------------------------------------------------------------
// One list per X ROW of the tile, shared by the 16 lanes (4 lane groups x 4 column waves) that see scores of that row:
// K 64-bit keys, descending, key = order-preserving(score) << 32 | (0xffffffff - y index) -- the total order of `better`
// (score desc, index asc) as ONE unsigned compare.  A candidate is inserted with a cascade of LDS `max` atomics
// (slot j keeps the larger of {slot, carried key}, the smaller travels on): slot 0 sees every inserted key, so it ends
// as their maximum; slot 1 sees every key but that one; ... -- the final list is the top K whatever the interleaving
// of the 16 lanes, and identical from run to run.  What this buys over per-lane lists in registers (8 lists x K x 2
// words per lane: 16 VGPRs at top-1, 64 at top-4, where hipcc spilled and the deferred fold could not be used):
//  * no list registers at all: every K runs the schedule of top-1 (group 0 defers its fold into group 1's interval);
//  * the threshold of a row is the row's TRUE K-th best (one ds_read_b32 of the last key's score word), not the
//    maximum of four waves' private K-th bests: no shuffles, no publish step, fewer false passes;
//  * the walk ends with the lists final: no cross-lane / cross-wave merge.
// Insertions are rare after the first tiles (~K ln(n / K) per row over a chunk of n rows); they take the slow path.
//
// the 8 row thresholds of a lane (rows L.row(mi)): score word of the last key of each list.  Inline asm, issue and wait in
// ONE statement: as C++ loads every one of them would get `s_waitcnt vmcnt(0)` from hipcc's LDS-DMA alias tracking (the operand
// slices of the next tile are in flight) -- gemm.hip, round-3 findings.  A stale value is a valid lower bound.
template <int K>
__device__ __forceinline__ void xs_thresholds(unsigned lds_addr, float (&t)[8]) {
  uint32_t o[8];
  asm volatile(
      "ds_read_b32 %0, %8 offset:%9\n\tds_read_b32 %1, %8 offset:%10\n\tds_read_b32 %2, %8 offset:%11\n\t"
      "ds_read_b32 %3, %8 offset:%12\n\tds_read_b32 %4, %8 offset:%13\n\tds_read_b32 %5, %8 offset:%14\n\t"
      "ds_read_b32 %6, %8 offset:%15\n\tds_read_b32 %7, %8 offset:%16\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
      : "v"(lds_addr), "n"(0 * 128 * K), "n"(1 * 128 * K), "n"(2 * 128 * K), "n"(3 * 128 * K), "n"(4 * 128 * K),
        "n"(5 * 128 * K), "n"(6 * 128 * K), "n"(7 * 128 * K)
      : "memory");
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) t[mi] = xs_unord(o[mi]);
}

// the 16 per-column fp32 of a lane (columns wc * 64 + ni * 16 + 4 kg + r of the tile) from a 256-entry tile slot in LDS (what a
// policy streams with a tile: the y scales of the int8 pass, the y biases of the biased one), in one asm statement for the
// reason given at xs_thresholds
__device__ __forceinline__ void xs_read_cols16(unsigned lds_addr, f32x4 (&v)[4]) {
  asm volatile(
      "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\t"
      "ds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
      : "v"(lds_addr)
      : "memory");
}

// The fold of a finished y tile (n0f = its first y row) into the row lists: a row is tested as a whole, on the largest of the
// lane's 16 scores of it, and only when some lane of the wave passes does the wave walk the insertion path.  Columns n >= ny
// never enter a list.  P turns sums into scores: fold_begin (what it reads per tile, into ts), row_max (the largest score of a
// row's 16) and score (one element, on the slow path).
// L comes BY VALUE, here and in XsF16::top1_fold: as a reference into the walk's frame hipcc allocates 15 more VGPRs to every
// tile kernel, 255 of 256 in the int8 ones (profiles/isa_identity_xsim_walk.txt).
// A policy that declares `static constexpr bool CEILING = true` is a PAGE: ceiling(row) is the packed key of
// the tile row's exclusive ceiling, and a candidate enters only with a key strictly below it.  The test sits on the insertion
// path alone; a policy without the member compiles to the text without it.
template <class P, class = void>
struct xs_has_ceiling : std::false_type {};
template <class P>
struct xs_has_ceiling<P, std::enable_if_t<P::CEILING>> : std::true_type {};

template <int K, class P>
__device__ __forceinline__ void xs_fold_lists(P& p, const typename P::acc_t (&acc)[4][8], unsigned long long* lists,
                                              unsigned thr_addr, const XsLane L, int n0f, int ny) {
  float rowthr[8], vmx[8];
  xs_thresholds<K>(thr_addr, rowthr);
  typename P::tile_t ts;
  p.fold_begin(n0f, ts);
  bool hit = false;
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
    vmx[mi] = p.row_max(acc, mi, ts);
    hit |= vmx[mi] >= rowthr[mi];
  }
  if (__any(hit)) {
    if constexpr (xs_has_ceiling<P>::value) {
      // a page: only candidates strictly behind the row's ceiling enter, one compare of keys.  The ceilings
      // of the lane's 8 rows are loaded HERE, on the insertion path, all in front of the first use: LDS is full at K = 16, and
      // 16 more registers per lane held across the whole walk would spill.  hipcc waits for the DMA slices in flight in
      // front of a global load's use (vmcnt): correct, once per fold, and the ring is full behind it.
      unsigned long long ceil[8];
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) ceil[mi] = p.ceiling(L.row(mi));
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        if (vmx[mi] >= rowthr[mi]) {
          unsigned long long* lst = lists + L.row(mi) * K;
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int n = L.col(ni, r, n0f);
              const float v = p.score(acc, ni, mi, r, ts) + 0.0f;  // -0 -> +0: the keys order them, `better` does not
              if (v >= rowthr[mi] && n < ny && xs_key(v, n) < ceil[mi]) xs_list_insert<K>(lst, v, n);
            }
        }
      }
    } else {
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        if (vmx[mi] >= rowthr[mi]) {
          unsigned long long* lst = lists + L.row(mi) * K;
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int n = L.col(ni, r, n0f);
              const float v = p.score(acc, ni, mi, r, ts);
              if (v >= rowthr[mi] && n < ny) xs_list_insert<K>(lst, v, n);
            }
        }
      }
    }
  }
}

// Xt / Yt: TILE-MAJOR copies of the operands (common.hpp; packed into the workspace by xsim_run): a K slice of an operand is
// one contiguous 16 KiB block and the Y stream of a chunk one linear walk, instead of 256 pieces of 64 B a row apart -- the
// layout that bought the GEMMs +7 % end to end and +26 % on the bare operand stream.
// Work split: grid = (x tiles) x (y chunks); a workgroup walks the y tiles of its chunk.  Partial results ps / pi
// [nchunks][nx_pad][K]; a chunk without tiles leaves (-inf, 0x7fffffff).
template <int K, class P>
__device__ __forceinline__ void xsim_walk(P& p, const typename P::elem_t* Xt, const typename P::elem_t* Yt, int d, int ntx,
                                          int nty, int nchunks, int tiles_per_chunk, int ny, int nx_pad, float* ps, int* pi) {
  constexpr int BLOCK = G2_BM * P::BK;  // elements of one operand's K slice: a tile-major block
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int tile_m, chunk;
  g2_tile_coords(ntx, nchunks, tile_m, chunk);
  const int m0 = tile_m * G2_BM;
  const XsLane L;
  const int tid = L.tid, lane = L.lane, wave = L.wave, wr = L.wr;

  const int t_begin = chunk * tiles_per_chunk;
  const int ntiles = min(nty, t_begin + tiles_per_chunk) - t_begin;
  const int nt = d / P::BK;
  const int S = max(ntiles, 0) * nt;

  char* above = smem + G2_LDS_BYTES;
  unsigned long long* lists = (unsigned long long*)above;  // LISTS: [256 rows][K] keys
  const unsigned thr_addr = (unsigned)(size_t)above + ((wr * 128 + L.l15) * K + (K - 1)) * 8 + 4;
  if constexpr (P::LISTS) {
    if (tid < 256) {
#pragma unroll
      for (int j = 0; j < K; ++j) lists[tid * K + j] = XS_EMPTY;
    }
  }
  p.init(L, above, m0, t_begin);
  if constexpr (P::LISTS) __syncthreads();  // (before any LDS-DMA is in flight)

  if (S > 0) {
    // DMA stream state: slice s = (tile s / nt, k = s % nt)
    const typename P::elem_t* xg[2];
    const typename P::elem_t* yg[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      // piece (wave * 2 + q) of a 16 KiB block: 16 rows x 64 B = 1 KiB, linear
      xg[q] = Xt + (size_t)tile_m * nt * BLOCK + (wave * 2 + q) * (16 * P::BK) + lane * (P::BK / 4);
      yg[q] = Yt + (size_t)t_begin * nt * BLOCK + (wave * 2 + q) * (16 * P::BK) + lane * (P::BK / 4);
    }
    // The counted waits below depend on how many DMA operations a group issues: a wait leaves the newest 8 (4, 0) in flight,
    // the groups of the slices behind the awaited one hold at least 4 each, and what is older than them has landed.  What a
    // policy streams with a tile (issue_tile: the y scales of the int8 pass) therefore goes FIRST in the group of the tile's
    // first slice: it is then older than the awaited slice's own four and has landed with them.  Where a group so holds 5
    // operations the same wait retires up to two operations of the next slice as well: correct, a little earlier than needed.
    int ik = 0, is = 0;
    auto issue = [&]() {
      char* slot = smem + (is & 3) * G2_SLOT_BYTES + wave * 2048;
      const size_t koff = (size_t)ik * BLOCK;
      if (ik == 0) p.issue_tile(above, wave);
      glds16(xg[0] + koff, slot);
      glds16(xg[1] + koff, slot + 1024);
      // block (tile, k) of Y sits at (tile * nt + k) * BLOCK: the chunk's slices are consecutive
      glds16(yg[0], slot + XS_BLOCK);
      glds16(yg[1], slot + XS_BLOCK + 1024);
      yg[0] += BLOCK;
      yg[1] += BLOCK;
      ++is;
      if (++ik == nt) ik = 0;
    };
    const int t_sw = (L.kg ^ tm_swz(L.l15)) << 4;
    const int xoff = (wr * 128 + L.l15) * 64 + t_sw;
    const int woff = XS_BLOCK + (L.wc * 64 + L.l15) * 64 + t_sw;

    typename P::acc_t acc[4][8];  // [ni][mi]: 16x16 blocks of the wave's 64(n) x 128(m) tile
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = typename P::acc_t{0, 0, 0, 0};

    issue();
    if (S > 1) issue();
    if (S > 2) issue();
    if (S > 2) SMI_WAIT_VMCNT(8);
    else if (S > 1) SMI_WAIT_VMCNT(4);
    else SMI_WAIT_VMCNT(0);
    SMI_BARRIER();
    if (wr == 1) SMI_BARRIER();

    int k = 0, n0 = t_begin * G2_BN;
#ifdef SMI_XSIM_TRACE
    unsigned long long tr_t0 = wall_clock64(), tr_fold = 0, tr_n = 0, tr_max = 0;
#endif
    // y tile finished: fold the 128x64 sums of this wave into the top-k (n0f = first y row of that tile).
    // (v_permlane16/32_swap joins instead of the two ds_bpermute shuffles measured SLOWER twice: r03 experiments 10 and 14)
    auto fold = [&](int n0f) {
#ifdef SMI_XSIM_TRACE
      const unsigned long long tr_f0 = wall_clock64();
#endif
      if constexpr (P::LISTS) xs_fold_lists<K>(p, acc, lists, thr_addr, L, n0f, ny);
      else p.top1_fold(acc, L, above, n0f, ny);
#ifdef SMI_XSIM_TRACE
      const unsigned long long dt = wall_clock64() - tr_f0;
      tr_fold += dt;
      tr_max = dt > tr_max ? dt : tr_max;
      ++tr_n;
#endif
    };
    // A fold makes its interval ~5x longer, and the OTHER group waits for it at the barrier.  Left where each group
    // finishes its tile (after its last MFMA segment) the two groups fold in DIFFERENT intervals, one after the other:
    // two long intervals per tile (the trace: 1.95 us per fold and group = 3.4 of a 29.6 us tile period at top-1).
    // Group 0 therefore DEFERS its fold by one interval -- it first reads the next tile's first slice, then folds in front
    // of that slice's MFMAs (which start from C = 0 and do not read the accumulators) -- so both groups fold in the same
    // interval and a tile has one long interval instead of two.
    // The 12 fragments of the next tile's first slice stay in registers across the deferred fold (with LDS lists there are no
    // list registers, so every K runs this schedule).  Same box, 262 144 x 1 M: top-1 443.5 / 445.6 -> 434.9 / 434.2 ms (r03
    // experiment 14).
    bool pending = false;
    int n0_pending = 0;
    for (int s = 0; s < S; ++s) {
      const char* slot = smem + (s & 3) * G2_SLOT_BYTES;
      typename P::frag_t fx[8], fw[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) fw[ni] = *(const typename P::frag_t*)(slot + woff + ni * 1024);
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) fx[mi] = *(const typename P::frag_t*)(slot + xoff + mi * 1024);
      // (a lambda, as in the fp16 kernel before the walk was shared: written in line, hipcc lays the prologue's blocks out in
      // another order and the fp16 K = 4 kernel ran 2 % slower -- profiles/isa_identity_xsim_walk.txt)
      auto issue_and_wait = [&]() {
        if (s + 3 < S) {
          issue();
          SMI_WAIT_VMCNT(8);
        } else if (s + 2 < S) {
          SMI_WAIT_VMCNT(4);
        } else {
          SMI_WAIT_VMCNT(0);
        }
        SMI_LGKM0_BARRIER();
      };
      issue_and_wait();
      if (pending) {  // group 0
        fold(n0_pending);
        pending = false;
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      if (k == 0) {
        // first slice of a y tile: C = 0 is an operand of the instruction, the 128 accumulator registers
        // are never cleared by hand
        const typename P::acc_t z = {0, 0, 0, 0};
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int mi = 0; mi < 8; ++mi) acc[ni][mi] = P::mfma(fw[ni], fx[mi], z);
      } else {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int mi = 0; mi < 8; ++mi) acc[ni][mi] = P::mfma(fw[ni], fx[mi], acc[ni][mi]);
      }
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      SMI_BARRIER();
      if (++k == nt) {
        k = 0;
        if (wr == 0) {
          pending = true;
          n0_pending = n0;
        } else {
          fold(n0);
        }
        n0 += G2_BN;
      }
    }
    if (pending) fold(n0_pending);
#ifdef SMI_XSIM_TRACE
    // per workgroup and ping-pong group, the 100 MHz wall-clock ticks of the whole slice stream, of the folds inside it, the
    // number of folds and the longest one (lane 0 of waves 0 and 4 of the first 256 workgroups)
    if constexpr (P::TRACED) {
      if (lane == 0 && (wave == 0 || wave == 4) && blockIdx.x < 256) {
        unsigned long long* o = P::trace_buf() + (blockIdx.x * 2 + wr) * 4;
        o[0] = wall_clock64() - tr_t0;
        o[1] = tr_fold;
        o[2] = tr_n;
        o[3] = tr_max;
      }
    }
#endif
    if (wr == 0) SMI_BARRIER();
  }

  if constexpr (P::LISTS) {  // the lists are final: one thread per row writes its chunk-partial list
    __syncthreads();
    if (tid < 256) {
      const size_t o = ((size_t)chunk * nx_pad + m0 + tid) * K;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const unsigned long long key = lists[tid * K + j];
        ps[o + j] = xs_key_value(key);
        pi[o + j] = xs_key_index(key);
      }
    }
  } else {
    p.top1_write(L, smem, (size_t)chunk * nx_pad + m0, ps, pi);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
inline int xsim_chunks(int64_t nty) { return (int)(nty < 8 ? nty : 8); }
inline int round_k(int k) { return k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : 8)); }

// f(std::integral_constant<int, K>) for K = k rounded up to 1, 2, 4 or 8: the list lengths the kernels are built for
template <class F>
auto xs_with_k(int k, F&& f) {
  switch (round_k(k)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// workspace: partial scores fp32 [chunks][nx_pad][K] | partial indices int32 [chunks][nx_pad][K] | tile-major copy of the x
//            rows [nx_pad][row_bytes] | of the y rows [ny_pad][row_bytes] (one pass over each: ~1.5 ms of the 1.8 s at
//            1 M x 1 M fp16).  Every region is a multiple of 1 KiB: over a 16-byte aligned base each one is 16-byte aligned.
// `chunks` is one per chunk_rows rows of y up to 8: the fp16 pass sizes one per 128 (GT_BN, the size since the 128 x 128 engine),
// the int8 pass one per 256 (G2_BN); xsim_run fills one per 256, never more.
// The layout depends on the shapes alone: what a caller queried is what xsim_run writes, whatever another host thread does
// to the tuning switches in between.
struct XsimWs : smi_host::WsLayout {
  float* ps;
  int* pi;
  char *xtm, *ytm;
  XsimWs(void* ws, int64_t nx_pad, int64_t ny_pad, int K, int64_t row_bytes, int chunk_rows) : smi_host::WsLayout(ws) {
    const size_t lists = (size_t)xsim_chunks(ny_pad / chunk_rows) * nx_pad * K;
    ps = take<float>(lists);
    pi = take<int>(lists);
    xtm = take<char>((size_t)nx_pad * row_bytes);
    ytm = take<char>((size_t)ny_pad * row_bytes);
  }
};

// dst (tile-major) <- src [rows][row_bytes]: rows of row_bytes bytes are packed as fp16 [rows, row_bytes / 2], the same bytes
inline hipError_t xsim_pack(const char* src, char* dst, int64_t rows, int64_t row_bytes, hipStream_t stream) {
  for (int64_t r0 = 0; r0 < rows; r0 += 65535LL * TM_ROWS) {  // grid.y limit of the pack kernel
    const int64_t nr = std::min<int64_t>(rows - r0, 65535LL * TM_ROWS);
    hipError_t e = launch_pack_tile_major((const f16*)(src + r0 * row_bytes), (f16*)(dst + r0 * row_bytes), (int)nr,
                                          (int)(row_bytes / 2), 0, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// One pass: pack both operands tile-major, walk, merge.  X / Y: [nx_pad | ny_pad] rows of row_bytes bytes (d elements);
// `tiles(grid, w, ntx, nty, nchunks, tiles_per_chunk)` launches the pass's tile kernel over the packed copies w.xtm / w.ytm.
template <class Tiles>
hipError_t xsim_run(const void* X, int64_t nx, int64_t nx_pad, const void* Y, int64_t ny, int64_t ny_pad, int64_t row_bytes,
                    int chunk_rows, int k, int64_t y_off, int32_t* idx, float* score, void* ws, hipStream_t stream,
                    Tiles&& tiles) {
  const XsimWs w(ws, nx_pad, ny_pad, round_k(k), row_bytes, chunk_rows);
  const int ntx = (int)(nx_pad / G2_BM), nty = (int)(ny_pad / G2_BN);
  const int nchunks = xsim_chunks(nty);
  const int tpc = (nty + nchunks - 1) / nchunks;
  hipError_t e = xsim_pack((const char*)X, w.xtm, nx_pad, row_bytes, stream);
  if (e != hipSuccess) return e;
  e = xsim_pack((const char*)Y, w.ytm, ny_pad, row_bytes, stream);
  if (e != hipSuccess) return e;
  e = tiles(dim3(ntx * nchunks), w, ntx, nty, nchunks, tpc);
  if (e != hipSuccess) return e;
  return launch_xsim_merge(w.ps, w.pi, nchunks, nx, (int)nx_pad, k, y_off, idx, score, stream);
}

}  // namespace smi
