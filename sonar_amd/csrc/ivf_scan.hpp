// The scan unit of the IVF indexes (ivf.hip): what ivf_scan_lists_kernel and ivf_pq_scan_lists_kernel share BY
// CONSTRUCTION -- the unit lookup, the pair table with its key lists, the slice loop, the top-k fold and the read-out -- so
// that a PQ score is the flat score on the decoded row because both run the one loop below; each kernel adds its prologue,
// where a slice comes from (`fetch`) and what happens to a finished tile (`fold`).  ivf_selfjoin_kernel (whose score is the
// search score) and ivf_i8_scan_lists_kernel (the same byte geometry on int8) follow this text in copies of their own,
// for the reasons at the head of ivf.hip: a change here is made there too.  IvfKeyTest is the key predicate of the filtered
// search: what a kernel keeps of its keys, and the test its fold asks behind `id >= 0`.
//
// Workgroup b = unit b - ubase[l] of the list l with ubase[l] <= b < ubase[l + 1]: B rows of the unit's own (the pairs'
// query rows of a search, the own slots of the self-join: the MFMA B operand, columns of D) against the slots
// off[l] .. off[l + 1] (the A operand, rows of D), walked in tiles of B slots, B = 64 or 128 (chosen by the host from the
// shapes alone; the bits of a score do not depend on it).
//   Why the tile is as large as it is: every K slice of a tile is read from L2 (the list rows are shared by the units of the
//   list, the unit's rows are re-read for every tile), 2 * B * 128 bytes for B * B * 128 flop -- B / 2 flop per byte: at
//   B = 64 the scan ran at the L2's ~10 TB/s and 0.13 of the MFMA peak (profiles/ivf_experiments.txt, item 1).
//   A K slice is IVF_SLICE = 128 bytes of a row, 64 fp16, two MFMA K steps (v_mfma_f32_16x16x32_f16, fp32 accumulators);
//   lane (l15, kg) feeds the 16-byte chunk kk * 4 + kg of its row to step kk, of BOTH operands, K slices ascending: the
//   bits of a score depend on the two rows alone.
//   LDS: two K-slice buffers {the unit's rows [B][128 B], the tile's list rows [B][128 B]} (the 16-B chunk c of row r sits at
//   chunk c ^ (r & 7): the fragment reads of 16 consecutive rows spread over all banks), then what the kernel keeps behind
//   them.  Thread t loads chunk t & 7 of rows (t >> 3) + 32 j of both operands for slice i + 1 into registers while the
//   MFMAs of slice i run, and stores them to the other buffer behind them: one barrier per slice.
//   Wave (wr, wc) owns slots wr * B / 2 .. of the tile against unit rows wc * B / 2 .., so lane (l15, kg) holds unit row
//   wc * B / 2 + bi * 16 + l15 x slots wr * B / 2 + ai * 16 + 4 kg + r.
#pragma once
#include "common.hpp"
#include "topk_order.hpp"

namespace smi {

constexpr int IVF_TB = 256;     // threads per block of every kernel of ivf.hip
constexpr int IVF_SLICE = 128;  // bytes of a row in a K slice: 8 chunks of 16 B, 64 fp16 or 128 int8
static_assert(IVF_TB == 32 * (IVF_SLICE / 16), "the slice loader maps 256 threads to 32 rows x 8 chunks, B / 32 times; 2 x 2 waves");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the operands of the slice loop: fragment and accumulator types (Acc{} is the zero) and the MFMA of one 16-byte K step.  With
// one user, this struct, `extra` of ivf_pairs_init and `score` of ivf_topk_fold are more general than the two scans need: they
// are what was measured -- without them ivf_pq_scan_lists_kernel<4, 128> timed 0.3-0.9 % slower (profiles/isa_identity_ivf.txt)
struct IvfF16 {
  typedef half8 Frag;
  typedef f32x4 Acc;
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// the list of unit b < ubase[K]: the last l in [0, K) with ubase[l] <= b; ubase[l + 1] > b follows from b < ubase[K]
__device__ __forceinline__ int ivf_unit_list(const int32_t* __restrict__ ubase, int K, int b) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ubase[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the slice loop's nb_live of a unit with `nrow` rows: the 16-row blocks of this wave that hold a unit row at all (wave-uniform)
template <int B>
__device__ __forceinline__ int ivf_live_blocks(int nrow) {
  return min(B / 32, max(0, (nrow - (int)(threadIdx.x >> 6 & 1) * (B / 2) + 15) / 16));
}

// ---------------------------------------------------------------- the key predicate of a filtered scan
// Every slot has a signed int32 key (slot_keys, in slot order beside the ids; a pad slot's is unspecified), every query one
// (query_keys [nq]); a candidate passes iff bit cmp + 1 of `accept` is set, cmp = the sign of (slot key - query key) as ONE
// signed compare: bit 0 less, bit 1 equal, bit 2 greater (== 2, != 5, < 1, <= 3, > 4, >= 6; 0 nothing, 7 everything).  accept
// is a kernel argument, uniform over the launch: one instantiation serves every relation.
struct IvfNoKeys {};  // the arguments of an unkeyed scan: none
struct IvfKeys {
  const int32_t* slot_keys;
  const int32_t* query_keys;
  int accept;
};
// What a list-walking kernel keeps of its Keys.  IvfNoKeys: nothing, and every candidate passes -- the kernel is the text
// without it.  IvfKeys: B ints of LDS at `lds` (the query key of every unit row, written by pair() in the unit prologue, by
// the threads tid < B, in front of the prologue's barrier); rows() behind that barrier takes the keys of this lane's unit rows
// wc * B / 2 + bi * 16 + l15 into registers, as the range kernel holds thr[B / 32]; slots(slot0) loads the four slot keys
// of a fold beside the int4 of ids (slot0 % 4 == 0: 16-byte aligned); (bi, r) is the test.  It is to be asked behind id >= 0.
template <int B, class Keys>
struct IvfKeyTest;
template <int B>
struct IvfKeyTest<B, IvfNoKeys> {
  static constexpr int LDS = 0;
  __device__ __forceinline__ IvfKeyTest(IvfNoKeys, void*) {}
  __device__ __forceinline__ void pair(int, int) const {}
  __device__ __forceinline__ void rows() const {}
  __device__ __forceinline__ void slots(int) const {}
  __device__ __forceinline__ bool operator()(int, int) const { return true; }
};
template <int B>
struct IvfKeyTest<B, IvfKeys> {
  static constexpr int LDS = B * 4;
  const int32_t* __restrict__ slot_keys;
  const int32_t* __restrict__ query_keys;
  int accept;
  int* sqk;
  int qk[B / 32], rk[4];
  __device__ __forceinline__ IvfKeyTest(IvfKeys k, void* lds)
      : slot_keys(k.slot_keys), query_keys(k.query_keys), accept(k.accept), sqk((int*)lds) {}
  __device__ __forceinline__ void pair(int pr, int nprobe) { sqk[threadIdx.x] = pr >= 0 ? query_keys[pr / nprobe] : 0; }
  __device__ __forceinline__ void rows() {
    const int row0 = (threadIdx.x >> 6 & 1) * (B / 2) + (threadIdx.x & 15);
#pragma unroll
    for (int bi = 0; bi < B / 32; ++bi) qk[bi] = sqk[row0 + bi * 16];
  }
  __device__ __forceinline__ void slots(int slot0) {
    const int4 k4 = *(const int4*)(slot_keys + slot0);
    rk[0] = k4.x, rk[1] = k4.y, rk[2] = k4.z, rk[3] = k4.w;
  }
  __device__ __forceinline__ bool operator()(int bi, int r) const {
    const int cmp = (int)(rk[r] > qk[bi]) - (int)(rk[r] < qk[bi]);
    return accept >> (cmp + 1) & 1;
  }
};

// LDS of a search unit behind the slice buffers: the key lists [B][KT] and the pair numbers [B] (-1: no pair).  `extra(pr)`
// is what else a thread keeps of its pair; a barrier follows.
template <int KT, int B, class Extra>
__device__ __forceinline__ void ivf_pairs_init(unsigned long long* lists, int* spair, const int32_t* __restrict__ pairs, int p0,
                                               int npair, Extra extra) {
  const int tid = threadIdx.x;
  if (tid < B) {
    const int pr = tid < npair ? pairs[p0 + tid] : -1;
    spair[tid] = pr;
    extra(pr);
#pragma unroll
    for (int j = 0; j < KT; ++j) lists[tid * KT + j] = XS_EMPTY;
  }
  __syncthreads();
}

// The slice loop.  fetch(it, qv, lv): this thread's chunk of slice `it` (tile it / nk, K slice it % nk) of rows
// (tid >> 3) + 32 j of the unit's rows (qv) and of the tile's slots (lv), zeros where there is no row.  fold(slot0, acc):
// the tile is finished and acc[bi][r] is this lane's sum of slot slot0 + r (< s_end, slot0 % 4 == 0) against unit row
// wc * B / 2 + bi * 16 + l15; called for the 16-slot blocks of the wave below the end of the list only.  nb_live: the
// 16-row blocks of this wave that hold a unit row at all (wave-uniform).
template <int B, class Ops, class Fetch, class Fold>
__device__ __forceinline__ void ivf_slice_walk(char* smem, int s_begin, int s_end, int nk, int nb_live, Fetch fetch, Fold fold) {
  constexpr int OPB = B * IVF_SLICE;  // bytes of one operand's K slice
  constexpr int NR = B / 32;          // rows of an operand slice a thread loads; 16-row blocks of a wave per operand
  typedef typename Ops::Frag Frag;
  typedef typename Ops::Acc Acc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kg = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int T = (s_end - s_begin + B - 1) / B * nk;

  // where this thread's chunk of its rows lands in LDS
  const int cc = tid & 7;
  int lds_off[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int r = (tid >> 3) + 32 * j;
    lds_off[j] = r * IVF_SLICE + ((cc ^ (r & 7)) << 4);
  }
  u32x4 qv[NR], lv[NR];
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      *(u32x4*)(smem + buf * 2 * OPB + lds_off[j]) = qv[j];
      *(u32x4*)(smem + buf * 2 * OPB + OPB + lds_off[j]) = lv[j];
    }
  };

  Acc acc[NR][NR];  // [slot block ai][unit row block bi]
#pragma unroll
  for (int ai = 0; ai < NR; ++ai)
#pragma unroll
    for (int bi = 0; bi < NR; ++bi) acc[ai][bi] = Acc{};

  if (T > 0) {
    fetch(0, qv, lv);
    store(0);
  }
  __syncthreads();
  int ks = 0, tile = 0;
  for (int it = 0; it < T; ++it) {
    const int buf = it & 1;
    if (it + 1 < T) fetch(it + 1, qv, lv);
    // 16-slot blocks of this wave below the end of the list (the lists are padded to 16 slots): wave-uniform
    const int slot_w = s_begin + tile * B + wr * (B / 2);
    const int na_live = min(NR, max(0, (s_end - slot_w) / 16));
    if (na_live > 0 && nb_live > 0) {
      const char* qs = smem + buf * 2 * OPB;
      const char* ls = qs + OPB;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ch = kk * 4 + kg;
        Frag fa[NR], fb[NR];
#pragma unroll
        for (int ai = 0; ai < NR; ++ai) {
          const int ra = wr * (B / 2) + ai * 16 + l15;
          fa[ai] = *(const Frag*)(ls + ra * IVF_SLICE + ((ch ^ (ra & 7)) << 4));
        }
#pragma unroll
        for (int bi = 0; bi < NR; ++bi) {
          const int rb = wc * (B / 2) + bi * 16 + l15;
          fb[bi] = *(const Frag*)(qs + rb * IVF_SLICE + ((ch ^ (rb & 7)) << 4));
        }
#pragma unroll
        for (int ai = 0; ai < NR; ++ai)
          if (ai < na_live) {
#pragma unroll
            for (int bi = 0; bi < NR; ++bi)
              if (bi < nb_live) acc[ai][bi] = Ops::mfma(fa[ai], fb[bi], acc[ai][bi]);
          }
      }
    }
    if (it + 1 < T) store(buf ^ 1);
    if (++ks == nk) {
#pragma unroll
      for (int ai = 0; ai < NR; ++ai) {
        if (ai < na_live) fold(slot_w + ai * 16 + 4 * kg, acc[ai]);  // 16-byte aligned in int32 or fp32: off % 16 == 0
#pragma unroll
        for (int bi = 0; bi < NR; ++bi) acc[ai][bi] = Acc{};
      }
      ks = 0;
      ++tile;
    }
    __syncthreads();
  }
}

// The fold of a search: this wave's scores of four slots (ids id4; -1: a pad slot) into the pairs' key lists.  A candidate
// must beat the pair's current k-th key's score or tie it (the id decides then); a stale threshold is a valid lower bound.
// score(pr)(a, r) is the score of sum `a` of the r-th slot against pair pr.  pass(bi, r): the key predicate of slot r against
// this lane's unit row bi (IvfKeyTest; asked behind id >= 0: a pad slot's key is unspecified).
template <int KT, int B, class Acc, class Score, class Pass>
__device__ __forceinline__ void ivf_topk_fold(unsigned long long* lists, int npair, int4 id4, const Acc (&acc)[B / 32], Score score,
                                              const Pass& pass) {
  const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1;
  const int idr[4] = {id4.x, id4.y, id4.z, id4.w};
#pragma unroll
  for (int bi = 0; bi < B / 32; ++bi) {
    const int pr = wc * (B / 2) + bi * 16 + (lane & 15);
    if (pr < npair) {
      unsigned long long* lst = lists + pr * KT;
      const auto of = score(pr);
      const float thr =
          xs_unord((uint32_t)(__hip_atomic_load(lst + KT - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> 32));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = of(acc[bi][r], r);
        if (idr[r] >= 0 && pass(bi, r) && v >= thr) xs_insert<KT>(lst, v, idr[r]);
      }
    }
  }
}
// The ceiling of a page, in the place IvfKeyTest occupies in a list-walking kernel: B 64-bit keys of LDS at
// `lds`, the packed ceiling of the QUERY of every unit row (one per query, shared by its probes: the merged page is then the
// best after the ceiling over all probed lists), written by pair() in the unit prologue by the threads tid < B; rows() behind
// the prologue's barrier takes the keys of this lane's unit rows into registers; behind(bi, v, id) is the test, to be asked
// behind id >= 0.  keys null: no ceiling (every key is below ~0).  A unit row without a pair gets 0: nothing is behind it.
template <int B>
struct IvfCeiling {
  static constexpr int LDS = B * 8;
  const unsigned long long* __restrict__ keys;
  unsigned long long* sck;
  unsigned long long ck[B / 32];
  __device__ __forceinline__ IvfCeiling(const unsigned long long* k, void* lds) : keys(k), sck((unsigned long long*)lds) {}
  __device__ __forceinline__ void pair(int pr, int nprobe) { sck[threadIdx.x] = pr < 0 ? 0ull : keys ? keys[pr / nprobe] : ~0ull; }
  __device__ __forceinline__ void rows() {
    const int row0 = (threadIdx.x >> 6 & 1) * (B / 2) + (threadIdx.x & 15);
#pragma unroll
    for (int bi = 0; bi < B / 32; ++bi) ck[bi] = sck[row0 + bi * 16];
  }
  __device__ __forceinline__ bool behind(int bi, float v, int id) const { return xs_key(v, id) < ck[bi]; }
};

// ivf_topk_fold of a page: the fp32 sum is the score, its zero taken as +0 (the keys order -0 below +0, `better` does not),
// and a candidate enters only behind the ceiling of its unit row's query.
template <int KT, int B>
__device__ __forceinline__ void ivf_topk_fold_page(unsigned long long* lists, int npair, int4 id4, const f32x4 (&acc)[B / 32],
                                                   const IvfCeiling<B>& ceil) {
  const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1;
  const int idr[4] = {id4.x, id4.y, id4.z, id4.w};
#pragma unroll
  for (int bi = 0; bi < B / 32; ++bi) {
    const int pr = wc * (B / 2) + bi * 16 + (lane & 15);
    if (pr < npair) {
      unsigned long long* lst = lists + pr * KT;
      const float thr =
          xs_unord((uint32_t)(__hip_atomic_load(lst + KT - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> 32));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[bi][r] + 0.0f;
        if (idr[r] >= 0 && v >= thr && ceil.behind(bi, v, idr[r])) xs_list_insert<KT>(lst, v, idr[r]);
      }
    }
  }
}

// the fp32 sum is the score
struct IvfSumIsScore {
  __device__ __forceinline__ auto operator()(int) const {
    return [](float a, int) { return a; };
  }
};

// The read-out of a search unit: pair t's key list to the partial arrays [nprobe][nq][k_out].  (The last barrier of the slice
// loop, or the one before it when the list is empty, made the lists final.)
template <int KT>
__device__ __forceinline__ void ivf_lists_readout(const unsigned long long* lists, const int* spair, int npair, int nprobe, int nq,
                                                  int k_out, float* __restrict__ ps, int32_t* __restrict__ pi) {
  const int tid = threadIdx.x;
  if (tid < npair) {
    const int pr = spair[tid];
    const int q = pr / nprobe, p = pr - q * nprobe;
    const size_t o = ((size_t)p * nq + q) * k_out;
    for (int j = 0; j < k_out; ++j) {
      const unsigned long long key = lists[tid * KT + j];
      const bool have = key != XS_EMPTY;
      ps[o + j] = have ? xs_key_value(key) : -INFINITY;
      pi[o + j] = have ? xs_key_index(key) : -1;
    }
  }
}

// ---------------------------------------------------------------- the range scan
// LDS of a range unit behind the slice buffers, in place of the key lists: per unit row its pair number [B] (-1: no pair),
// the threshold of the pair's query [B] (fp32) and one 32-bit counter [B] (zero).  `extra(pr)` is ivf_pairs_init's.  A barrier
// follows.
template <int B, class Extra>
__device__ __forceinline__ void ivf_range_init(int* spair, float* sthr, unsigned* scnt, const int32_t* __restrict__ pairs, int p0,
                                               int npair, int nprobe, const float* __restrict__ threshold, Extra extra) {
  const int tid = threadIdx.x;
  if (tid < B) {
    const int pr = tid < npair ? pairs[p0 + tid] : -1;
    spair[tid] = pr;
    sthr[tid] = pr >= 0 ? threshold[pr / nprobe] : __builtin_nanf("");
    scnt[tid] = 0u;
    extra(pr);
  }
  __syncthreads();
}

// The fold of a range scan: sum acc[bi][r] of the slot with id id(r) against unit row wc * B / 2 + bi * 16 + l15 is a hit iff
// the unit row holds a pair, the slot holds a row (id >= 0: a pad slot is a zero row that scores 0.0 and must not hit at a
// threshold <= 0) and acc >= the pair's threshold, an fp32 compare (a NaN threshold gives no hit).  thr[bi]: the threshold of
// this lane's unit row bi, NaN where the row holds no pair -- that is how `pr < npair` is stated here.  Most tiles hold no hit:
// the ids are loaded and the slots are looked at one by one only where some lane of the wave has a sum at its threshold.
// hit(bi, mask, idr): the slots r of `mask` (bits 0 .. 3), whose ids are idr[r], are hits of unit row bi.  keys: the key
// predicate (IvfKeyTest), loaded and asked behind the wave-uniform exit only: a tile without a hit costs what it did.
template <int B, class Acc, class KeyTest, class Hit>
__device__ __forceinline__ void ivf_range_fold(const int32_t* __restrict__ ids, int slot0, const float (&thr)[B / 32],
                                               const Acc (&acc)[B / 32], KeyTest& keys, Hit hit) {
  bool some = false;
#pragma unroll
  for (int bi = 0; bi < B / 32; ++bi)
#pragma unroll
    for (int r = 0; r < 4; ++r) some |= acc[bi][r] >= thr[bi];
  if (!__any(some)) return;  // wave-uniform
  const int4 id4 = *(const int4*)(ids + slot0);
  const int idr[4] = {id4.x, id4.y, id4.z, id4.w};
  keys.slots(slot0);
#pragma unroll
  for (int bi = 0; bi < B / 32; ++bi) {
    unsigned mask = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) mask |= (unsigned)(idr[r] >= 0 && keys(bi, r) && acc[bi][r] >= thr[bi]) << r;
    if (mask) hit(bi, mask, idr);
  }
}

}  // namespace smi
