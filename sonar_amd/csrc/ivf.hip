// IVF-Flat index over rows of smi_xsim_normalize: K inverted lists, list-contiguous copies of the rows, and
// a scan that scores every query against the rows of the lists it probes only.  The coarse quantiser is spherical k-means
// (kmeans.hip) and the probe is smi_xsim_topk against its centroids; both are callers' business, not this file's.
//
// Both halves bucket int32 keys with the three passes of the k-means update (histogram, exclusive scan, cursor scatter, all
// wave-aggregated: bucket.hpp).  The build buckets the row numbers by label, the search buckets the nq * nprobe
// (query, probe slot) pairs by list -- the inverted probe table -- so that a work unit of the scan is ONE list and up to
// 64 or 128 of the pairs that probe it: the list's rows are read once per unit, not once per query.
//
// The scan unit walks its list in tiles of as many slots as it has pairs; a tile's scores are MFMA products, K slices
// ascending (the bits of a score depend on the two rows alone), that are folded into one running top-k per pair, the LDS key
// lists of xsim.hip.  A pair's list is written to the partial array [nprobe][nq][k]; smi_xsim_merge_topk's kernel merges
// the nprobe parts.  No atomics on results.  The unit itself -- lookup, pair table, slice loop, fold, read-out -- is
// ivf_scan.hpp (read its comment first).  Five kernels here walk lists that way:
//   ivf_scan_lists_kernel      fp16 rows (3.18): ivf_scan.hpp's functions; fetches both operands from memory;
//   ivf_range_lists_kernel     the same rows, unit and loop with a threshold fold (3.23): every row at or above a per-query
//                              threshold, counted in one walk and written in a second;
//   ivf_pq_scan_lists_kernel   product-quantised rows (3.21): the same functions, so a score has the flat scan's bits BY
//                              CONSTRUCTION; the list operand is decoded from the codebooks in the fetch; its RES
//                              instantiation (3.22: rows encoded as residuals against their list's centroid) adds one fp32
//                              per pair, the query's score against that centroid, where a sum meets the fold;
//   ivf_i8_scan_lists_kernel   int8 codes and one fp32 scale per row (3.19): the integer MFMA, the scales enter in the fold;
//   ivf_selfjoin_kernel        SemDeDup's per-list self-join (3.20): the unit's rows are list rows, its own fold and ending.
// The last two spell the same loop out in their own text (keep it equal to ivf_slice_walk's): as instances of the
// function the 128-row self-join waited for the prefetched slice in front of its MFMAs, and the int8 scan measured
// 0.2-0.4 % slower in two cells of one round of two (profiles/isa_identity_ivf.txt).
// The first four answer a search and each has a KEYED TWIN for the filtered search (3.24: a per-query key predicate in the
// fold; a row mask needs no kernel, only ids of -1): their text is csrc/ivf_list_kernels.hpp, included twice below.
// The bucketing, the unit rule, the merge and the host halves are shared by calls: an entry gives the skeletons below
// (build_entry, search_entry, rows_entry) its own checks and its gather or scan launch.  The quantisers (int8 rows; PQ
// encode, train, decode) and the gathers that encode follow their scans.
#include "api_common.hpp"
#include "ivf_scan.hpp"
#include "bucket.hpp"
#include "l2_rows.hpp"

#include <type_traits>

using namespace smi;
using namespace smi_host;

namespace smi {

namespace {

constexpr int IVF_ALIGN = SMI_IVF_LIST_ALIGN;  // slots: one 16-row A block of the 16x16x32 MFMA
constexpr int IVF_BM = SMI_IVF_UNIT_QUERIES;   // (query, probe slot) pairs of a scan unit = slots of its tiles ...
constexpr int IVF_BIG = 2 * IVF_BM;            // ... or twice that, where the lists are probed by many pairs
constexpr int IVF_BK = IVF_SLICE / 2;  // fp16 of a K slice
constexpr int64_t IVF_MAX = 0x7fffff00LL;

static_assert(IVF_ALIGN == 16, "a 16-slot A block of the scan's MFMA never spans two lists");
static_assert(IVF_BM == 64, "the slice loader takes B / 32 passes");

// ---------------------------------------------------------------- bucketing (bucket.hpp, for any int32 keys)
// off[c] = sum over c' < c of counts[c'] rounded up to `align`, off[K] = the total; cursor = a copy of off[0 .. K) for the
// scatter to advance; ubase (nullable) [K + 1] = the same prefix sum of ceil(counts / unit).
__global__ __launch_bounds__(IVF_TB) void ivf_scan_kernel(const int32_t* __restrict__ counts, int K, int align, int unit,
                                                          int32_t* __restrict__ off, int32_t* __restrict__ cursor,
                                                          int32_t* __restrict__ ubase) {
  bucket_scan<IVF_TB, 2>(
      K,
      [&](int i, int(&v)[2]) {
        const int c = counts[i];
        v[0] = (c + align - 1) / align * align;
        v[1] = (c + unit - 1) / unit;
      },
      [&](int i, const int(&run)[2]) {
        off[i] = cursor[i] = run[0];
        if (ubase) ubase[i] = run[1];
      },
      [&](const int(&run)[2]) {
        off[K] = run[0];
        if (ubase) ubase[K] = run[1];
      });
}

// ---------------------------------------------------------------- build: the row copies
// One wave per slot below off[K]: the row ids[slot] names, or zeros for a pad slot (id -1).  16 bytes per lane per access.
__global__ __launch_bounds__(IVF_TB) void ivf_gather_kernel(const f16* __restrict__ xn, int d, const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ off, int K, f16* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (slot >= off[K]) return;  // wave-uniform
  const int id = ids[slot];
  u32x4* o = (u32x4*)(rows + (size_t)slot * d);
  if (id < 0) {
    for (int c = lane; c < d / 8; c += 64) o[c] = u32x4{0u, 0u, 0u, 0u};
  } else {
    const u32x4* s = (const u32x4*)(xn + (size_t)id * d);
    for (int c = lane; c < d / 8; c += 64) o[c] = s[c];
  }
}

// ---------------------------------------------------------------- search
// every partial list starts as k x (-inf, -1): what a probe slot that names no list contributes
__global__ __launch_bounds__(IVF_TB) void ivf_fill_kernel(float* __restrict__ ps, int32_t* __restrict__ pi, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  if (i < m) {
    ps[i] = -INFINITY;
    pi[i] = -1;
  }
}

// The unit of ivf_scan.hpp with pairs poff[l] + B * (b - ubase[l]) .. of the bucketed pair order as its rows: the query rows
// the pairs name.  LDS behind the slice buffers: the key lists [B][KT], the pair numbers [B].
template <int B>
constexpr int ivf_scan_lds(int KT) { return 2 * 2 * B * IVF_SLICE + B * KT * 8 + B * 4; }

// (the kernel, ivf_scan_lists_kernel<KT, B>, and its keyed twin: ivf_list_kernels.hpp, included below)

int64_t slots_bound(int64_t n, int64_t K) {
  const int64_t m = std::min(n, K);
  return m * IVF_ALIGN + (n - m) / IVF_ALIGN * IVF_ALIGN;
}
// (a *_workspace_bytes function runs the shape checks of its entry under KeepLastError: api_common.hpp)
// pairs of a scan unit = slots of its tiles: 128 where the lists are probed by 256 pairs or more on average, else 64.  (At
// 128 pairs per list of ~61 rows, 1 M rows over 16 384 lists at nprobe = 8, the 128-slot tile is half empty and the scan took
// 1.84 ms against 1.34; at 256 pairs per list of ~977 rows it took 1.45 ms against 2.53: profiles/ivf_experiments.txt.)
int unit_pairs(int64_t pairs, int64_t K) { return pairs >= 2 * (int64_t)IVF_BIG * K ? IVF_BIG : IVF_BM; }
// the scan's grid: a list with pairs has at most floor(pairs / unit) + 1 units
int64_t units_bound(int64_t pairs, int64_t K, int unit) { return pairs / unit + std::min(pairs, K); }

// build: cursor int32 [K]
struct BuildWs : WsLayout {
  int32_t* cursor;
  BuildWs(void* ws, int64_t K) : WsLayout(ws) { cursor = take<int32_t>(K, 16); }
};
// search: pair counts [K] | pair offsets [K + 1] | unit offsets [K + 1] | cursor [K] | bucketed pairs [nq * nprobe] |
//         partial scores fp32 [nprobe][nq][k] | partial ids int32 [nprobe][nq][k]
//         and behind them, in the int8 search (i8_dim = its d, else 0): query codes int8 [nq, d] | query scales fp32 [nq]
//         and, in the paged search (ceil_rows = its nq, else 0): one 64-bit ceiling key per query
struct SearchWs : WsLayout {
  int32_t *pcount, *poff, *ubase, *cursor, *pairs, *pi;
  float *ps, *qscale;
  int8_t* qc;
  unsigned long long* ceil;
  SearchWs(void* ws, int64_t nq, int64_t K, int nprobe, int k, int i8_dim = 0, int64_t ceil_rows = 0) : WsLayout(ws) {
    const size_t P = (size_t)nq * nprobe;
    pcount = take<int32_t>(K, 16);
    poff = take<int32_t>(K + 1, 16);
    ubase = take<int32_t>(K + 1, 16);
    cursor = take<int32_t>(K, 16);
    pairs = take<int32_t>(P, 16);
    ps = take<float>(P * k, 16);
    pi = take<int32_t>(P * k, 16);
    qc = take<int8_t>(i8_dim ? (size_t)nq * i8_dim : 0, 16);
    qscale = take<float>(i8_dim ? nq : 0, 16);
    ceil = take<unsigned long long>((size_t)ceil_rows, 16);
  }
};

// the launch of a list-walking kernel: its instantiation for units of IVF_BM or of IVF_BIG rows, as `unit` says
template <auto Small, auto Big, typename... Args>
hipError_t launch_units(int unit, int64_t units, int lds_small, int lds_big, hipStream_t st, Args... args) {
  if (unit == IVF_BIG) return launch_with_lds<Big>(dim3((unsigned)units), IVF_TB, lds_big, st, args...);
  return launch_with_lds<Small>(dim3((unsigned)units), IVF_TB, lds_small, st, args...);
}
// the same for a kernel with a keyed twin: with keys, the twin, the keys behind the kernel's own arguments and
// the query keys [unit] behind its LDS
template <auto Small, auto Big, auto KeyedSmall, auto KeyedBig, typename... Args>
hipError_t launch_units_keyed(const IvfKeys* keys, int unit, int64_t units, int lds_small, int lds_big, hipStream_t st,
                              Args... args) {
  if (!keys) return launch_units<Small, Big>(unit, units, lds_small, lds_big, st, args...);
  return launch_units<KeyedSmall, KeyedBig>(unit, units, lds_small + IVF_BM * 4, lds_big + IVF_BIG * 4, st, args..., *keys);
}
// the refusals of a keyed entry's own arguments: they follow the null checks of its twin
int check_keys(const IvfKeys& keys) {
  if (!keys.slot_keys || !keys.query_keys) return fail(SMI_ERR_INVALID_ARG, "null slot_keys or query_keys");
  if ((uintptr_t)keys.slot_keys % 16) return fail(SMI_ERR_INVALID_ARG, "slot_keys must be 16-byte aligned");
  if (keys.accept < 0 || keys.accept > 7)
    return fail(SMI_ERR_INVALID_ARG, "accept=%d must be in [0, 7]: bit 0 less, bit 1 equal, bit 2 greater", keys.accept);
  return SMI_OK;
}

// ---------------------------------------------------------------- range search
// ivf_scan_lists_kernel with another fold and another ending: every row of the probed lists whose score is at least the
// query's threshold, not the k best.  The unit, the pair table, the fetch and the slice loop are the flat scan's, so a hit's
// score has the bits smi_ivf_search returns for the same two rows.  How many rows a pair hits is not known before the walk, so
// the lists are walked twice: !EMIT counts (a lane's unit rows are fixed for the whole walk: it counts in registers and adds
// to the LDS counter of the row once, at the end; a pair belongs to one unit, which writes pair_counts[pair]: no global
// atomics), EMIT writes hit number c of a pair (c: a fetch-add on the row's LDS counter, any order) to base[pair] + c --
// only below base[pair + 1] and below `total`, so thresholds that were lowered between the two calls lose hits and never
// write outside the pair's segment.  LDS behind the slice buffers: pair numbers [B], thresholds [B], counters [B].
template <int B>
constexpr int ivf_range_lds() { return 2 * 2 * B * IVF_SLICE + 3 * B * 4; }
// (the kernel, ivf_range_lists_kernel<B, EMIT>, and its keyed twin: ivf_list_kernels.hpp, included below)

// ================================================================ int8 scalar-quantised lists
// The same lists with one signed byte per element and one fp32 scale per row.  The scan is ivf_scan.hpp's decomposition
// with the byte geometry unchanged: a K slice is still 128 bytes of a row, now 128 elements and two
// v_mfma_i32_16x16x64_i8 steps, so a tile takes half as many slices and barriers.  The int32 sums are exact; the scales
// meet the sum in the tile fold only.
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int IVF_I8_MAX_DIM = SMI_IVF_I8_MAX_DIM;  // 127^2 * d < 2^31
static_assert((int64_t)127 * 127 * IVF_I8_MAX_DIM < (1LL << 31), "the int32 sum of a row pair cannot overflow");

__device__ __forceinline__ float i8_absmax8(u32x4 v) {
  const half8 h = __builtin_bit_cast(half8, v);
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)h[e]));
  return m;
}

// THE row quantiser, one wave per row (lane = threadIdx.x & 63; every lane of the wave calls it): codes[0 .. d) and the
// value of *scale of the d fp16 at x.  amax is a max of exact fp32 values: the same in any order.  Two passes over the row;
// the second finds it in the cache.
__device__ __forceinline__ void i8_encode_row(const f16* __restrict__ x, int d, int lane, int8_t* __restrict__ codes,
                                              float* __restrict__ scale) {
  const u32x4* s = (const u32x4*)x;
  float amax = 0.f;
  for (int c = lane; c < d / 8; c += 64) amax = fmaxf(amax, i8_absmax8(s[c]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const bool zero = amax == 0.f;
  const float inv = zero ? 0.f : __fdiv_rn(127.0f, amax);
  if (lane == 0) *scale = zero ? 0.f : __fdiv_rn(amax, 127.0f);
  uint2* o = (uint2*)codes;
  for (int c = lane; c < d / 8; c += 64) {
    const half8 h = __builtin_bit_cast(half8, s[c]);
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float r = fminf(fmaxf(rintf((float)h[e] * inv), -127.f), 127.f);
      w[e >> 2] |= ((unsigned)(int)r & 0xffu) << ((e & 3) * 8);
    }
    o[c] = uint2{w[0], w[1]};
  }
}

__global__ __launch_bounds__(IVF_TB) void ivf_i8_encode_kernel(const f16* __restrict__ xn, int64_t n, int d,
                                                               int8_t* __restrict__ codes, float* __restrict__ scales) {
  const int64_t row = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  i8_encode_row(xn + (size_t)row * d, d, threadIdx.x & 63, codes + (size_t)row * d, scales + row);
}

// One wave per slot below off[K]: the encoding of the row ids[slot] names, or zero codes and scale 0 for a pad slot.
__global__ __launch_bounds__(IVF_TB) void ivf_i8_gather_kernel(const f16* __restrict__ xn, int d,
                                                               const int32_t* __restrict__ ids,
                                                               const int32_t* __restrict__ off, int K,
                                                               int8_t* __restrict__ codes, float* __restrict__ scales) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (slot >= off[K]) return;  // wave-uniform
  const int id = ids[slot];
  if (id < 0) {
    uint2* o = (uint2*)(codes + (size_t)slot * d);
    for (int c = lane; c < d / 8; c += 64) o[c] = uint2{0u, 0u};
    if (lane == 0) scales[slot] = 0.f;
  } else {
    i8_encode_row(xn + (size_t)id * d, d, lane, codes + (size_t)slot * d, scales + slot);
  }
}

// ivf_scan_lists_kernel on int8 codes: the same units, tiles, loader mapping, swizzle, buffers and key lists (read
// ivf_scan.hpp's comment first), spelled out here (see the head of the file).
// What differs: a K slice is IVF_I8_BK = 128 ELEMENTS (the same 128 bytes of a row), lane (l15, kg) feeds chunk
// kk * 4 + kg of its row to MFMA step kk as 16 consecutive K bytes of BOTH operands, so the sum is the exact integer
// whatever K order the instruction uses; nk = ceil(d / 128) and the chunks of the last slice past d (d % 128 == 64) are
// zero-filled, which adds 0 exactly.  The fold loads the four slot scales beside the four ids, takes the pair's query scale
// from LDS and forms fl32(fl32((float)acc * scale_x) * scale_q).
constexpr int IVF_I8_BK = 128;            // bytes = elements of a K slice (256 was tried: profiles/ivf_i8_experiments.txt)
constexpr int IVF_I8_CH = IVF_I8_BK / 16;  // 16-byte chunks of a row's slice; the swizzle is over all of them
constexpr int IVF_I8_RP = IVF_TB / IVF_I8_CH;  // rows of an operand slice the 256 threads load in one pass
static_assert(IVF_I8_BK % 64 == 0 && (IVF_I8_CH & (IVF_I8_CH - 1)) == 0 && IVF_BM % IVF_I8_RP == 0, "loader mapping");

template <int B>
constexpr int ivf_i8_scan_lds(int KT) { return 2 * 2 * B * IVF_I8_BK + B * KT * 8 + 2 * B * 4; }

// (the kernel, ivf_i8_scan_lists_kernel<KT, B>, and its keyed twin: ivf_list_kernels.hpp)

// ---------------------------------------------------------------- the list-walking kernels, each with its keyed twin
// The four kernels that answer a search are stated once, in ivf_list_kernels.hpp, and compiled twice: as
// they always were (IvfNoKeys: IvfKeyTest keeps nothing and lets every candidate pass, and the kernel is instruction for
// instruction what it was: profiles/isa_identity_filter.txt), and as <name>_keyed with one more argument, IvfKeys,
// the query keys [B] behind everything else in LDS and the key predicate in the fold.  Two inclusions, not one function
// called by two kernels: as the instance of a shared function the unkeyed kernels came out with other registers and another
// order of their argument loads, whichever way the arguments were passed.
constexpr int PQ_CW = 256;  // codewords of every sub-quantiser of the product-quantised lists (3.21): a code is one byte
#define IVF_TWIN(name) name
#define IVF_TWIN_PARAM
#define IVF_TWIN_KEYS IvfNoKeys
#define IVF_TWIN_KEYARGS IvfNoKeys{}
#include "ivf_list_kernels.hpp"
#undef IVF_TWIN
#undef IVF_TWIN_PARAM
#undef IVF_TWIN_KEYS
#undef IVF_TWIN_KEYARGS
#define IVF_TWIN(name) name##_keyed
#define IVF_TWIN_PARAM , IvfKeys keyargs
#define IVF_TWIN_KEYS IvfKeys
#define IVF_TWIN_KEYARGS keyargs
#include "ivf_list_kernels.hpp"
#undef IVF_TWIN
#undef IVF_TWIN_PARAM
#undef IVF_TWIN_KEYS
#undef IVF_TWIN_KEYARGS

// ---------------------------------------------------------------- a page of the flat search
// ivf_scan_lists_kernel with key lists of IVF_PAGE = 16 and the ceiling of the pair's query in the fold (IvfCeiling,
// ivf_scan.hpp): the 16 best of the list strictly behind the ceiling.  The unit, the fetch and the slice loop are the flat
// scan's, so a score has smi_ivf_search's bits.  Lists longer than 16 are not the way to more results: a row inserts about
// K (1 + ln(n / K)) times, a quarter of a 1000-row list's candidates at K = 64, each a cascade of K dependent LDS atomics.
// LDS behind the slice buffers: the key lists [B][16], the pair numbers [B], the ceiling keys [B].
constexpr int IVF_PAGE = 16;
template <int B>
constexpr int ivf_page_scan_lds() { return ivf_scan_lds<B>(IVF_PAGE) + IvfCeiling<B>::LDS; }

template <int B>
__global__ __launch_bounds__(IVF_TB) void ivf_scan_page_kernel(const f16* __restrict__ qn, int d, int nq, int nprobe,
                                                               const f16* __restrict__ rows, const int32_t* __restrict__ ids,
                                                               const int32_t* __restrict__ off, int K,
                                                               const int32_t* __restrict__ poff,
                                                               const int32_t* __restrict__ ubase,
                                                               const int32_t* __restrict__ pairs, int k_out,
                                                               float* __restrict__ ps, int32_t* __restrict__ pi,
                                                               const unsigned long long* __restrict__ ceil_keys) {
  constexpr int NR = B / 32, KT = IVF_PAGE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lists = (unsigned long long*)(smem + 4 * B * IVF_SLICE);
  int* spair = (int*)(lists + B * KT);
  IvfCeiling<B> ceil(ceil_keys, spair + B);
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= ubase[K]) return;
  const int l = ivf_unit_list(ubase, K, b);
  const int p0 = poff[l] + (b - ubase[l]) * B;
  const int npair = min(B, poff[l + 1] - p0);
  const int s_begin = off[l], s_end = off[l + 1];
  ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [&](int pr) { ceil.pair(pr, nprobe); });
  ceil.rows();

  const int nk = d / IVF_BK, cc = tid & 7;
  const f16* qsrc[NR];  // this thread's query rows of a slice
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int pr = spair[(tid >> 3) + 32 * j];
    qsrc[j] = pr >= 0 ? qn + (size_t)(pr / nprobe) * d + cc * 8 : nullptr;
  }
  auto fetch = [&](int it, u32x4(&qv)[NR], u32x4(&lv)[NR]) {  // ivf_scan_lists_kernel's
    const int tile = it / nk, ks = it - tile * nk;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int slot = s_begin + tile * B + (tid >> 3) + 32 * j;
      qv[j] = qsrc[j] ? *(const u32x4*)(qsrc[j] + ks * IVF_BK) : u32x4{0u, 0u, 0u, 0u};
      lv[j] = slot < s_end ? *(const u32x4*)(rows + (size_t)slot * d + ks * IVF_BK + cc * 8) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto fold = [&](int slot0, const f32x4(&acc)[NR]) {
    ivf_topk_fold_page<KT, B>(lists, npair, *(const int4*)(ids + slot0), acc, ceil);
  };
  ivf_slice_walk<B, IvfF16>(smem, s_begin, s_end, nk, ivf_live_blocks<B>(npair), fetch, fold);
  ivf_lists_readout<KT>(lists, spair, npair, nprobe, nq, k_out, ps, pi);
}

int i8_check_dim(int32_t d) {
  if (d > IVF_I8_MAX_DIM)
    return fail(SMI_ERR_UNSUPPORTED, "d=%d: above %d the int32 sum of int8 products could overflow", d, IVF_I8_MAX_DIM);
  return SMI_OK;
}

// ---------------------------------------------------------------- host halves shared by the flat, int8 and PQ entries
// the refusals of a build: on shape (all the sizing functions ask), then on the caller's storage and workspace
int check_build_shape(int64_t n, int32_t d, int64_t K) {
  if (const int rc = check_shape(n, "n", d, K, "list")) return rc;
  if (slots_bound(n, K) > IVF_MAX)
    return fail(SMI_ERR_UNSUPPORTED, "n=%lld rows over K=%lld lists can need %lld slots: slot numbers must fit int32",
                (long long)n, (long long)K, (long long)slots_bound(n, K));
  return SMI_OK;
}
int check_build_args(int64_t n, int32_t d, int64_t K, int64_t capacity_slots, const void* ws, int64_t ws_bytes,
                     const char* sizing) {
  if (const int rc = check_build_shape(n, d, K)) return rc;
  if (capacity_slots < slots_bound(n, K))
    return fail(SMI_ERR_INVALID_ARG, "capacity of %lld slots, smi_ivf_slots_bound(n, K) = %lld", (long long)capacity_slots,
                (long long)slots_bound(n, K));
  return check_ws(ws, ws_bytes, BuildWs(nullptr, K).bytes(), sizing);
}

// the three bucketing passes of a build: list_sizes, list_offsets and the row number of every slot (-1: pad or unused)
hipError_t bucket_rows(const int32_t* labels, int64_t n, int64_t K, int32_t* list_ids, int64_t capacity_slots,
                       int32_t* list_offsets, int32_t* list_sizes, int32_t* cursor, hipStream_t st) {
  if (hipError_t e = hipMemsetAsync(list_sizes, 0, (size_t)K * 4, st); e != hipSuccess) return e;
  if (hipError_t e = hipMemsetAsync(list_ids, 0xff, (size_t)capacity_slots * 4, st); e != hipSuccess) return e;  // -1
  const dim3 block(IVF_TB), rows_grid = grid_for(n, IVF_TB);
  hipLaunchKernelGGL(bucket_hist_kernel<IVF_TB>, rows_grid, block, 0, st, labels, (int)n, (int)K, list_sizes);
  hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), block, 0, st, list_sizes, (int)K, IVF_ALIGN, 1, list_offsets, cursor,
                     (int32_t*)nullptr);
  hipLaunchKernelGGL(bucket_scatter_kernel<IVF_TB>, rows_grid, block, 0, st, labels, (int)n, (int)K, cursor, list_ids,
                     (int32_t*)nullptr);
  return hipGetLastError();
}

constexpr auto no_refusals = [] { return (int)SMI_OK; };
inline auto keys_refusals(const IvfKeys* keys) {
  return [keys] { return keys ? check_keys(*keys) : (int)SMI_OK; };
}
// How a search kind keeps the k results of a pair: the most k and nprobe it takes, with_key_list(k, launch) = launch(KT as a
// std::integral_constant), KT the key-list length of its scan for k results, and the merge of the nprobe partial lists.
struct ProbeLimits {
  int k, nprobe;  // k = 0: an entry without k (the range search)
};
struct TopkLists {  // lists of 1, 2, 4 or 8 keys in registers
  static constexpr ProbeLimits limits{8, 8};
  static constexpr auto merge = launch_topk_merge;
  template <class Launch>
  static hipError_t with_key_list(int k, Launch launch) {
    if (k == 1) return launch(std::integral_constant<int, 1>{});
    if (k == 2) return launch(std::integral_constant<int, 2>{});
    if (k <= 4) return launch(std::integral_constant<int, 4>{});
    return launch(std::integral_constant<int, 8>{});
  }
};
struct PageLists {  // a page of IVF_PAGE keys, whatever k
  static constexpr ProbeLimits limits{IVF_PAGE, 64};
  static constexpr auto merge = launch_topk_merge_page;
  template <class Launch>
  static hipError_t with_key_list(int, Launch launch) {
    return launch(std::integral_constant<int, IVF_PAGE>{});
  }
};
// the shape refusals of every entry over nq queries with nprobe probes each: the search, the page and the range search
int check_search_args(int64_t nq, int32_t d, int64_t K, int32_t nprobe, int32_t k, ProbeLimits most = TopkLists::limits) {
  if (const int rc = check_shape(nq, "nq", d, K, "list")) return rc;
  if (most.k && (k < 1 || k > most.k)) return fail(SMI_ERR_INVALID_ARG, "k=%d must be in [1, %d]", k, most.k);
  if (nprobe < 1 || nprobe > most.nprobe)
    return fail(SMI_ERR_INVALID_ARG, "nprobe=%d must be in [1, %d]", nprobe, most.nprobe);
  if (nq * nprobe > IVF_MAX) return fail(SMI_ERR_UNSUPPORTED, "nq * nprobe = %lld must fit int32", (long long)(nq * nprobe));
  return SMI_OK;
}

// invert the probe table: the (query, probe slot) pairs q * nprobe + p bucketed by the list they name, the units' prefix
// sum for `unit` pairs per unit, and (k > 0) the partial lists pre-filled
hipError_t invert_probes(const int32_t* probes, int64_t P, int64_t K, int k, int unit, const SearchWs& w, hipStream_t st) {
  if (hipError_t e = hipMemsetAsync(w.pcount, 0, (size_t)K * 4, st); e != hipSuccess) return e;
  const dim3 block(IVF_TB), pair_grid = grid_for(P, IVF_TB);
  hipLaunchKernelGGL(bucket_hist_kernel<IVF_TB>, pair_grid, block, 0, st, probes, (int)P, (int)K, w.pcount);
  hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), block, 0, st, w.pcount, (int)K, 1, unit, w.poff, w.cursor, w.ubase);
  hipLaunchKernelGGL(bucket_scatter_kernel<IVF_TB>, pair_grid, block, 0, st, probes, (int)P, (int)K, w.cursor, w.pairs,
                     (int32_t*)nullptr);
  if (k > 0) hipLaunchKernelGGL(ivf_fill_kernel, grid_for(P * k, IVF_TB), block, 0, st, w.ps, w.pi, P * k);
  return hipGetLastError();
}

// A build entry, stated once.  The kind gives: whether a pointer of its own is null, the name of its sizing function, its own
// refusals (they follow check_build_args) and gather(grid, st), the launch of one wave per slot any labelling can need:
// the waves from list_offsets[K] on find nothing to do.
template <class Refusals, class Gather>
int build_entry(bool null_arg, const int32_t* labels, int64_t n, int32_t d, int64_t K, int32_t* list_ids, int64_t capacity_slots,
                int32_t* list_offsets, int32_t* list_sizes, void* ws, int64_t ws_bytes, void* stream, const char* sizing,
                Refusals refusals, Gather gather) {
  if (null_arg || !labels || !list_ids || !list_offsets || !list_sizes) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_build_args(n, d, K, capacity_slots, ws, ws_bytes, sizing)) return rc;
  if (const int rc = refusals()) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(bucket_rows(labels, n, K, list_ids, capacity_slots, list_offsets, list_sizes, BuildWs(ws, K).cursor, st));
  gather(grid_for(slots_bound(n, K), IVF_TB / 64), st);
  HIP_TRY(hipGetLastError());
  return SMI_OK;
}

// A search entry, stated once.  Lists: how the kind keeps its results (above).  The kind gives: whether a pointer of its own is
// null, the refusals of its further arguments (keys_refusals of a keyed entry, DESIGN.md 3.24, whose scan hands the keys to
// launch_units_keyed; the ceilings of a page), the name of its sizing function, the i8_dim and ceil_rows of its workspace,
// its own refusals on shape (they follow check_search_args), prepare(w, st), what it enqueues in front of the inversion (the
// int8 search encodes its queries there, the page its ceiling keys), and scan(kt, unit, units, w, st), the launch of its
// list-walking kernel with key lists of decltype(kt)::value over units for every pair count the table can have: those from
// ubase[K] on find nothing to do.
template <class Lists = TopkLists, class ArgRefusals, class Refusals, class Prepare, class Scan>
int search_entry(bool null_arg, ArgRefusals arg_refusals, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                 const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* ws,
                 int64_t ws_bytes, void* stream, const char* sizing, int i8_dim, int64_t ceil_rows, Refusals refusals,
                 Prepare prepare, Scan scan) {
  if (null_arg || !probes || !list_ids || !list_offsets || !idx || !score) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = arg_refusals()) return rc;
  if (const int rc = check_search_args(nq, d, K, nprobe, k, Lists::limits)) return rc;
  if (const int rc = refusals()) return rc;
  const int64_t P = nq * nprobe;
  const SearchWs w(ws, nq, K, nprobe, k, i8_dim, ceil_rows);
  if (const int rc = check_ws(ws, ws_bytes, w.bytes(), sizing)) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(prepare(w, st));
  // one unit rule for every kind: the image and the MFMA work of a PQ unit are the flat unit's, and on int8 lists 128 won
  // from 256 pairs per list on and 64 below as well (profiles/ivf_i8_experiments.txt)
  const int unit = unit_pairs(P, K);
  HIP_TRY(invert_probes(probes, P, K, k, unit, w, st));
  const int64_t units = units_bound(P, K, unit);
  HIP_TRY(Lists::with_key_list(k, [&](auto kt) { return scan(kt, unit, units, w, st); }));
  HIP_TRY(Lists::merge(w.ps, w.pi, nprobe, nq, k, score, idx, st));
  return SMI_OK;
}
constexpr auto no_prepare = [](const SearchWs&, hipStream_t) { return hipSuccess; };

// The two passes of the range search, stated once.  Its workspace is the search's with k = 0: the inverted
// probe table and no partial lists.  `emit` (pair_base non-null) trusts the workspace as `count` left it.
int check_range_shape(int64_t nq, int32_t d, int64_t K, int32_t nprobe) { return check_search_args(nq, d, K, nprobe, 0, {0, 8}); }
int range_entry(bool null_arg, const IvfKeys* keys, const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                const float* threshold, const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets, int64_t K,
                int32_t* pair_counts, const int64_t* pair_base, int64_t total, float* score, int32_t* idx, void* ws,
                int64_t ws_bytes, void* stream) {
  if (null_arg || !qn || !probes || !threshold || !list_rows || !list_ids || !list_offsets)
    return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (keys)
    if (const int rc = check_keys(*keys)) return rc;
  if (const int rc = check_range_shape(nq, d, K, nprobe)) return rc;
  const int64_t P = nq * nprobe;
  const SearchWs w(ws, nq, K, nprobe, 0);
  if (const int rc = check_ws(ws, ws_bytes, w.bytes(), "smi_range_search_ws_bytes(nq, K, nprobe, d)")) return rc;
  if (pair_base && total < 0) return fail(SMI_ERR_INVALID_ARG, "total=%lld: the last entry of pair_base", (long long)total);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t st = (hipStream_t)stream;
  const int unit = unit_pairs(P, K);  // the search's rule, a function of the shapes: both passes walk the same units
  const int64_t units = units_bound(P, K, unit);
  const auto walk = [&](auto emit) {
    constexpr bool EMIT = decltype(emit)::value;
    return launch_units_keyed<ivf_range_lists_kernel<IVF_BM, EMIT>, ivf_range_lists_kernel<IVF_BIG, EMIT>,
                              ivf_range_lists_kernel_keyed<IVF_BM, EMIT>, ivf_range_lists_kernel_keyed<IVF_BIG, EMIT>>(
        keys, unit, units, ivf_range_lds<IVF_BM>(), ivf_range_lds<IVF_BIG>(), st, (const f16*)qn, d, nprobe, threshold,
        (const f16*)list_rows, list_ids, list_offsets, (int)K, (const int32_t*)w.poff, (const int32_t*)w.ubase,
        (const int32_t*)w.pairs, pair_counts, pair_base, total, score, idx);
  };
  if (pair_base) {
    HIP_TRY(walk(std::true_type{}));
    return SMI_OK;
  }
  // a pair that names no list is in no unit: its count reads 0
  HIP_TRY(hipMemsetAsync(pair_counts, 0, (size_t)P * 4, st));
  HIP_TRY(invert_probes(probes, P, K, 0, unit, w, st));
  HIP_TRY(walk(std::false_type{}));
  return SMI_OK;
}

// A one-kernel entry over n rows of d fp16 (the encoders, the decoder, the residuals), stated once: null pointers, the
// alignment of the output `name` (out16; null where the kernel does not need it), check_shape, the kind's own refusals, the
// device, the launch.
template <class Refusals, class Launch>
int rows_entry(bool null_arg, const void* out16, const char* name, int64_t n, int32_t d, Refusals refusals, Launch launch) {
  if (null_arg) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if ((uintptr_t)out16 % 16) return fail(SMI_ERR_INVALID_ARG, "%s must be 16-byte aligned", name);
  if (const int rc = check_shape(n, "n", d, 1, "list")) return rc;
  if (const int rc = refusals()) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  launch();
  HIP_TRY(hipGetLastError());
  return SMI_OK;
}

// ================================================================ semantic de-duplication
// The per-list self-join of SemDeDup over the flat lists: for every row, the best score against the rows of its own list
// that PRECEDE it in a keep order (higher priority first, ties to the lower original id).  The queries are the list rows
// themselves, so nothing is gathered by index and no probe table is inverted: a unit is one list and B consecutive slots of
// it (its own rows, the MFMA B operand) and walks the whole list in tiles of B slots (the A operand) with the slice loop of
// ivf_scan.hpp, so a score has the bits smi_ivf_search returns for the same two rows.  What it adds is
// the fold: one 64-bit key per own row and lane, in registers, which a candidate enters iff it is a row (id >= 0) and
// precedes the own row; and the join of those keys at the end of the walk.
// A COPY: the kernel spells ivf_slice_walk's loop out (lds_off to the barrier at the loop's end; keep the two texts the same).
// As an instance of the function hipcc waits for the prefetched slice before the MFMAs of the current one in the
// 128-row kernel, whichever way the fold was written (profiles/isa_identity_ivf.txt), so the loop keeps its text here.

// span[l] = off[l + 1] - off[l]: the padded size of every list, what the unit prefix scan counts
__global__ __launch_bounds__(IVF_TB) void ivf_span_kernel(const int32_t* __restrict__ off, int K, int32_t* __restrict__ span) {
  const int64_t l = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  if (l < K) span[l] = off[l + 1] - off[l];
}

// sprio[slot] = priority[ids[slot]] for the slots in use: the priorities in slot order, once per call.  0 for a pad slot
// (never compared) and for every slot when there is no priority (all equal: the id decides).
__global__ __launch_bounds__(IVF_TB) void ivf_slot_priority_kernel(const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ off, int K,
                                                                   const float* __restrict__ priority, int n,
                                                                   float* __restrict__ sprio) {
  const int64_t slot = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  if (slot >= off[K]) return;
  const int id = ids[slot];
  sprio[slot] = priority && id >= 0 && id < n ? priority[id] : 0.f;  // an id outside [0, n) breaks the contract: not read
}

// The row filter of a search, in slot order, once per filter: fid[slot] = ids[slot] where the row is visible
// (mask null, or mask[id] != 0), else -1 -- the "effective id" array every scan runs on unchanged, since a slot whose id is
// -1 never enters -- and skey[slot] (nullable) = keys[id].  One thread per slot of the storage: a pad slot and a slot from
// off[K] on get id -1 and key 0; an id outside [0, n) of the given tensors is treated as masked out and never read.
__global__ __launch_bounds__(IVF_TB) void ivf_slot_filter_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ off,
                                                                 int K, const int32_t* __restrict__ keys,
                                                                 const uint8_t* __restrict__ mask, int64_t n,
                                                                 int64_t slots, int32_t* __restrict__ fid,
                                                                 int32_t* __restrict__ skey) {
  const int64_t slot = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  if (slot >= slots) return;
  const int id = slot < off[K] ? ids[slot] : -1;
  const bool seen = id >= 0 && id < n && (!mask || mask[id] != 0);
  fid[slot] = seen ? id : -1;
  if (skey) skey[slot] = seen && keys ? keys[id] : 0;
}

template <int B>
constexpr int ivf_selfjoin_lds() { return 2 * 2 * B * IVF_SLICE + B * 8; }

// Workgroup b = unit b - ubase[l] of the list l with ubase[l] <= b < ubase[l + 1]: own slots off[l] + B * that .. against
// the slots off[l] .. off[l + 1].  Lane (l15, kg) of wave (wr, wc) holds own row wc * B / 2 + bi * 16 + l15 x candidate
// slots wr * B / 2 + ai * 16 + 4 kg + r of the tile: the best key of an own row is spread over 4 lanes of 2 waves until the
// end of the walk, where two shuffles and one LDS max per wave join it.
template <int B>
__global__ __launch_bounds__(IVF_TB) void ivf_selfjoin_kernel(const f16* __restrict__ rows, int d,
                                                              const int32_t* __restrict__ ids,
                                                              const float* __restrict__ sprio,
                                                              const int32_t* __restrict__ off, int K,
                                                              const int32_t* __restrict__ ubase, int n,
                                                              float* __restrict__ max_sim, int32_t* __restrict__ nearest) {
  constexpr int OPB = B * IVF_BK * 2;  // bytes of one operand's K slice
  constexpr int NR = B / 32;           // rows of an operand slice a thread loads; 16-row blocks of a wave per operand
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* sbest = (unsigned long long*)(smem + 4 * OPB);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kg = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int b = blockIdx.x;
  if (b >= ubase[K]) return;
  const int l = ivf_unit_list(ubase, K, b);
  const int s_begin = off[l], s_end = off[l + 1];
  const int u0 = s_begin + (b - ubase[l]) * B;  // < s_end: the list has ceil((s_end - s_begin) / B) units
  const int nown = min(B, s_end - u0);          // a multiple of 16

  if (tid < B) sbest[tid] = XS_EMPTY;

  const int nk = d / IVF_BK;
  const int ntiles = (s_end - s_begin + B - 1) / B;
  const int T = ntiles * nk;

  // this thread's rows of a slice, and where its chunk lands in LDS
  const int cc = tid & 7;
  const f16* qsrc[NR];
  int lds_off[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int r = (tid >> 3) + 32 * j;
    qsrc[j] = r < nown ? rows + (size_t)(u0 + r) * d + cc * 8 : nullptr;
    lds_off[j] = r * (IVF_BK * 2) + ((cc ^ (r & 7)) << 4);
  }
  u32x4 qv[NR], lv[NR];
  auto load = [&](int it) {
    const int tile = it / nk, ks = it - tile * nk;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int slot = s_begin + tile * B + (tid >> 3) + 32 * j;
      qv[j] = qsrc[j] ? *(const u32x4*)(qsrc[j] + ks * IVF_BK) : u32x4{0u, 0u, 0u, 0u};
      lv[j] = slot < s_end ? *(const u32x4*)(rows + (size_t)slot * d + ks * IVF_BK + cc * 8) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      *(u32x4*)(smem + buf * 2 * OPB + lds_off[j]) = qv[j];
      *(u32x4*)(smem + buf * 2 * OPB + OPB + lds_off[j]) = lv[j];
    }
  };

  f32x4 acc[NR][NR];  // [candidate block ai][own block bi]
#pragma unroll
  for (int ai = 0; ai < NR; ++ai)
#pragma unroll
    for (int bi = 0; bi < NR; ++bi) acc[ai][bi] = f32x4{0.f, 0.f, 0.f, 0.f};
  // 16-row blocks of this wave that hold an own slot at all (wave-uniform)
  const int nb_live = min(NR, max(0, (nown - wc * (B / 2)) / 16));
  // this lane's own rows: id (-1: a pad slot, or no slot), priority, best key so far
  int own_id[NR];
  float own_p[NR];
  unsigned long long best[NR];
#pragma unroll
  for (int bi = 0; bi < NR; ++bi) {
    const int pr = wc * (B / 2) + bi * 16 + l15;
    own_id[bi] = pr < nown ? ids[u0 + pr] : -1;
    own_p[bi] = pr < nown ? sprio[u0 + pr] : 0.f;
    best[bi] = XS_EMPTY;
  }

  load(0);  // T > 0: a list with a unit has a slot
  store(0);
  __syncthreads();
  int ks = 0, tile = 0;
  for (int it = 0; it < T; ++it) {
    const int buf = it & 1;
    if (it + 1 < T) load(it + 1);
    // 16-slot blocks of this wave below the end of the list (the lists are padded to 16 slots): wave-uniform
    const int slot_w = s_begin + tile * B + wr * (B / 2);
    const int na_live = min(NR, max(0, (s_end - slot_w) / 16));
    if (na_live > 0 && nb_live > 0) {
      const char* qs = smem + buf * 2 * OPB;
      const char* ls = qs + OPB;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ch = kk * 4 + kg;
        half8 fa[NR], fb[NR];
#pragma unroll
        for (int ai = 0; ai < NR; ++ai) {
          const int ra = wr * (B / 2) + ai * 16 + l15;
          fa[ai] = *(const half8*)(ls + ra * (IVF_BK * 2) + ((ch ^ (ra & 7)) << 4));
        }
#pragma unroll
        for (int bi = 0; bi < NR; ++bi) {
          const int rb = wc * (B / 2) + bi * 16 + l15;
          fb[bi] = *(const half8*)(qs + rb * (IVF_BK * 2) + ((ch ^ (rb & 7)) << 4));
        }
#pragma unroll
        for (int ai = 0; ai < NR; ++ai)
          if (ai < na_live) {
#pragma unroll
            for (int bi = 0; bi < NR; ++bi)
              if (bi < nb_live) acc[ai][bi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[ai], fb[bi], acc[ai][bi], 0, 0, 0);
          }
      }
    }
    if (it + 1 < T) store(buf ^ 1);
    if (++ks == nk) {
      // the tile is finished: a candidate enters the own row's key iff it is a row and precedes the own row
#pragma unroll
      for (int ai = 0; ai < NR; ++ai) {
        if (ai < na_live && nb_live > 0) {
          const int slot0 = slot_w + ai * 16 + 4 * kg;  // < s_end, 16-byte aligned: off % 16 == 0
          const int4 id4 = *(const int4*)(ids + slot0);
          const float4 p4 = *(const float4*)(sprio + slot0);
          const int idr[4] = {id4.x, id4.y, id4.z, id4.w};
          const float prr[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
          for (int bi = 0; bi < NR; ++bi) {
            const int oid = own_id[bi];
            const float op = own_p[bi];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool precedes = idr[r] >= 0 && oid >= 0 && (prr[r] > op || (prr[r] == op && idr[r] < oid));
              const unsigned long long key = xs_key(acc[ai][bi][r], idr[r]);
              if (precedes && key > best[bi]) best[bi] = key;
            }
          }
        }
#pragma unroll
        for (int bi = 0; bi < NR; ++bi) acc[ai][bi] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      ks = 0;
      ++tile;
    }
    __syncthreads();
  }

  // join the 4 kg lanes of an own row, then the two wr waves (sbest was initialised before the loop's barriers)
#pragma unroll
  for (int bi = 0; bi < NR; ++bi) {
    unsigned long long k = best[bi];
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const unsigned long long other = __shfl_xor(k, o, 64);
      k = other > k ? other : k;
    }
    if (kg == 0 && k != XS_EMPTY)
      __hip_atomic_fetch_max(sbest + wc * (B / 2) + bi * 16 + l15, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  // the unit owns its rows: no atomics on results.  A row nothing precedes keeps the pre-filled (-inf, -1).
  if (tid < nown) {
    const int id = ids[u0 + tid];
    const unsigned long long key = sbest[tid];
    if (id >= 0 && id < n && key != XS_EMPTY) {  // (an id outside [0, n) breaks the contract: nothing is written through it)
      max_sim[id] = xs_key_value(key);
      nearest[id] = xs_key_index(key);
    }
  }
}

int check_dedup_shape(int64_t slots, int64_t n, int64_t K, int32_t d) {
  if (const int rc = check_shape(n, "n", d, K, "list")) return rc;
  if (slots < 1) return fail(SMI_ERR_INVALID_ARG, "slots=%lld: empty storage", (long long)slots);
  if (slots > IVF_MAX) return fail(SMI_ERR_UNSUPPORTED, "slots=%lld: slot numbers must fit int32", (long long)slots);
  if (slots % IVF_ALIGN)
    return fail(SMI_ERR_INVALID_ARG, "slots=%lld must be a multiple of %d, as smi_ivf_build's storage is", (long long)slots,
                IVF_ALIGN);
  if (slots / IVF_BM + K > IVF_MAX)
    return fail(SMI_ERR_UNSUPPORTED, "slots=%lld, K=%lld: the unit count must fit int32", (long long)slots, (long long)K);
  return SMI_OK;
}
// dedup: padded list sizes [K] | their prefix sum [K + 1] (the scan's first output: list_offsets again) | unit offsets
//        [K + 1] | cursor [K] | priorities in slot order fp32 [slots]
struct DedupWs : WsLayout {
  int32_t *span, *span_off, *ubase, *cursor;
  float* sprio;
  DedupWs(void* ws, int64_t slots, int64_t K) : WsLayout(ws) {
    span = take<int32_t>(K, 16);
    span_off = take<int32_t>(K + 1, 16);
    ubase = take<int32_t>(K + 1, 16);
    cursor = take<int32_t>(K, 16);
    sprio = take<float>(slots, 16);
  }
};

// ================================================================ product-quantised lists
// The same lists with one byte per sub-quantiser and row: d = M * dsub, M sub-quantisers of PQ_CW = 256 codewords each,
// codebooks fp16 [M][256][dsub], a code row uint8 [M].  The bucketing, the unit rule, the key lists and the merge above are
// called.  New: the product quantiser (encode, train, decode), the gather that encodes, and a scan whose fetch decodes a
// tile's codes into the slice loop's LDS image once per tile and K slice: the loop is ivf_scan_lists_kernel's, so a score
// has the bits smi_ivf_search returns against the decoded row.
constexpr int PQ_ROWS = 2048;  // rows one block of the training update takes of one sub-quantiser

int pq_check_dsub(int32_t d, int32_t dsub) {  // behind check_shape: d > 0
  if (dsub != 8 && dsub != 16 && dsub != 32 && dsub != 64)
    return fail(SMI_ERR_UNSUPPORTED, "dsub=%d must be 8, 16, 32 or 64", dsub);
  if (d % dsub) return fail(SMI_ERR_UNSUPPORTED, "dsub=%d does not divide d=%d", dsub, d);
  return SMI_OK;
}
// the refusals every entry that is given codebooks starts its own with: dsub, then the pointer
int pq_check_codebooks(int32_t d, int32_t dsub, const void* cb) {
  if (const int rc = pq_check_dsub(d, dsub)) return rc;
  if (!cb) return fail(SMI_ERR_INVALID_ARG, "null codebooks");
  if ((uintptr_t)cb % 16) return fail(SMI_ERR_INVALID_ARG, "codebooks must be 16-byte aligned");
  return SMI_OK;
}
int pq_shift(int dsub) { return dsub == 8 ? 3 : dsub == 16 ? 4 : dsub == 32 ? 5 : 6; }

// Residual encoding: a row is quantised as its difference from the centroid of its list.  THE residual
// element, wherever one is formed: fp16_rn(fp32_rn((float)x - (float)c)), two roundings to nearest even (the bits of numpy's
// (x.astype(f32) - c.astype(f32)).astype(f16)).
__device__ __forceinline__ f16 pq_residual(f16 x, f16 c) { return (f16)((float)x - (float)c); }
__device__ __forceinline__ half8 pq_residual8(half8 x, half8 c) {
  half8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = pq_residual(x[e], c[e]);
  return r;
}
// the centroid row a label names, or null: a label outside [0, K) addresses nothing and the residual is the row itself
__device__ __forceinline__ const f16* pq_centroid_row(const f16* __restrict__ cent, int K, int d, int label) {
  return (unsigned)label < (unsigned)K ? cent + (size_t)label * d : nullptr;
}
// 8 elements at x + k against the same 8 of the centroid row c (null: none)
__device__ __forceinline__ half8 pq_residual_chunk(const f16* __restrict__ x, const f16* __restrict__ c, int k) {
  const half8 h = *(const half8*)(x + k);
  return c ? pq_residual8(h, *(const half8*)(c + k)) : h;
}

// The key of subvector x against the codeword at cw, the contract's chain: n2 = c_0 c_0 + c_1 c_1 + ... ascending (the
// product of two fp16 is exact in fp32, so fmaf(c, c, n2) is the rounded add of the header), bias = -0.5 n2 (exact),
// key = fmaf(x_j, c_j, key) ascending from the bias.  The largest key is the Euclidean nearest codeword.
template <int DSUB>
__device__ __forceinline__ float pq_key(const half8 (&x)[DSUB / 8], const f16* __restrict__ cw) {
  half8 c[DSUB / 8];
#pragma unroll
  for (int ch = 0; ch < DSUB / 8; ++ch) c[ch] = *(const half8*)(cw + ch * 8);
  float n2 = 0.f;
#pragma unroll
  for (int ch = 0; ch < DSUB / 8; ++ch)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float cf = (float)c[ch][e];
      n2 = __fmaf_rn(cf, cf, n2);
    }
  float key = -0.5f * n2;
#pragma unroll
  for (int ch = 0; ch < DSUB / 8; ++ch)
#pragma unroll
    for (int e = 0; e < 8; ++e) key = __fmaf_rn((float)x[ch][e], (float)c[ch][e], key);
  return key;
}

// THE row encoder, one wave per row (every lane of the wave calls it): codes[0 .. d / DSUB) of the d fp16 at x.  Lane l
// scores the codewords l, l + 64, l + 128, l + 192 of a sub-quantiser (ascending, a later one must beat the earlier), a
// butterfly takes the largest key of the wave, ties to the lower code, and leaves it in every lane; lane m % 64 keeps
// the code of sub-quantiser m and the wave stores 64 consecutive code bytes at a time.  RES: what is encoded is the residual
// of x against the centroid row c (null: x itself).
template <int DSUB, bool RES = false>
__device__ __forceinline__ void pq_encode_row_t(const f16* __restrict__ x, int d, const f16* __restrict__ cb, int lane,
                                                uint8_t* __restrict__ codes, const f16* __restrict__ c = nullptr) {
  const int M = d / DSUB;
  int mine = 0;
  for (int m = 0; m < M; ++m) {
    half8 xs[DSUB / 8];
#pragma unroll
    for (int ch = 0; ch < DSUB / 8; ++ch) {
      if constexpr (RES) xs[ch] = pq_residual_chunk(x, c, m * DSUB + ch * 8);
      else xs[ch] = *(const half8*)(x + m * DSUB + ch * 8);
    }
    const f16* cm = cb + (size_t)m * PQ_CW * DSUB;
    float best = pq_key<DSUB>(xs, cm + (size_t)lane * DSUB);
    int bc = lane;
#pragma unroll
    for (int i = 1; i < PQ_CW / 64; ++i) {
      const int c = i * 64 + lane;
      const float key = pq_key<DSUB>(xs, cm + (size_t)c * DSUB);
      if (key > best) {
        best = key;
        bc = c;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ok = __shfl_xor(best, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (ok > best || (ok == best && oc < bc)) {
        best = ok;
        bc = oc;
      }
    }
    if (lane == (m & 63)) mine = bc;
    if ((m & 63) == 63 || m == M - 1) {
      if (lane <= (m & 63)) codes[(m & ~63) + lane] = (uint8_t)mine;
    }
  }
}

__device__ __forceinline__ void pq_encode_row(const f16* __restrict__ x, int d, int dsub, const f16* __restrict__ cb, int lane,
                                              uint8_t* __restrict__ codes) {
  switch (dsub) {  // wave-uniform
    case 8: pq_encode_row_t<8>(x, d, cb, lane, codes); break;
    case 16: pq_encode_row_t<16>(x, d, cb, lane, codes); break;
    case 32: pq_encode_row_t<32>(x, d, cb, lane, codes); break;
    default: pq_encode_row_t<64>(x, d, cb, lane, codes); break;
  }
}

__global__ __launch_bounds__(IVF_TB) void pq_encode_kernel(const f16* __restrict__ xn, int64_t n, int d, int dsub,
                                                           const f16* __restrict__ cb, uint8_t* __restrict__ codes) {
  const int64_t row = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  pq_encode_row(xn + (size_t)row * d, d, dsub, cb, threadIdx.x & 63, codes + (size_t)row * (d / dsub));
}
// The same on the residual of row `row` against the centroid labels[row] names.  The residual kernels take dsub as a template
// argument, chosen by the host: behind the in-kernel switch every dsub pays the registers of dsub = 64, and with the centroid's
// chunks on top of the row's that was 200 VGPRs and one wave per SIMD less than the plain encoder (tools/kernel_resources.py).
template <int DSUB>
__global__ __launch_bounds__(IVF_TB) void pq_encode_residual_kernel(const f16* __restrict__ xn, int64_t n, int d,
                                                                    const f16* __restrict__ cb, uint8_t* __restrict__ codes,
                                                                    const int32_t* __restrict__ labels,
                                                                    const f16* __restrict__ cent, int K) {
  const int64_t row = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform
  pq_encode_row_t<DSUB, true>(xn + (size_t)row * d, d, cb, threadIdx.x & 63, codes + (size_t)row * (d / DSUB),
                              pq_centroid_row(cent, K, d, labels[row]));
}

// out[r] = the residual of row r: one thread per 16 bytes of output
__global__ __launch_bounds__(IVF_TB) void pq_residuals_kernel(const f16* __restrict__ xn, int64_t n, int d,
                                                              const int32_t* __restrict__ labels,
                                                              const f16* __restrict__ cent, int K, f16* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  const int cpr = d / 8;
  if (t >= n * cpr) return;
  const int64_t r = t / cpr;
  const int k0 = (int)(t - r * cpr) * 8;
  *(half8*)(out + (size_t)t * 8) = pq_residual_chunk(xn + (size_t)r * d, pq_centroid_row(cent, K, d, labels[r]), k0);
}

// rows[r] = the concatenation of the codewords codes[r] names: one thread per 16 bytes of output
__global__ __launch_bounds__(IVF_TB) void pq_decode_kernel(const uint8_t* __restrict__ codes, int64_t n, int d, int dsub,
                                                           const f16* __restrict__ cb, f16* __restrict__ rows) {
  const int64_t t = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  const int cpr = d / 8;
  if (t >= n * cpr) return;
  const int64_t r = t / cpr;
  const int k0 = (int)(t - r * cpr) * 8, m = k0 / dsub;
  const int code = codes[(size_t)r * (d / dsub) + m];
  *(u32x4*)(rows + (size_t)t * 8) = *(const u32x4*)(cb + ((size_t)m * PQ_CW + code) * dsub + k0 % dsub);
}

// training, the start: codeword c of every sub-quantiser = that subvector of row init[c] (RES: of its residual against the
// centroid labels[init[c]] names).  One thread per 16 bytes.
template <bool RES>
__global__ __launch_bounds__(IVF_TB) void pq_init_kernel(const f16* __restrict__ xn, int d, int dsub,
                                                         const int32_t* __restrict__ init, f16* __restrict__ cb,
                                                         const int32_t* __restrict__ labels, const f16* __restrict__ cent,
                                                         int K) {
  const int t = blockIdx.x * IVF_TB + threadIdx.x;  // < 256 * d / 8
  if (t >= PQ_CW * (d / 8)) return;
  const int cpc = dsub / 8, cw = t / cpc, ch = t - cw * cpc;
  const int m = cw / PQ_CW, c = cw - m * PQ_CW;
  const int row = init[c];
  if constexpr (RES) {
    *(half8*)(cb + (size_t)t * 8) =
        pq_residual_chunk(xn + (size_t)row * d, pq_centroid_row(cent, K, d, labels[row]), m * dsub + ch * 8);
  } else {
    *(u32x4*)(cb + (size_t)t * 8) = *(const u32x4*)(xn + (size_t)row * d + m * dsub + ch * 8);
  }
}

// training, the update: block (row block rb, sub-quantiser m) = blockIdx.x adds the subvectors m of its PQ_ROWS rows, as
// int64 in units of 2^-24 (exact in any order: kmeans.hip), into LDS sums [256][DSUB] and counts [256] with LDS integer
// atomics, and flushes what is not zero with global integer atomics.  LDS: 2 KB * DSUB + 1 KB, 129 KB at DSUB = 64.
template <int DSUB>
constexpr int pq_accumulate_lds() { return PQ_CW * DSUB * 8 + PQ_CW * 4; }

// RES: what is added is the residual of the row against the centroid its label names.
template <int DSUB, bool RES>
__global__ __launch_bounds__(IVF_TB) void pq_accumulate_kernel(const f16* __restrict__ xn, int64_t n, int d,
                                                               const uint8_t* __restrict__ codes,
                                                               unsigned long long* __restrict__ sums,
                                                               int32_t* __restrict__ counts,
                                                               const int32_t* __restrict__ labels,
                                                               const f16* __restrict__ cent, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* ls = (unsigned long long*)smem;
  int* lc = (int*)(smem + PQ_CW * DSUB * 8);
  const int M = d / DSUB, tid = threadIdx.x;
  const int m = blockIdx.x % M;
  const int64_t r0 = (int64_t)(blockIdx.x / M) * PQ_ROWS;
  const int64_t r1 = r0 + PQ_ROWS < n ? r0 + PQ_ROWS : n;
  for (int i = tid; i < PQ_CW * DSUB; i += IVF_TB) ls[i] = 0ull;
  lc[tid] = 0;  // IVF_TB == PQ_CW
  __syncthreads();
  for (int64_t r = r0 + tid; r < r1; r += IVF_TB) {
    const int code = codes[(size_t)r * M + m];
    atomicAdd(lc + code, 1);
    const f16* x = xn + (size_t)r * d + m * DSUB;
    const f16* c = nullptr;
    if constexpr (RES) {
      c = pq_centroid_row(cent, K, d, labels[r]);
      if (c) c += m * DSUB;
    }
#pragma unroll
    for (int ch = 0; ch < DSUB / 8; ++ch) {
      half8 h;
      if constexpr (RES) h = pq_residual_chunk(x, c, ch * 8);
      else h = *(const half8*)(x + ch * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const long long v = (long long)((float)h[e] * 0x1p24f);  // exact: an fp16 is a multiple of 2^-24 below 2^40
        if (v != 0) atomicAdd(ls + code * DSUB + ch * 8 + e, (unsigned long long)v);
      }
    }
  }
  __syncthreads();
  unsigned long long* gs = sums + (size_t)m * PQ_CW * DSUB;
  for (int i = tid; i < PQ_CW * DSUB; i += IVF_TB) {
    const unsigned long long v = ls[i];
    if (v != 0ull) atomicAdd(gs + i, v);
  }
  if (lc[tid] != 0) atomicAdd(counts + m * PQ_CW + tid, lc[tid]);
}
static_assert(IVF_TB == PQ_CW, "one thread per codeword count");

// training, the finalise: c_j = fp16_rn(fdiv_rn((float)S, (float)count) * 2^-24), the conversions and the division to
// nearest even, the scaling exact; a codeword with no member keeps its value.  One thread per element.
__global__ __launch_bounds__(IVF_TB) void pq_finalize_kernel(const long long* __restrict__ sums,
                                                             const int32_t* __restrict__ counts, int d, int dsub,
                                                             f16* __restrict__ cb) {
  const int t = blockIdx.x * IVF_TB + threadIdx.x;
  if (t >= PQ_CW * d) return;
  const int count = counts[t / dsub];
  if (count > 0) cb[t] = (f16)(__fdiv_rn(__ll2float_rn(sums[t]), (float)count) * 0x1p-24f);
}

// One wave per slot below off[K]: the codes of the row ids[slot] names, or zero codes for a pad slot.  RES_DSUB = 0: the plain
// gather, dsub at run time; RES_DSUB = dsub: the codes of the row's residual against the centroid its label names, which is
// the centroid of the slot's list.
template <int RES_DSUB>
__global__ __launch_bounds__(IVF_TB) void ivf_pq_gather_kernel(const f16* __restrict__ xn, int d, int dsub,
                                                               const f16* __restrict__ cb, const int32_t* __restrict__ ids,
                                                               const int32_t* __restrict__ off, int K,
                                                               uint8_t* __restrict__ codes,
                                                               const int32_t* __restrict__ labels,
                                                               const f16* __restrict__ cent) {
  const int lane = threadIdx.x & 63, M = d / dsub;
  const int64_t slot = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (slot >= off[K]) return;  // wave-uniform
  const int id = ids[slot];
  if (id < 0) {
    for (int m = lane; m < M; m += 64) codes[(size_t)slot * M + m] = 0;
  } else if constexpr (RES_DSUB != 0) {
    pq_encode_row_t<RES_DSUB, true>(xn + (size_t)id * d, d, cb, lane, codes + (size_t)slot * M,
                                    pq_centroid_row(cent, K, d, labels[id]));
  } else {
    pq_encode_row(xn + (size_t)id * d, d, dsub, cb, lane, codes + (size_t)slot * M);
  }
}

// ivf_scan_lists_kernel's unit on product-quantised lists.  What it adds is where the list operand's slice comes from: thread
// (row r, chunk cc) of slice ks owns the dimensions ks * 64 + cc * 8 .. + 8, reads the code byte of sub-quantiser
// m = (ks * 64 + cc * 8) / dsub of its slot and gathers 16 bytes of that codeword from the codebooks (256 * d * 2 bytes,
// which stay in L2).  Code -> codeword is two dependent round trips and one slice of prefetch covers one, so the code
// bytes are fetched a slice further ahead than the codewords: `fetch(it)` gathers with the codes an earlier call left in
// cd and fetches those of slice it + 1.  Slots at or past the end of the list are zero-filled without touching the codes;
// a pad slot (codes 0) decodes codeword 0 of every sub-quantiser and is skipped by the fold (id -1).
// RES (3.22): the rows are residuals against their list's centroid and a score is fl32(sum + coarse[pair]), coarse fp32
// [nq][nprobe] = the query's score against that centroid: a pair's value is kept in a float [B] behind the pair numbers in
// LDS and added where a sum meets the fold.
template <int B>
constexpr int ivf_pq_residual_scan_lds(int KT) { return ivf_scan_lds<B>(KT) + B * 4; }

// (the kernel, ivf_pq_scan_lists_kernel<KT, B, RES>, and its keyed twin: ivf_list_kernels.hpp, included above)
// training: codes uint8 [n, M] | sums int64 [M][256][dsub] | counts int32 [M][256] (one memset clears the sums and the counts)
struct PqTrainWs : WsLayout {
  uint8_t* codes;
  unsigned long long* sums;
  int32_t* counts;
  PqTrainWs(void* ws, int64_t n, int d, int dsub) : WsLayout(ws) {
    codes = take<uint8_t>((size_t)n * (d / dsub), 16);
    sums = take<unsigned long long>((size_t)PQ_CW * d);
    counts = take<int32_t>((size_t)PQ_CW * (d / dsub));
  }
};
// blocks of the training update: (row blocks) x M
int64_t pq_update_blocks(int64_t n, int d, int dsub) { return (n + PQ_ROWS - 1) / PQ_ROWS * (d / dsub); }
int pq_check_train_size(int64_t n, int32_t d, int32_t dsub) {  // behind check_shape and pq_check_dsub
  if ((int64_t)PQ_CW * d > IVF_MAX || pq_update_blocks(n, d, dsub) > IVF_MAX)
    return fail(SMI_ERR_UNSUPPORTED, "n=%lld, d=%d: the codebook elements and the update's blocks must fit int32", (long long)n, d);
  return SMI_OK;
}

template <int DSUB, bool RES>
hipError_t launch_pq_accumulate(int64_t blocks, hipStream_t st, const f16* xn, int64_t n, int d, const uint8_t* codes,
                                unsigned long long* sums, int32_t* counts, const int32_t* labels, const f16* cent, int K) {
  return launch_with_lds<pq_accumulate_kernel<DSUB, RES>>(dim3((unsigned)blocks), IVF_TB, pq_accumulate_lds<DSUB>(), st, xn, n,
                                                          d, codes, sums, counts, labels, cent, K);
}

// launch(dsub as a std::integral_constant): the residual kernels that take dsub at compile time
template <class Launch>
void with_dsub(int dsub, Launch launch) {
  if (dsub == 8) launch(std::integral_constant<int, 8>{});
  else if (dsub == 16) launch(std::integral_constant<int, 16>{});
  else if (dsub == 32) launch(std::integral_constant<int, 32>{});
  else launch(std::integral_constant<int, 64>{});
}
void launch_pq_encode_residual(const f16* xn, int64_t n, int d, int dsub, const f16* cb, uint8_t* codes, const int32_t* labels,
                               const f16* cent, int K, hipStream_t st) {
  with_dsub(dsub, [&](auto ds) {
    hipLaunchKernelGGL(pq_encode_residual_kernel<decltype(ds)::value>, grid_for(n, IVF_TB / 64), dim3(IVF_TB), 0, st, xn, n, d, cb,
                       codes, labels, cent, K);
  });
}

int pq_check_centroids(const void* centroids, int64_t K) {
  if (!centroids) return fail(SMI_ERR_INVALID_ARG, "null centroids");
  if ((uintptr_t)centroids % 16) return fail(SMI_ERR_INVALID_ARG, "centroids must be 16-byte aligned");
  if (K < 1) return fail(SMI_ERR_INVALID_ARG, "K=%lld: at least one list", (long long)K);
  if (K > IVF_MAX) return fail(SMI_ERR_UNSUPPORTED, "K=%lld: list numbers must fit int32", (long long)K);
  return SMI_OK;
}

// The entries of the plain (3.21) and the residual (3.22) product quantiser, stated once: the refusals of the plain entry, in
// its order, then those of what RES adds (labels, the centroids cent fp16 [K, d], coarse), then the launches.
template <bool RES>
int pq_train_entry(const void* xn, const int32_t* labels, int64_t n, int32_t d, const void* cent, int64_t K, int32_t dsub,
                   const int32_t* init, int32_t n_iter, void* codebooks, void* ws, int64_t ws_bytes, void* stream) {
  if (!xn || !init || (RES && !labels)) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_shape(n, "n", d, 1, "list")) return rc;
  if (const int rc = pq_check_codebooks(d, dsub, codebooks)) return rc;
  if constexpr (RES)
    if (const int rc = pq_check_centroids(cent, K)) return rc;
  if (n_iter < 0) return fail(SMI_ERR_INVALID_ARG, "n_iter=%d must not be negative", n_iter);
  if (const int rc = pq_check_train_size(n, d, dsub)) return rc;
  const PqTrainWs w(ws, n, d, dsub);
  if (const int rc = check_ws(ws, ws_bytes, w.bytes(), "smi_pq_train_workspace_bytes(n, d, dsub)")) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t st = (hipStream_t)stream;
  const int M = d / dsub;
  const dim3 block(IVF_TB);
  hipLaunchKernelGGL(pq_init_kernel<RES>, grid_for((int64_t)PQ_CW * (d / 8), IVF_TB), block, 0, st, (const f16*)xn, d, dsub, init,
                     (f16*)codebooks, labels, (const f16*)cent, (int)K);
  HIP_TRY(hipGetLastError());
  const int64_t blocks = pq_update_blocks(n, d, dsub);
  auto accumulate = dsub == 8 ? launch_pq_accumulate<8, RES> : dsub == 16 ? launch_pq_accumulate<16, RES>
                  : dsub == 32 ? launch_pq_accumulate<32, RES> : launch_pq_accumulate<64, RES>;
  for (int it = 0; it < n_iter; ++it) {
    if constexpr (RES)
      launch_pq_encode_residual((const f16*)xn, n, d, dsub, (const f16*)codebooks, w.codes, labels, (const f16*)cent, (int)K, st);
    else
      hipLaunchKernelGGL(pq_encode_kernel, grid_for(n, IVF_TB / 64), block, 0, st, (const f16*)xn, n, d, dsub,
                         (const f16*)codebooks, w.codes);
    HIP_TRY(hipMemsetAsync(w.sums, 0, (size_t)PQ_CW * d * 8 + (size_t)PQ_CW * M * 4, st));  // the sums and the counts behind
    HIP_TRY(accumulate(blocks, st, (const f16*)xn, n, d, w.codes, w.sums, w.counts, labels, (const f16*)cent, (int)K));
    hipLaunchKernelGGL(pq_finalize_kernel, grid_for((int64_t)PQ_CW * d, IVF_TB), block, 0, st, (const long long*)w.sums,
                       w.counts, d, dsub, (f16*)codebooks);
    HIP_TRY(hipGetLastError());
  }
  return SMI_OK;
}

template <bool RES>
int pq_build_entry(const void* xn, const int32_t* labels, int64_t n, int32_t d, int64_t K, const void* cent, int32_t dsub,
                   const void* codebooks, void* list_codes, int32_t* list_ids, int64_t capacity_slots, int32_t* list_offsets,
                   int32_t* list_sizes, void* ws, int64_t ws_bytes, void* stream) {
  return build_entry(
      !xn || !list_codes, labels, n, d, K, list_ids, capacity_slots, list_offsets, list_sizes, ws, ws_bytes, stream,
      "smi_ivf_pq_build_workspace_bytes(n, K, d, dsub)",
      [&] {
        const int rc = pq_check_codebooks(d, dsub, codebooks);
        return rc || !RES ? rc : pq_check_centroids(cent, K);
      },
      [&](dim3 grid, hipStream_t st) {
        auto gather = [&](auto ds) {
          hipLaunchKernelGGL(ivf_pq_gather_kernel<decltype(ds)::value>, grid, dim3(IVF_TB), 0, st, (const f16*)xn, d, dsub,
                             (const f16*)codebooks, (const int32_t*)list_ids, (const int32_t*)list_offsets, (int)K,
                             (uint8_t*)list_codes, labels, (const f16*)cent);
        };
        if constexpr (RES) with_dsub(dsub, gather);
        else gather(std::integral_constant<int, 0>{});
      });
}

template <bool RES>
int pq_search_entry(const void* qn, int64_t nq, int32_t d, const int32_t* probes, const float* coarse, int32_t nprobe,
                    const void* list_codes, int32_t dsub, const void* codebooks, const int32_t* list_ids,
                    const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* ws, int64_t ws_bytes,
                    void* stream, const IvfKeys* keys = nullptr) {
  return search_entry(
      !qn || !list_codes || (RES && !coarse), keys_refusals(keys), nq, d, probes, nprobe, list_ids, list_offsets, K, k, idx, score, ws, ws_bytes, stream,
      "smi_ivf_pq_search_workspace_bytes(nq, K, nprobe, k, d, dsub)", 0, 0, [&] { return pq_check_codebooks(d, dsub, codebooks); },
      no_prepare, [&](auto kt, int unit, int64_t units, const SearchWs& w, hipStream_t st) {
        constexpr int KT = decltype(kt)::value;
        constexpr int lds_small = RES ? ivf_pq_residual_scan_lds<IVF_BM>(KT) : ivf_scan_lds<IVF_BM>(KT);
        constexpr int lds_big = RES ? ivf_pq_residual_scan_lds<IVF_BIG>(KT) : ivf_scan_lds<IVF_BIG>(KT);
        return launch_units_keyed<ivf_pq_scan_lists_kernel<KT, IVF_BM, RES>, ivf_pq_scan_lists_kernel<KT, IVF_BIG, RES>,
                                  ivf_pq_scan_lists_kernel_keyed<KT, IVF_BM, RES>, ivf_pq_scan_lists_kernel_keyed<KT, IVF_BIG, RES>>(
            keys, unit, units, lds_small, lds_big, st, (const f16*)qn, d, (int)nq, nprobe, (const uint8_t*)list_codes, pq_shift(dsub),
            (const f16*)codebooks, list_ids, list_offsets, (int)K, (const int32_t*)w.poff, (const int32_t*)w.ubase,
            (const int32_t*)w.pairs, k, w.ps, w.pi, coarse);
      });
}

// smi_ivf_search / smi_ivf_i8_search and their keyed twins, stated once each
int flat_search_entry(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                      const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score,
                      void* ws, int64_t ws_bytes, void* stream, const IvfKeys* keys) {
  return search_entry(
      !qn || !list_rows, keys_refusals(keys), nq, d, probes, nprobe, list_ids, list_offsets, K, k, idx, score, ws, ws_bytes, stream,
      "smi_ivf_search_workspace_bytes(nq, K, nprobe, k, d)", 0, 0, no_refusals, no_prepare,
      [&](auto kt, int unit, int64_t units, const SearchWs& w, hipStream_t st) {
        constexpr int KT = decltype(kt)::value;
        return launch_units_keyed<ivf_scan_lists_kernel<KT, IVF_BM>, ivf_scan_lists_kernel<KT, IVF_BIG>,
                                  ivf_scan_lists_kernel_keyed<KT, IVF_BM>, ivf_scan_lists_kernel_keyed<KT, IVF_BIG>>(
            keys, unit, units, ivf_scan_lds<IVF_BM>(KT), ivf_scan_lds<IVF_BIG>(KT), st, (const f16*)qn, d, (int)nq, nprobe,
            (const f16*)list_rows, list_ids, list_offsets, (int)K, (const int32_t*)w.poff, (const int32_t*)w.ubase,
            (const int32_t*)w.pairs, k, w.ps, w.pi);
      });
}
int i8_search_entry(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_codes,
                    const float* list_scales, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k,
                    int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream, const IvfKeys* keys) {
  return search_entry(
      !qn || !list_codes || !list_scales, keys_refusals(keys), nq, d, probes, nprobe, list_ids, list_offsets, K, k, idx, score, ws, ws_bytes,
      stream, "smi_ivf_i8_search_workspace_bytes(nq, K, nprobe, k, d)", d, 0, [&] { return i8_check_dim(d); },
      [&](const SearchWs& w, hipStream_t st) {  // the queries, encoded like the rows
        hipLaunchKernelGGL(ivf_i8_encode_kernel, grid_for(nq, IVF_TB / 64), dim3(IVF_TB), 0, st, (const f16*)qn, nq, d, w.qc,
                           w.qscale);
        return hipSuccess;  // (a launch that failed answers at the inversion's end)
      },
      [&](auto kt, int unit, int64_t units, const SearchWs& w, hipStream_t st) {
        constexpr int KT = decltype(kt)::value;
        return launch_units_keyed<ivf_i8_scan_lists_kernel<KT, IVF_BM>, ivf_i8_scan_lists_kernel<KT, IVF_BIG>,
                                  ivf_i8_scan_lists_kernel_keyed<KT, IVF_BM>, ivf_i8_scan_lists_kernel_keyed<KT, IVF_BIG>>(
            keys, unit, units, ivf_i8_scan_lds<IVF_BM>(KT), ivf_i8_scan_lds<IVF_BIG>(KT), st, (const int8_t*)w.qc,
            (const float*)w.qscale, d, (int)nq, nprobe, (const int8_t*)list_codes, list_scales, list_ids, list_offsets, (int)K,
            (const int32_t*)w.poff, (const int32_t*)w.ubase, (const int32_t*)w.pairs, k, w.ps, w.pi);
      });
}

// smi_ivf_search_page: the flat search with lists of a page, up to 64 probes and a ceiling per query.  Its
// workspace is the search's and one 64-bit ceiling key per query behind it.
int flat_search_page_entry(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                           const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, const float* ceil_score,
                           const int32_t* ceil_idx, int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream) {
  return search_entry<PageLists>(
      !qn || !list_rows,
      [&] {
        return !ceil_score != !ceil_idx ? fail(SMI_ERR_INVALID_ARG, "ceil_score and ceil_idx go together: both or neither")
                                        : (int)SMI_OK;
      },
      nq, d, probes, nprobe, list_ids, list_offsets, K, k, idx, score, ws, ws_bytes, stream,
      "smi_ivf_search_page_ws_bytes(nq, K, nprobe, k, d)", 0, nq, no_refusals,
      [&](const SearchWs& w, hipStream_t st) {
        return ceil_idx ? launch_ceiling_keys(ceil_score, ceil_idx, nq, nq, 0, w.ceil, st) : hipSuccess;
      },
      [&](auto, int unit, int64_t units, const SearchWs& w, hipStream_t st) {
        return launch_units<ivf_scan_page_kernel<IVF_BM>, ivf_scan_page_kernel<IVF_BIG>>(
            unit, units, ivf_page_scan_lds<IVF_BM>(), ivf_page_scan_lds<IVF_BIG>(), st, (const f16*)qn, d, (int)nq, nprobe,
            (const f16*)list_rows, list_ids, list_offsets, (int)K, (const int32_t*)w.poff, (const int32_t*)w.ubase,
            (const int32_t*)w.pairs, k, w.ps, w.pi, (const unsigned long long*)(ceil_idx ? w.ceil : nullptr));
      });
}

// ---------------------------------------------------------------- L2 flat search
// ivf_scan_lists_kernel with ONE change: the fold loads the four slot biases (bias fp32 [slots], -1/2 ||row||^2 of the row a
// slot holds, smi_l2_slot_bias) with one 16-byte load beside the four ids, and the score of a candidate is sum + bias.  The
// sum starts from +0 and is never -0, so a zero score is +0 (l2.hip).  A pad slot stays out by id >= 0, whatever its bias.  Its
// own kernel, outside the twice-included ivf_list_kernels.hpp: there is no keyed twin.
template <int KT, int B>
__global__ __launch_bounds__(IVF_TB) void ivf_l2_scan_lists_kernel(const f16* __restrict__ qn, int d, int nq, int nprobe,
                                                                   const f16* __restrict__ rows, const int32_t* __restrict__ ids,
                                                                   const float* __restrict__ bias, const int32_t* __restrict__ off,
                                                                   int K, const int32_t* __restrict__ poff,
                                                                   const int32_t* __restrict__ ubase,
                                                                   const int32_t* __restrict__ pairs, int k_out,
                                                                   float* __restrict__ ps, int32_t* __restrict__ pi) {
  constexpr int NR = B / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lists = (unsigned long long*)(smem + 4 * B * IVF_SLICE);
  int* spair = (int*)(lists + B * KT);
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= ubase[K]) return;
  const int l = ivf_unit_list(ubase, K, b);
  const int p0 = poff[l] + (b - ubase[l]) * B;
  const int npair = min(B, poff[l + 1] - p0);
  const int s_begin = off[l], s_end = off[l + 1];
  ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [](int) {});

  const int nk = d / IVF_BK, cc = tid & 7;
  const f16* qsrc[NR];  // this thread's query rows of a slice
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int pr = spair[(tid >> 3) + 32 * j];
    qsrc[j] = pr >= 0 ? qn + (size_t)(pr / nprobe) * d + cc * 8 : nullptr;
  }
  auto fetch = [&](int it, u32x4(&qv)[NR], u32x4(&lv)[NR]) {  // ivf_scan_lists_kernel's
    const int tile = it / nk, ks = it - tile * nk;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int slot = s_begin + tile * B + (tid >> 3) + 32 * j;
      qv[j] = qsrc[j] ? *(const u32x4*)(qsrc[j] + ks * IVF_BK) : u32x4{0u, 0u, 0u, 0u};
      lv[j] = slot < s_end ? *(const u32x4*)(rows + (size_t)slot * d + ks * IVF_BK + cc * 8) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto fold = [&](int slot0, const f32x4(&acc)[NR]) {
    const f32x4 b4 = *(const f32x4*)(bias + slot0);
    ivf_topk_fold<KT, B>(
        lists, npair, *(const int4*)(ids + slot0), acc, [b4](int) { return [b4](float a, int r) { return a + b4[r]; }; },
        IvfKeyTest<B, IvfNoKeys>(IvfNoKeys{}, nullptr));
  };
  ivf_slice_walk<B, IvfF16>(smem, s_begin, s_end, nk, ivf_live_blocks<B>(npair), fetch, fold);
  ivf_lists_readout<KT>(lists, spair, npair, nprobe, nq, k_out, ps, pi);
}

// smi_l2_flat_search: smi_ivf_search's entry over the kernel above
int l2_flat_search_entry(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                         const float* list_bias, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k,
                         int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream) {
  return search_entry(
      !qn || !list_rows || !list_bias, no_refusals, nq, d, probes, nprobe, list_ids, list_offsets, K, k, idx, score, ws, ws_bytes, stream,
      "smi_l2_flat_search_ws_bytes(nq, K, nprobe, k, d)", 0, 0,
      [&] { return (uintptr_t)list_bias % 16 ? fail(SMI_ERR_INVALID_ARG, "list_bias must be 16-byte aligned") : (int)SMI_OK; },
      no_prepare, [&](auto kt, int unit, int64_t units, const SearchWs& w, hipStream_t st) {
        constexpr int KT = decltype(kt)::value;
        return launch_units<ivf_l2_scan_lists_kernel<KT, IVF_BM>, ivf_l2_scan_lists_kernel<KT, IVF_BIG>>(
            unit, units, ivf_scan_lds<IVF_BM>(KT), ivf_scan_lds<IVF_BIG>(KT), st, (const f16*)qn, d, (int)nq, nprobe,
            (const f16*)list_rows, list_ids, list_bias, list_offsets, (int)K, (const int32_t*)w.poff, (const int32_t*)w.ubase,
            (const int32_t*)w.pairs, k, w.ps, w.pi);
      });
}

// ---------------------------------------------------------------- regrouping: extend, remove, merge
#include "ivf_regroup.hpp"

// ---------------------------------------------------------------- L2 over the product-quantised lists
#include "ivf_pq_l2.hpp"

}  // namespace

}  // namespace smi

extern "C" {

int64_t smi_ivf_search_page_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d) {
  const KeepLastError keep;
  return check_search_args(nq, d, K, nprobe, k, PageLists::limits) ? 0 : (int64_t)SearchWs(nullptr, nq, K, nprobe, k, 0, nq).bytes();
}

int smi_ivf_search_page(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                        const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score,
                        void* ws, int64_t ws_bytes, void* stream, const float* ceil_score, const int32_t* ceil_idx) {
  return flat_search_page_entry(qn, nq, d, probes, nprobe, list_rows, list_ids, list_offsets, K, k, ceil_score, ceil_idx, idx, score,
                                ws, ws_bytes, stream);
}

int32_t smi_ivf_list_align(void) { return IVF_ALIGN; }

int64_t smi_ivf_slots_bound(int64_t n, int64_t K) {
  const KeepLastError keep;
  return check_build_shape(n, 64, K) ? 0 : slots_bound(n, K);  // (any d a build takes: the bound does not depend on it)
}

int64_t smi_ivf_build_workspace_bytes(int64_t n, int64_t K, int32_t d) {
  const KeepLastError keep;
  return check_build_shape(n, d, K) ? 0 : (int64_t)BuildWs(nullptr, K).bytes();
}

int smi_ivf_build(const void* xn, const int32_t* labels, int64_t n, int32_t d, int64_t K, void* list_rows, int32_t* list_ids,
                  int64_t capacity_slots, int32_t* list_offsets, int32_t* list_sizes, void* ws, int64_t ws_bytes,
                  void* stream) {
  return build_entry(
      !xn || !list_rows, labels, n, d, K, list_ids, capacity_slots, list_offsets, list_sizes, ws, ws_bytes, stream,
      "smi_ivf_build_workspace_bytes(n, K, d)", no_refusals, [&](dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(ivf_gather_kernel, grid, dim3(IVF_TB), 0, st, (const f16*)xn, d, list_ids, list_offsets, (int)K,
                           (f16*)list_rows);
      });
}

int64_t smi_ivf_search_workspace_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d) {
  const KeepLastError keep;
  return check_search_args(nq, d, K, nprobe, k) ? 0 : (int64_t)SearchWs(nullptr, nq, K, nprobe, k).bytes();
}

int smi_ivf_search(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                   const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score,
                   void* ws, int64_t ws_bytes, void* stream) {
  return flat_search_entry(qn, nq, d, probes, nprobe, list_rows, list_ids, list_offsets, K, k, idx, score, ws, ws_bytes, stream,
                           nullptr);
}

// ---------------------------------------------------------------- range search
int64_t smi_range_search_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t d) {
  const KeepLastError keep;
  return check_range_shape(nq, d, K, nprobe) ? 0 : (int64_t)SearchWs(nullptr, nq, K, nprobe, 0).bytes();
}

int smi_range_search_count(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const float* threshold,
                           const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets, int64_t K,
                           int32_t* pair_counts, void* ws, int64_t ws_bytes, void* stream) {
  return range_entry(!pair_counts, nullptr, qn, nq, d, probes, nprobe, threshold, list_rows, list_ids, list_offsets, K, pair_counts,
                     nullptr, 0, nullptr, nullptr, ws, ws_bytes, stream);
}

int smi_range_search_emit(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const float* threshold,
                          const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets, int64_t K,
                          const int64_t* pair_base, int64_t total, float* score, int32_t* idx, void* ws, int64_t ws_bytes,
                          void* stream) {
  return range_entry(!pair_base || !score || !idx, nullptr, qn, nq, d, probes, nprobe, threshold, list_rows, list_ids, list_offsets, K,
                     nullptr, pair_base, total, score, idx, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- semantic de-duplication
int64_t smi_ivf_dedup_workspace_bytes(int64_t slots, int64_t n, int64_t K, int32_t d) {
  const KeepLastError keep;
  return check_dedup_shape(slots, n, K, d) ? 0 : (int64_t)DedupWs(nullptr, slots, K).bytes();
}

int smi_ivf_dedup(const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int64_t slots,
                  int32_t d, const float* priority, int64_t n, float* max_sim, int32_t* nearest, void* ws, int64_t ws_bytes,
                  void* stream) {
  if (!list_rows || !list_ids || !list_offsets || !max_sim || !nearest) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_dedup_shape(slots, n, K, d)) return rc;
  const DedupWs w(ws, slots, K);
  if (const int rc = check_ws(ws, ws_bytes, w.bytes(), "smi_ivf_dedup_workspace_bytes(slots, n, K, d)")) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t st = (hipStream_t)stream;
  // own rows of a unit = slots of its tiles: 128 where the lists average 256 rows or more, else 64 (unit_pairs' rule with
  // one "pair" per row)
  const int unit = unit_pairs(n, K);
  const dim3 block(IVF_TB);
  hipLaunchKernelGGL(ivf_fill_kernel, grid_for(n, IVF_TB), block, 0, st, max_sim, nearest, n);
  hipLaunchKernelGGL(ivf_span_kernel, grid_for(K, IVF_TB), block, 0, st, list_offsets, (int)K, w.span);
  hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), block, 0, st, w.span, (int)K, 1, unit, w.span_off, w.cursor, w.ubase);
  hipLaunchKernelGGL(ivf_slot_priority_kernel, grid_for(slots, IVF_TB), block, 0, st, list_ids, list_offsets, (int)K, priority,
                     (int)n, w.sprio);
  HIP_TRY(hipGetLastError());
  // units for every list layout the storage can hold: a list has ceil(padded size / unit) of them, at most slots / unit + K
  // in all; those from ubase[K] on find nothing to do
  const int64_t units = slots / unit + K;
  HIP_TRY((launch_units<ivf_selfjoin_kernel<IVF_BM>, ivf_selfjoin_kernel<IVF_BIG>>(
      unit, units, ivf_selfjoin_lds<IVF_BM>(), ivf_selfjoin_lds<IVF_BIG>(), st, (const f16*)list_rows, d, list_ids, w.sprio,
      list_offsets, (int)K, w.ubase, (int)n, max_sim, nearest)));
  return SMI_OK;
}

// ---------------------------------------------------------------- int8 lists
int smi_ivf_i8_encode(const void* xn, int64_t n, int32_t d, void* codes, float* scales, void* stream) {
  return rows_entry(!xn || !codes || !scales, nullptr, "", n, d, [&] { return i8_check_dim(d); }, [&] {
    hipLaunchKernelGGL(ivf_i8_encode_kernel, grid_for(n, IVF_TB / 64), dim3(IVF_TB), 0, (hipStream_t)stream, (const f16*)xn, n, d,
                       (int8_t*)codes, scales);
  });
}

int64_t smi_ivf_i8_build_workspace_bytes(int64_t n, int64_t K, int32_t d) {
  const KeepLastError keep;
  return check_build_shape(n, d, K) || i8_check_dim(d) ? 0 : (int64_t)BuildWs(nullptr, K).bytes();
}

int smi_ivf_i8_build(const void* xn, const int32_t* labels, int64_t n, int32_t d, int64_t K, void* list_codes,
                     float* list_scales, int32_t* list_ids, int64_t capacity_slots, int32_t* list_offsets,
                     int32_t* list_sizes, void* ws, int64_t ws_bytes, void* stream) {
  return build_entry(
      !xn || !list_codes || !list_scales, labels, n, d, K, list_ids, capacity_slots, list_offsets, list_sizes, ws, ws_bytes, stream,
      "smi_ivf_i8_build_workspace_bytes(n, K, d)", [&] { return i8_check_dim(d); }, [&](dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(ivf_i8_gather_kernel, grid, dim3(IVF_TB), 0, st, (const f16*)xn, d, list_ids, list_offsets, (int)K,
                           (int8_t*)list_codes, list_scales);
      });
}

int64_t smi_ivf_i8_search_workspace_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d) {
  const KeepLastError keep;
  const bool refused = check_search_args(nq, d, K, nprobe, k) || i8_check_dim(d);
  return refused ? 0 : (int64_t)SearchWs(nullptr, nq, K, nprobe, k, d).bytes();
}

int smi_ivf_i8_search(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_codes,
                      const float* list_scales, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k,
                      int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream) {
  return i8_search_entry(qn, nq, d, probes, nprobe, list_codes, list_scales, list_ids, list_offsets, K, k, idx, score, ws,
                         ws_bytes, stream, nullptr);
}

// ---------------------------------------------------------------- product quantiser and product-quantised lists
int smi_pq_encode(const void* xn, int64_t n, int32_t d, int32_t dsub, const void* codebooks, void* codes, void* stream) {
  return rows_entry(!xn || !codes, nullptr, "", n, d, [&] { return pq_check_codebooks(d, dsub, codebooks); }, [&] {
    hipLaunchKernelGGL(pq_encode_kernel, grid_for(n, IVF_TB / 64), dim3(IVF_TB), 0, (hipStream_t)stream, (const f16*)xn, n, d, dsub,
                       (const f16*)codebooks, (uint8_t*)codes);
  });
}

int smi_pq_decode(const void* codes, int64_t n, int32_t d, int32_t dsub, const void* codebooks, void* rows, void* stream) {
  return rows_entry(!codes || !rows, rows, "rows", n, d, [&] { return pq_check_codebooks(d, dsub, codebooks); }, [&] {
    hipLaunchKernelGGL(pq_decode_kernel, grid_for(n * (d / 8), IVF_TB), dim3(IVF_TB), 0, (hipStream_t)stream, (const uint8_t*)codes,
                       n, d, dsub, (const f16*)codebooks, (f16*)rows);
  });
}

int64_t smi_pq_train_workspace_bytes(int64_t n, int32_t d, int32_t dsub) {
  const KeepLastError keep;
  const bool refused = check_shape(n, "n", d, 1, "list") || pq_check_dsub(d, dsub) || pq_check_train_size(n, d, dsub);
  return refused ? 0 : (int64_t)PqTrainWs(nullptr, n, d, dsub).bytes();
}

int smi_pq_train(const void* xn, int64_t n, int32_t d, int32_t dsub, const int32_t* init, int32_t n_iter, void* codebooks,
                 void* ws, int64_t ws_bytes, void* stream) {
  return pq_train_entry<false>(xn, nullptr, n, d, nullptr, 0, dsub, init, n_iter, codebooks, ws, ws_bytes, stream);
}

int64_t smi_ivf_pq_build_workspace_bytes(int64_t n, int64_t K, int32_t d, int32_t dsub) {
  const KeepLastError keep;
  return check_build_shape(n, d, K) || pq_check_dsub(d, dsub) ? 0 : (int64_t)BuildWs(nullptr, K).bytes();
}

int smi_ivf_pq_build(const void* xn, const int32_t* labels, int64_t n, int32_t d, int64_t K, int32_t dsub,
                     const void* codebooks, void* list_codes, int32_t* list_ids, int64_t capacity_slots,
                     int32_t* list_offsets, int32_t* list_sizes, void* ws, int64_t ws_bytes, void* stream) {
  return pq_build_entry<false>(xn, labels, n, d, K, nullptr, dsub, codebooks, list_codes, list_ids, capacity_slots, list_offsets,
                               list_sizes, ws, ws_bytes, stream);
}

int64_t smi_ivf_pq_search_workspace_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d, int32_t dsub) {
  const KeepLastError keep;
  const bool refused = check_search_args(nq, d, K, nprobe, k) || pq_check_dsub(d, dsub);
  return refused ? 0 : (int64_t)SearchWs(nullptr, nq, K, nprobe, k).bytes();
}

int smi_ivf_pq_search(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_codes,
                      int32_t dsub, const void* codebooks, const int32_t* list_ids, const int32_t* list_offsets, int64_t K,
                      int32_t k, int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream) {
  return pq_search_entry<false>(qn, nq, d, probes, nullptr, nprobe, list_codes, dsub, codebooks, list_ids, list_offsets, K, k, idx,
                                score, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- residual encoding against the list centroid (3.22)
int smi_pq_residuals(const void* xn, const int32_t* labels, int64_t n, int32_t d, const void* centroids, int64_t K, void* out,
                     void* stream) {
  return rows_entry(!xn || !labels || !out, out, "out", n, d, [&] { return pq_check_centroids(centroids, K); }, [&] {
    hipLaunchKernelGGL(pq_residuals_kernel, grid_for(n * (d / 8), IVF_TB), dim3(IVF_TB), 0, (hipStream_t)stream, (const f16*)xn, n,
                       d, labels, (const f16*)centroids, (int)K, (f16*)out);
  });
}

int smi_pq_encode_residual(const void* xn, const int32_t* labels, int64_t n, int32_t d, const void* centroids, int64_t K,
                           int32_t dsub, const void* codebooks, void* codes, void* stream) {
  return rows_entry(
      !xn || !labels || !codes, nullptr, "", n, d,
      [&] {
        const int rc = pq_check_codebooks(d, dsub, codebooks);
        return rc ? rc : pq_check_centroids(centroids, K);
      },
      [&] {
        launch_pq_encode_residual((const f16*)xn, n, d, dsub, (const f16*)codebooks, (uint8_t*)codes, labels, (const f16*)centroids,
                                  (int)K, (hipStream_t)stream);
      });
}

int smi_pq_train_residual(const void* xn, const int32_t* labels, int64_t n, int32_t d, const void* centroids, int64_t K,
                          int32_t dsub, const int32_t* init, int32_t n_iter, void* codebooks, void* ws, int64_t ws_bytes,
                          void* stream) {
  return pq_train_entry<true>(xn, labels, n, d, centroids, K, dsub, init, n_iter, codebooks, ws, ws_bytes, stream);
}

int smi_ivf_pq_build_residual(const void* xn, const int32_t* labels, int64_t n, int32_t d, int64_t K, const void* centroids,
                              int32_t dsub, const void* codebooks, void* list_codes, int32_t* list_ids, int64_t capacity_slots,
                              int32_t* list_offsets, int32_t* list_sizes, void* ws, int64_t ws_bytes, void* stream) {
  return pq_build_entry<true>(xn, labels, n, d, K, centroids, dsub, codebooks, list_codes, list_ids, capacity_slots, list_offsets,
                              list_sizes, ws, ws_bytes, stream);
}

int smi_ivf_pq_search_residual(const void* qn, int64_t nq, int32_t d, const int32_t* probes, const float* coarse, int32_t nprobe,
                               const void* list_codes, int32_t dsub, const void* codebooks, const int32_t* list_ids,
                               const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* ws,
                               int64_t ws_bytes, void* stream) {
  return pq_search_entry<true>(qn, nq, d, probes, coarse, nprobe, list_codes, dsub, codebooks, list_ids, list_offsets, K, k, idx,
                               score, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- filtered search
int smi_slot_filter(const int32_t* list_ids, const int32_t* list_offsets, int64_t K, const int32_t* row_keys,
                    const uint8_t* row_mask, int64_t n, int32_t* slot_ids_out, int32_t* slot_keys_out, int64_t slots,
                    void* stream) {
  if (!list_ids || !list_offsets || !slot_ids_out) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (!row_keys && !row_mask) return fail(SMI_ERR_INVALID_ARG, "null row_keys and null row_mask: nothing to filter by");
  if (!row_keys != !slot_keys_out)
    return fail(SMI_ERR_INVALID_ARG, "row_keys and slot_keys_out go together: both, or neither");
  if ((uintptr_t)slot_ids_out % 16 || (uintptr_t)slot_keys_out % 16)
    return fail(SMI_ERR_INVALID_ARG, "slot_ids_out and slot_keys_out must be 16-byte aligned");
  if (K < 1) return fail(SMI_ERR_INVALID_ARG, "K=%lld: at least one list", (long long)K);
  if (n < 1) return fail(SMI_ERR_INVALID_ARG, "n=%lld: empty input", (long long)n);
  if (slots < 1) return fail(SMI_ERR_INVALID_ARG, "slots=%lld: empty storage", (long long)slots);
  if (n > IVF_MAX || K > IVF_MAX || slots > IVF_MAX)
    return fail(SMI_ERR_UNSUPPORTED, "n=%lld, K=%lld, slots=%lld: row, list and slot numbers must fit int32", (long long)n,
                (long long)K, (long long)slots);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  // one thread per slot the storage holds
  hipLaunchKernelGGL(ivf_slot_filter_kernel, grid_for(slots, IVF_TB), dim3(IVF_TB), 0, (hipStream_t)stream, list_ids, list_offsets,
                     (int)K, row_keys, row_mask, n, slots, slot_ids_out, slot_keys_out);
  HIP_TRY(hipGetLastError());
  return SMI_OK;
}

int smi_ivf_search_keyed(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                         const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score,
                         void* ws, int64_t ws_bytes, void* stream, const int32_t* slot_keys, const int32_t* query_keys,
                         int32_t accept) {
  const IvfKeys keys{slot_keys, query_keys, accept};
  return flat_search_entry(qn, nq, d, probes, nprobe, list_rows, list_ids, list_offsets, K, k, idx, score, ws, ws_bytes, stream,
                           &keys);
}

int smi_ivf_i8_search_keyed(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_codes,
                            const float* list_scales, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k,
                            int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream, const int32_t* slot_keys,
                            const int32_t* query_keys, int32_t accept) {
  const IvfKeys keys{slot_keys, query_keys, accept};
  return i8_search_entry(qn, nq, d, probes, nprobe, list_codes, list_scales, list_ids, list_offsets, K, k, idx, score, ws,
                         ws_bytes, stream, &keys);
}

int smi_ivf_pq_search_keyed(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_codes,
                            int32_t dsub, const void* codebooks, const int32_t* list_ids, const int32_t* list_offsets, int64_t K,
                            int32_t k, int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream,
                            const int32_t* slot_keys, const int32_t* query_keys, int32_t accept) {
  const IvfKeys keys{slot_keys, query_keys, accept};
  return pq_search_entry<false>(qn, nq, d, probes, nullptr, nprobe, list_codes, dsub, codebooks, list_ids, list_offsets, K, k, idx,
                                score, ws, ws_bytes, stream, &keys);
}

int smi_ivf_pq_search_residual_keyed(const void* qn, int64_t nq, int32_t d, const int32_t* probes, const float* coarse,
                                     int32_t nprobe, const void* list_codes, int32_t dsub, const void* codebooks,
                                     const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx,
                                     float* score, void* ws, int64_t ws_bytes, void* stream, const int32_t* slot_keys,
                                     const int32_t* query_keys, int32_t accept) {
  const IvfKeys keys{slot_keys, query_keys, accept};
  return pq_search_entry<true>(qn, nq, d, probes, coarse, nprobe, list_codes, dsub, codebooks, list_ids, list_offsets, K, k, idx,
                               score, ws, ws_bytes, stream, &keys);
}

int smi_range_search_count_keyed(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                                 const float* threshold, const void* list_rows, const int32_t* list_ids,
                                 const int32_t* list_offsets, int64_t K, int32_t* pair_counts, void* ws, int64_t ws_bytes,
                                 void* stream, const int32_t* slot_keys, const int32_t* query_keys, int32_t accept) {
  const IvfKeys keys{slot_keys, query_keys, accept};
  return range_entry(!pair_counts, &keys, qn, nq, d, probes, nprobe, threshold, list_rows, list_ids, list_offsets, K, pair_counts,
                     nullptr, 0, nullptr, nullptr, ws, ws_bytes, stream);
}

int smi_range_search_emit_keyed(const void* qn, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                                const float* threshold, const void* list_rows, const int32_t* list_ids,
                                const int32_t* list_offsets, int64_t K, const int64_t* pair_base, int64_t total, float* score,
                                int32_t* idx, void* ws, int64_t ws_bytes, void* stream, const int32_t* slot_keys,
                                const int32_t* query_keys, int32_t accept) {
  const IvfKeys keys{slot_keys, query_keys, accept};
  return range_entry(!pair_base || !score || !idx, &keys, qn, nq, d, probes, nprobe, threshold, list_rows, list_ids, list_offsets,
                     K, nullptr, pair_base, total, score, idx, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------- L2 flat search
int64_t smi_l2_flat_search_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d) {
  const KeepLastError keep;
  return check_search_args(nq, d, K, nprobe, k) ? 0 : (int64_t)SearchWs(nullptr, nq, K, nprobe, k).bytes();
}

int smi_l2_flat_search(const void* q_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                       const float* list_bias, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k,
                       int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream) {
  return l2_flat_search_entry(q_f16, nq, d, probes, nprobe, list_rows, list_bias, list_ids, list_offsets, K, k, idx, score, ws,
                              ws_bytes, stream);
}

// ---------------------------------------------------------------- regrouping
int64_t smi_lists_regroup_ws_bytes(int64_t old_slots, int64_t n_new, int64_t K) {
  const KeepLastError keep;
  return check_regroup_shape(old_slots, n_new, K) ? 0 : (int64_t)RegroupWs(nullptr, old_slots + n_new, K).bytes();
}

int smi_lists_regroup(const void* old_rows, const float* old_aux, const int32_t* old_ids, const int32_t* old_offsets,
                    int64_t old_slots, int64_t old_rows_bound, const void* new_rows, const float* new_aux,
                    const int32_t* new_labels, const int32_t* new_ids, int32_t new_id_base, int64_t n_new, int32_t row_bytes,
                    int64_t K, void* list_rows, float* list_aux, int32_t* list_ids, int64_t capacity_slots, int32_t* list_offsets,
                    int32_t* list_sizes, void* ws, int64_t ws_bytes, void* stream) {
  return regroup_entry(old_rows, old_aux, old_ids, old_offsets, old_slots, old_rows_bound, new_rows, new_aux, new_labels, new_ids,
                       new_id_base, n_new, row_bytes, K, list_rows, list_aux, list_ids, capacity_slots, list_offsets, list_sizes, ws,
                       ws_bytes, stream);
}

// ---------------------------------------------------------------- L2 over the product-quantised lists
int smi_l2_pq_bias(const void* codes, int64_t n, int32_t d, int32_t dsub, const void* codebooks, const int32_t* slot_ids,
                   const int32_t* list_offsets, const int32_t* labels, const void* centroids, int64_t K, float* out,
                   void* stream) {
  return pq_l2_bias_entry(codes, n, d, dsub, codebooks, slot_ids, list_offsets, labels, centroids, K, out, stream);
}

int64_t smi_l2_pq_search_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d, int32_t dsub) {
  const KeepLastError keep;
  const bool refused = check_search_args(nq, d, K, nprobe, k) || pq_check_dsub(d, dsub);
  return refused ? 0 : (int64_t)SearchWs(nullptr, nq, K, nprobe, k).bytes();
}

int smi_l2_pq_search(const void* q_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_codes,
                     int32_t dsub, const void* codebooks, const float* list_bias, const int32_t* list_ids,
                     const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* ws, int64_t ws_bytes,
                     void* stream) {
  return pq_l2_search_entry<false>(q_f16, nq, d, probes, nullptr, nprobe, list_codes, dsub, codebooks, list_bias, list_ids,
                                   list_offsets, K, k, idx, score, ws, ws_bytes, stream);
}

int smi_l2_pq_search_residual(const void* q_f16, int64_t nq, int32_t d, const int32_t* probes, const float* coarse,
                              int32_t nprobe, const void* list_codes, int32_t dsub, const void* codebooks, const float* list_bias,
                              const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx,
                              float* score, void* ws, int64_t ws_bytes, void* stream) {
  return pq_l2_search_entry<true>(q_f16, nq, d, probes, coarse, nprobe, list_codes, dsub, codebooks, list_bias, list_ids,
                                  list_offsets, K, k, idx, score, ws, ws_bytes, stream);
}

}  // extern "C"
