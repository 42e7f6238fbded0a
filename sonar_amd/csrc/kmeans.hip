// Spherical k-means over rows of smi_xsim_normalize.  The assignment step is smi_xsim_topk with k = 1
// against the normalised centroids, unchanged.  New here: the centroid update (a scatter-reduce of n fp16 rows into K
// sums), the finalise step and the round loop that strings them on one stream.
//
// The update is EXACT.  Every finite fp16 value is an integer multiple of 2^-24, so x * 2^24 is an integer (|.| <= 2^24
// for |x| <= 1, < 2^41 for any finite x) and the int64 sum of any number of rows is the same integer whatever the order,
// grid or chunking.  Integer atomics are therefore as reproducible here as a fixed-order sum.
//
// Mechanism (sized in DESIGN.md 3.17): adding every element with a global atomic would be n * d atomics (1e9 per million
// rows).  Instead the row numbers are bucketed by label -- histogram, exclusive scan, cursor scatter (bucket.hpp), all with
// wave-aggregated int32 atomics (one atomic per distinct label of a wave, so one huge cluster costs n / 64 of them) -- and
// every work unit, ONE WAVE, takes KM_UNIT consecutive positions of the bucketed order, gathers their rows with 16-byte
// loads and accumulates in registers (exactly, see the kernel).  A unit adds its registers to `sums` when the label changes
// and at its end:
// at most n / KM_UNIT + K flushes of d int64 atomics, each wave instruction 512 contiguous bytes (through an LDS
// transpose).  A unit is a run of positions, not of one cluster: a cluster holding every row is spread over n / KM_UNIT
// units, and a thousand tiny clusters share a few.
#include <algorithm>

#include "api_common.hpp"
#include "common.hpp"
#include "bucket.hpp"
#include "l2_rows.hpp"

using namespace smi;
using namespace smi_host;

namespace smi {

namespace {

constexpr int KM_TB = 256;    // threads per block of every kernel here
constexpr int KM_UNIT = 64;   // SMI_KMEANS_UNIT_ROWS: positions of the bucketed order one work unit (one wave) takes
constexpr int KM_NV = 2;      // 16-byte vectors per lane and column pass: a pass covers 64 * 8 * KM_NV = 1024 columns
constexpr int KM_PASS = 64 * 8 * KM_NV;
constexpr int KM_PARTS = 256; // fixed partitions of the objective sum

static_assert(KM_UNIT == 64, "a unit's row numbers and labels live one per lane; its fp64 partial sums need KM_UNIT <= 2^12");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Does one of the 8 fp16 of w have an all-ones exponent (Inf / NaN)?  Per half (h & 0x7c00) + 0x0400 reaches bit 15 only
// then, and never carries into the other half.
__device__ __forceinline__ bool km_has_nonfinite(u32x4 w) {
  unsigned t = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) t |= (w[j] & 0x7c007c00u) + 0x04000400u;
  return (t & 0x80008000u) != 0;
}
// ... then those halves become +0 (the rare path).
__device__ __forceinline__ u32x4 km_zero_nonfinite(u32x4 w) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned lo = w[j] & 0xffffu, hi = w[j] >> 16;
    if ((lo & 0x7c00u) == 0x7c00u) lo = 0;
    if ((hi & 0x7c00u) == 0x7c00u) hi = 0;
    w[j] = lo | (hi << 16);
  }
  return w;
}

// cursor[c] = number of valid rows with a label below c; *total = number of valid rows (bucket.hpp's one-block scan)
__global__ __launch_bounds__(KM_TB) void km_scan_kernel(const int32_t* __restrict__ counts, int K,
                                                        int32_t* __restrict__ cursor, int32_t* __restrict__ total) {
  bucket_scan<KM_TB, 1>(
      K, [&](int i, int(&v)[1]) { v[0] = counts[i]; }, [&](int i, const int(&run)[1]) { cursor[i] = run[0]; },
      [&](const int(&run)[1]) { *total = run[0]; });
}

// One wave = one work unit: positions [u * KM_UNIT, (u + 1) * KM_UNIT) of the bucketed order.  Lane l of a column pass owns
// columns cb + (k * 64 + l) * 8 .. + 8, k < KM_NV (one 16-byte load each), 8 * KM_NV accumulators.  Inside a unit the
// accumulators are fp64 and still exact: every addend is a multiple of 2^-24 below 2^16, so a sum of at most KM_UNIT = 64 of
// them is a multiple of 2^-24 below 2^22 -- 46 significant bits of fp64's 53 -- and no add rounds (two conversions and one
// add per element, where the integer route costs a 64-bit shift, a negate and a select).  It becomes an int64 at the flush,
// where the accumulators go through the wave's own LDS slab so that lane l adds column cb + j * 64 + l: 512 contiguous bytes per
// atomic instruction.  No block barrier anywhere: the waves of a block are independent.
__global__ __launch_bounds__(KM_TB) void km_accumulate_kernel(const f16* __restrict__ xn, int d,
                                                              const int32_t* __restrict__ order,
                                                              const int32_t* __restrict__ olab,
                                                              const int32_t* __restrict__ total,
                                                              unsigned long long* __restrict__ sums) {
  __shared__ long long slab[KM_TB / 64][KM_PASS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = ((int64_t)blockIdx.x * (KM_TB / 64) + wave) * KM_UNIT;
  const int64_t m = *total;
  if (p0 >= m) return;
  const int cnt = (int)(m - p0 < KM_UNIT ? m - p0 : KM_UNIT);
  const int my_row = lane < cnt ? order[p0 + lane] : 0;
  const int my_lab = lane < cnt ? olab[p0 + lane] : 0;
  long long* st = slab[wave];

  for (int cb = 0; cb < d; cb += KM_PASS) {
    double acc[KM_NV][8];
#pragma unroll
    for (int k = 0; k < KM_NV; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[k][e] = 0.0;
    bool live[KM_NV];
#pragma unroll
    for (int k = 0; k < KM_NV; ++k) live[k] = cb + (k * 64 + lane) * 8 < d;

    auto flush = [&](int c) {
#pragma unroll
      for (int k = 0; k < KM_NV; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) st[(k * 64 + lane) * 8 + e] = (long long)(acc[k][e] * 0x1p24);  // exact: see above
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      unsigned long long* row = sums + (size_t)c * d + cb;
#pragma unroll
      for (int j = 0; j < 8 * KM_NV; ++j) {
        const int col = j * 64 + lane;
        const long long v = st[col];
        if (cb + col < d && v != 0) atomicAdd(row + col, (unsigned long long)v);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int k = 0; k < KM_NV; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.0;
    };

    int cur = __shfl(my_lab, 0, 64);
    for (int i = 0; i < cnt; i += 4) {
      u32x4 v[4][KM_NV];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (i + q < cnt) {
          const int r = __shfl(my_row, i + q, 64);
          const u32x4* src = (const u32x4*)(xn + (size_t)r * d + cb);
#pragma unroll
          for (int k = 0; k < KM_NV; ++k)
            if (live[k]) v[q][k] = src[k * 64 + lane];
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (i + q < cnt) {
          const int c = __shfl(my_lab, i + q, 64);
          if (c != cur) {  // wave-uniform
            flush(cur);
            cur = c;
          }
#pragma unroll
          for (int k = 0; k < KM_NV; ++k)
            if (live[k]) {
              u32x4 w = v[q][k];
              if (km_has_nonfinite(w)) w = km_zero_nonfinite(w);
              const half8 h = __builtin_bit_cast(half8, w);
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[k][e] += (double)h[e];
            }
        }
      }
    }
    flush(cur);
  }
}

// One wave per cluster.  Live = has members and a non-zero sum: its fp32 row is written, (float)sum (one round to nearest
// even) times 2^-24 (exact).  Any other cluster is counted and nothing of it is touched.
__global__ __launch_bounds__(KM_TB) void km_finalize_kernel(const long long* __restrict__ sums,
                                                            const int32_t* __restrict__ counts, int K, int d,
                                                            float* __restrict__ cf32, int32_t* __restrict__ live_flag,
                                                            int32_t* __restrict__ empty_count) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (KM_TB / 64) + (threadIdx.x >> 6);
  if (c >= K) return;  // wave-uniform
  const long long* s = sums + (size_t)c * d;
  bool nz = false;
  for (int col = lane; col < d; col += 64) nz |= s[col] != 0;
  const bool live = counts[c] > 0 && __ballot(nz) != 0;
  if (live) {
    float* o = cf32 + (size_t)c * d;
    for (int col = lane; col < d; col += 64) o[col] = (float)s[col] * 0x1p-24f;
  }
  if (lane == 0) {
    live_flag[c] = live;
    if (!live) atomicAdd(empty_count, 1);
  }
}

// dst row r = (r < K ? (live ? src row r : unchanged) : zero); one wave per row, 16 bytes per lane per access.
__global__ __launch_bounds__(KM_TB) void km_select_kernel(const f16* __restrict__ src, const int32_t* __restrict__ live_flag,
                                                          int K, int64_t rows_pad, int d, f16* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (KM_TB / 64) + (threadIdx.x >> 6);
  if (r >= rows_pad) return;
  u32x4* o = (u32x4*)(dst + (size_t)r * d);
  if (r >= K) {
    for (int c = lane; c < d / 8; c += 64) o[c] = u32x4{0u, 0u, 0u, 0u};
  } else if (live_flag[r]) {
    const u32x4* s = (const u32x4*)(src + (size_t)r * d);
    for (int c = lane; c < d / 8; c += 64) o[c] = s[c];
  }
}

// After an assignment: block b sums the scores of its fixed partition of the rows in fp64 (a thread strides its partition,
// then a fixed tree) and counts the rows whose label changed; `labels` then takes the new labels.
__global__ __launch_bounds__(KM_TB) void km_round_part_kernel(const float* __restrict__ scores,
                                                              const int32_t* __restrict__ new_labels,
                                                              int32_t* __restrict__ labels, int n, int per,
                                                              double* __restrict__ part_obj, int32_t* __restrict__ part_moved) {
  __shared__ double so[KM_TB];
  __shared__ int sm[KM_TB];
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double obj = 0.0;
  int moved = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += KM_TB) {
    obj += (double)scores[i];
    const int c = new_labels[i];
    moved += c != labels[i];
    labels[i] = c;
  }
  so[threadIdx.x] = obj;
  sm[threadIdx.x] = moved;
  __syncthreads();
  for (int w = KM_TB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      so[threadIdx.x] += so[threadIdx.x + w];
      sm[threadIdx.x] += sm[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part_obj[blockIdx.x] = so[0];
    part_moved[blockIdx.x] = sm[0];
  }
}

__global__ __launch_bounds__(KM_PARTS) void km_round_sum_kernel(const double* __restrict__ part_obj,
                                                                const int32_t* __restrict__ part_moved,
                                                                double* __restrict__ objective, int32_t* __restrict__ moved) {
  __shared__ double so[KM_PARTS];
  __shared__ int sm[KM_PARTS];
  so[threadIdx.x] = part_obj[threadIdx.x];
  sm[threadIdx.x] = part_moved[threadIdx.x];
  __syncthreads();
  for (int w = KM_PARTS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      so[threadIdx.x] += so[threadIdx.x + w];
      sm[threadIdx.x] += sm[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *objective = so[0];
    *moved = sm[0];
  }
}

// update: cursor int32 [K] | total int32 [4] | order int32 [n] | labels in bucket order int32 [n]
struct KmUpdateWs : WsLayout {
  int32_t *cursor, *total, *order, *olab;
  KmUpdateWs(void* ws, int64_t n, int64_t K) : WsLayout(ws) {
    cursor = take<int32_t>(K, 16);
    total = take<int32_t>(4, 16);
    order = take<int32_t>(n, 16);
    olab = take<int32_t>(n, 16);
  }
};
// finalise: live flags int32 [K] | fp16 rows from smi_xsim_normalize [padded K][d]
struct KmFinalizeWs : WsLayout {
  int32_t* live_flag;
  f16* tmp;
  KmFinalizeWs(void* ws, int64_t K, int d) : WsLayout(ws) {
    live_flag = take<int32_t>(K, 16);
    tmp = take<f16>((size_t)smi_xsim_padded_rows(K) * d, 16);
  }
};
// the two are never live at once: smi_kmeans_workspace_bytes
size_t km_workspace_bytes(int64_t n, int64_t K, int d) {
  return std::max(KmUpdateWs(nullptr, n, K).bytes(), KmFinalizeWs(nullptr, K, d).bytes());
}
// fit: the workspace of update and finalise | the top-1 pass's | new labels int32 [n] | the centroids' bias fp32 [bias_rows] |
//      partial objectives fp64 [KM_PARTS] | partial moved counts int32 [KM_PARTS]
struct KmFitWs : WsLayout {
  void *km_ws, *xs_ws;
  int32_t *new_labels, *part_moved;
  float* bias;
  double* part_obj;
  KmFitWs(void* ws, int64_t n, size_t km_bytes, size_t xs_bytes, int64_t bias_rows) : WsLayout(ws) {
    km_ws = take<char>(km_bytes, 16);
    xs_ws = take<char>(xs_bytes, 16);
    new_labels = take<int32_t>(n, 16);
    bias = take<float>(bias_rows, 16);
    part_obj = take<double>(KM_PARTS);
    part_moved = take<int32_t>(KM_PARTS);
  }
};
// the spherical fit: update and finalise share their workspace, the pass is smi_xsim_topk's at k = 1, no bias
KmFitWs km_fit_ws(void* ws, int64_t n, int64_t K, int d) {
  return KmFitWs(ws, n, km_workspace_bytes(n, K, d), (size_t)smi_xsim_workspace_bytes(n, K, 1, d), 0);
}

hipError_t km_update(const f16* xn, const int32_t* labels, int n, int d, int K, long long* sums, int32_t* counts, void* ws,
                     hipStream_t stream) {
  const KmUpdateWs w(ws, n, K);
  hipError_t e;
  if ((e = hipMemsetAsync(counts, 0, (size_t)K * 4, stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(sums, 0, (size_t)K * d * 8, stream)) != hipSuccess) return e;
  const dim3 rows_grid = grid_for(n, KM_TB), block(KM_TB);
  // order[p] = a row number, olab[p] = its label, the rows of a cluster at consecutive p.  Which member lands where inside
  // its cluster's run depends on the atomics' arrival order; the sums do not.
  hipLaunchKernelGGL(bucket_hist_kernel<KM_TB>, rows_grid, block, 0, stream, labels, n, K, counts);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), block, 0, stream, counts, K, w.cursor, w.total);
  hipLaunchKernelGGL(bucket_scatter_kernel<KM_TB>, rows_grid, block, 0, stream, labels, n, K, w.cursor, w.order, w.olab);
  // units for all n rows: those past the number of valid rows find nothing to do
  const int64_t units = ((int64_t)n + KM_UNIT - 1) / KM_UNIT;
  hipLaunchKernelGGL(km_accumulate_kernel, grid_for(units, KM_TB / 64), block, 0, stream, xn, d, w.order, w.olab, w.total,
                     (unsigned long long*)sums);
  return hipGetLastError();
}

hipError_t km_finalize(const long long* sums, const int32_t* counts, int K, int d, float* cf32, f16* cf16,
                       int32_t* empty_count, void* ws, hipStream_t stream) {
  const KmFinalizeWs w(ws, K, d);
  const int64_t rows_pad = smi_xsim_padded_rows(K);
  hipError_t e;
  if ((e = hipMemsetAsync(empty_count, 0, 4, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(km_finalize_kernel, grid_for(K, KM_TB / 64), dim3(KM_TB), 0, stream, sums, counts, K, d, cf32, w.live_flag,
                     empty_count);
  // the fp16 rows are smi_xsim_normalize's, of every fp32 row; only the live ones are taken over
  if ((e = launch_l2_normalize(cf32, 1, w.tmp, K, d, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(km_select_kernel, grid_for(rows_pad, KM_TB / 64), dim3(KM_TB), 0, stream, w.tmp, w.live_flag, K, rows_pad, d,
                     cf16);
  return hipGetLastError();
}

// ---- Euclidean k-means: the update above, unchanged (its integer sums are exact for any finite fp16 rows),
// a finalise that divides by the count, and the assignment as smi_l2_topk's pass at k = 1 with the bias -h_c.
//
// One wave per row of the padded centroid matrix.  A cluster with members: centroid_f32 = fl32(fl64(sum) * 2^-24 / fl64(count))
// (int64 -> fp64 by round to nearest even, the scale exact, one correctly rounded fp64 division, one rounding to fp32), the
// fp16 row its round to nearest even, h_c = l2_half_norm of that fp16 row.  A cluster without members keeps all three and is
// counted.  Rows from K on: fp16 row and half norm zeroed.
__global__ __launch_bounds__(KM_TB) void km_l2_finalize_kernel(const long long* __restrict__ sums, const int32_t* __restrict__ counts,
                                                               int K, int64_t rows_pad, int d, float* __restrict__ cf32,
                                                               f16* __restrict__ cf16, float* __restrict__ ch,
                                                               int32_t* __restrict__ empty_count) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (KM_TB / 64) + (threadIdx.x >> 6);
  if (r >= rows_pad) return;  // wave-uniform
  half8* o = (half8*)(cf16 + (size_t)r * d);
  if (r >= K) {
    for (int c = lane; c < d / 8; c += 64) o[c] = half8{0, 0, 0, 0, 0, 0, 0, 0};
    if (lane == 0) ch[r] = 0.f;
    return;
  }
  const int cnt = counts[r];
  if (cnt <= 0) {
    if (lane == 0) atomicAdd(empty_count, 1);
    return;
  }
  const long long* s = sums + (size_t)r * d;
  float* c32 = cf32 + (size_t)r * d;
  const double n = (double)cnt;
  const float h = l2_half_norm(d, lane, [&](int c) {
    half8 v;
    f32x4 f[2];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e >> 2][e & 3] = (float)((double)s[c * 8 + e] * 0x1p-24 / n);
      v[e] = (f16)f[e >> 2][e & 3];
    }
    *(f32x4*)(c32 + c * 8) = f[0];
    *(f32x4*)(c32 + c * 8 + 4) = f[1];
    o[c] = v;
    return v;
  });
  if (lane == 0) ch[r] = h;
}

hipError_t km_l2_finalize(const long long* sums, const int32_t* counts, int K, int d, float* cf32, f16* cf16, float* ch,
                          int32_t* empty_count, hipStream_t stream) {
  const int64_t rows_pad = smi_xsim_padded_rows(K);
  hipError_t e;
  if ((e = hipMemsetAsync(empty_count, 0, 4, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(km_l2_finalize_kernel, grid_for(rows_pad, KM_TB / 64), dim3(KM_TB), 0, stream, sums, counts, K, rows_pad, d,
                     cf32, cf16, ch, empty_count);
  return hipGetLastError();
}

// the Euclidean fit: its finalise needs no workspace, the pass is smi_l2_topk's at k = 1, one bias per padded centroid row
KmFitWs km_l2_fit_ws(void* ws, int64_t n, int64_t K, int d) {
  return KmFitWs(ws, n, KmUpdateWs(nullptr, n, K).bytes(), l2_topk_ws_bytes(smi_xsim_padded_rows(n), smi_xsim_padded_rows(K), 1, d),
                 smi_xsim_padded_rows(K));
}

// A fit, stated once: `resume` = 0 starts from centroids_f32 (start(st) makes the metric's fp16 centroids of them and one
// assignment is recorded in slot 0), then n_iter rounds of update, finalize(it, w, st) and an assignment.  An assignment is
// nearest(w, st), the metric's top-1 pass into w.new_labels and scores (ties to the lower index), and the round's record:
// the objective and how many rows moved.  null_arg, refusals (they follow the checks of n_iter and resume), layout and its
// sizing call are the entry's own.
template <class Refusals, class Start, class Finalize, class Nearest>
int km_fit(bool null_arg, const void* x, int64_t n, int32_t d, int64_t K, int32_t n_iter, int32_t resume, int32_t* labels, float* scores,
           int64_t* sums, int32_t* counts, double* objective, int32_t* moved, void* ws, int64_t ws_bytes, void* stream,
           KmFitWs (*layout)(void*, int64_t, int64_t, int), const char* sizing, Refusals refusals, Start start, Finalize finalize,
           Nearest nearest) {
  if (null_arg || !x || !labels || !scores || !sums || !counts || !objective || !moved)
    return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_shape(n, nullptr, d, K, "cluster")) return rc;
  if (n_iter < 0) return fail(SMI_ERR_INVALID_ARG, "n_iter=%d", n_iter);
  if (resume != 0 && resume != 1) return fail(SMI_ERR_INVALID_ARG, "resume=%d (0 or 1)", resume);
  if (const int rc = refusals()) return rc;
  const KmFitWs w = layout(ws, n, K, d);
  if (const int rc = check_ws(ws, ws_bytes, w.bytes(), sizing)) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t st = (hipStream_t)stream;
  const int per = (int)((n + KM_PARTS - 1) / KM_PARTS);

  auto assign = [&](int slot) -> int {
    HIP_TRY(nearest(w, st));
    hipLaunchKernelGGL(km_round_part_kernel, dim3(KM_PARTS), dim3(KM_TB), 0, st, scores, w.new_labels, labels, (int)n, per,
                       w.part_obj, w.part_moved);
    hipLaunchKernelGGL(km_round_sum_kernel, dim3(1), dim3(KM_PARTS), 0, st, w.part_obj, w.part_moved, objective + slot,
                       moved + slot);
    HIP_TRY(hipGetLastError());
    return SMI_OK;
  };

  int slot = 0;
  if (!resume) {
    HIP_TRY(start(st));
    HIP_TRY(hipMemsetAsync(labels, 0xff, (size_t)n * 4, st));  // -1: every row counts as moved
    if (const int rc = assign(slot++)) return rc;
  }
  for (int it = 0; it < n_iter; ++it) {
    HIP_TRY(km_update((const f16*)x, labels, (int)n, d, (int)K, (long long*)sums, counts, w.km_ws, st));
    HIP_TRY(finalize(it, w, st));
    if (const int rc = assign(slot++)) return rc;
  }
  return SMI_OK;
}

}  // namespace

}  // namespace smi

extern "C" {

// (a sizing function asks the entries' shape check, and leaves smi_last_error() as it was)
int64_t smi_kmeans_workspace_bytes(int64_t n, int64_t K, int32_t d) {
  const KeepLastError keep;
  return check_shape(n, nullptr, d, K, "cluster") ? 0 : (int64_t)km_workspace_bytes(n, K, d);
}

int smi_kmeans_update(const void* xn, const int32_t* labels, int64_t n, int32_t d, int64_t K, int64_t* sums,
                      int32_t* counts, void* ws, int64_t ws_bytes, void* stream) {
  if (!xn || !labels || !sums || !counts) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_shape(n, nullptr, d, K, "cluster")) return rc;
  if (const int rc = check_ws(ws, ws_bytes, smi_kmeans_workspace_bytes(n, K, d), "smi_kmeans_workspace_bytes(n, K, d)"))
    return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(km_update((const f16*)xn, labels, (int)n, d, (int)K, (long long*)sums, counts, ws, (hipStream_t)stream));
  return SMI_OK;
}

int smi_kmeans_finalize(const int64_t* sums, const int32_t* counts, int64_t K, int32_t d, float* centroids_f32,
                        void* centroids_f16, int32_t* empty_count, void* ws, int64_t ws_bytes, void* stream) {
  if (!sums || !counts || !centroids_f32 || !centroids_f16 || !empty_count) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_shape(1, nullptr, d, K, "cluster")) return rc;
  if (const int rc = check_ws(ws, ws_bytes, smi_kmeans_workspace_bytes(1, K, d), "smi_kmeans_workspace_bytes(1, K, d)"))
    return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(km_finalize((const long long*)sums, counts, (int)K, d, centroids_f32, (f16*)centroids_f16, empty_count, ws,
                      (hipStream_t)stream));
  return SMI_OK;
}

int smi_kmeans_fit(const void* xn, int64_t n, int32_t d, int64_t K, int32_t n_iter, int32_t resume, float* centroids_f32,
                   void* centroids_f16, int32_t* labels, float* scores, int64_t* sums, int32_t* counts, double* objective,
                   int32_t* moved, int32_t* empty, void* ws, int64_t ws_bytes, void* stream) {
  const int64_t n_pad = smi_xsim_padded_rows(n), k_pad = smi_xsim_padded_rows(K);
  return km_fit(
      !centroids_f32 || !centroids_f16 || !empty, xn, n, d, K, n_iter, resume, labels, scores, sums, counts, objective, moved, ws,
      ws_bytes, stream, km_fit_ws,
      "smi_kmeans_workspace_bytes(n, K, d) + smi_xsim_workspace_bytes(n, K, 1, d) + 4 n (each rounded up to 16) + 3072",
      [] { return (int)SMI_OK; },
      [&](hipStream_t st) { return launch_l2_normalize(centroids_f32, 1, (f16*)centroids_f16, K, d, st); },
      [&](int it, const KmFitWs& w, hipStream_t st) {
        return km_finalize((const long long*)sums, counts, (int)K, d, centroids_f32, (f16*)centroids_f16, empty + it, w.km_ws, st);
      },
      [&](const KmFitWs& w, hipStream_t st) {
        return launch_xsim_topk((const f16*)xn, n, n_pad, (const f16*)centroids_f16, K, k_pad, d, 1, 0, w.new_labels, scores,
                                w.xs_ws, st);
      });
}

// ---- Euclidean k-means
int smi_l2_kmeans_finalize(const int64_t* sums, const int32_t* counts, int64_t K, int32_t d, float* centroids_f32,
                           void* centroids_f16, float* centroid_half_norms, int32_t* empty_count, void* stream) {
  if (!sums || !counts || !centroids_f32 || !centroids_f16 || !centroid_half_norms || !empty_count)
    return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_shape(1, nullptr, d, K, "cluster")) return rc;
  if (((uintptr_t)centroids_f32 | (uintptr_t)centroids_f16) % 16)
    return fail(SMI_ERR_INVALID_ARG, "centroids_f32 and centroids_f16 must be 16-byte aligned");
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(km_l2_finalize((const long long*)sums, counts, (int)K, d, centroids_f32, (f16*)centroids_f16, centroid_half_norms,
                         empty_count, (hipStream_t)stream));
  return SMI_OK;
}

int64_t smi_l2_kmeans_fit_ws_bytes(int64_t n, int64_t K, int32_t d) {
  const KeepLastError keep;
  return check_shape(n, nullptr, d, K, "cluster") ? 0 : (int64_t)km_l2_fit_ws(nullptr, n, K, d).bytes();
}

int smi_l2_kmeans_fit(const void* x_f16, int64_t n, int32_t d, int64_t K, int32_t n_iter, int32_t resume, float* centroids_f32,
                      void* centroids_f16, float* centroid_half_norms, int32_t* labels, float* scores, int64_t* sums,
                      int32_t* counts, double* objective, int32_t* moved, int32_t* empty, void* ws, int64_t ws_bytes,
                      void* stream) {
  const int64_t n_pad = smi_xsim_padded_rows(n), k_pad = smi_xsim_padded_rows(K);
  return km_fit(
      !centroids_f32 || !centroids_f16 || !centroid_half_norms || !empty, x_f16, n, d, K, n_iter, resume, labels, scores, sums,
      counts, objective, moved, ws, ws_bytes, stream, km_l2_fit_ws, "smi_l2_kmeans_fit_ws_bytes(n, K, d)",
      [&] {
        return ((uintptr_t)x_f16 | (uintptr_t)centroids_f32 | (uintptr_t)centroids_f16) % 16
                   ? fail(SMI_ERR_INVALID_ARG, "x_f16, centroids_f32 and centroids_f16 must be 16-byte aligned")
                   : (int)SMI_OK;
      },
      [&](hipStream_t st) { return launch_l2_prepare(centroids_f32, 1, (f16*)centroids_f16, centroid_half_norms, K, d, st); },
      [&](int it, const KmFitWs&, hipStream_t st) {
        return km_l2_finalize((const long long*)sums, counts, (int)K, d, centroids_f32, (f16*)centroids_f16, centroid_half_norms,
                              empty + it, st);
      },
      [&](const KmFitWs& w, hipStream_t st) {  // the biased top-1 with b = -h_c
        if (hipError_t e = launch_l2_neg_gather(nullptr, k_pad, centroid_half_norms, w.bias, st); e != hipSuccess) return e;
        return launch_l2_topk((const f16*)x_f16, n, n_pad, (const f16*)centroids_f16, K, k_pad, d, 1, 0, w.bias, w.new_labels,
                              scores, w.xs_ws, st);
      });
}

}  // extern "C"
