// xsim cosine-similarity mining: for every row of X find the k most similar
// rows of Y (cosine = dot product of L2-normalised rows).  The reference only
// names xsim (README.md:5); its in-tree form is F.normalize(x) @ F.normalize(y).T
// (tests/integration_tests/test_text_sonar.py:42-53).  Here the Nx x Ny score
// matrix is never materialised: each 256x256 score tile comes out of the
// shared MFMA tile engine straight into a running top-k (registers at k = 1,
// per-row lists in LDS for k >= 2), so HBM traffic stays ~(Nx+Ny)*d*2 B and the
// kernel is MFMA-bound (2*d flop per pair).
//
// Work split: grid = (x tiles) x (y chunks); a workgroup walks the y tiles of
// its chunk.  The grouped XCD raster makes the ~64 workgroups resident on one
// XCD an 8(x) x 8(chunk) block: its 8 X panels stay L2-resident for the whole
// walk and every streamed Y tile is shared by 8 workgroups.
//
// The tile walk itself, the LDS key lists and the host side of a pass are xsim_walk.hpp's, shared with the int8 pass
// (xsim_i8.hip); this file holds the fp16 operand policy with its top-1 register lists, the chunk merge, and the kernels
// around the pass (normalise, k-way shard merge, margin re-scoring).
#include "api_common.hpp"
#include "gemm_tile.hpp"
#include "kernels.hpp"
#include "xsim_walk.hpp"

namespace smi {

#ifdef SMI_XSIM_TRACE
// development aid (-DSMI_XSIM_TRACE, tools/xsim_trace.py): what the walk records of the fp16 kernel (xsim_walk.hpp)
__device__ unsigned long long xs_trace_buf[256 * 2 * 4];
#endif

// The fp16 operand policy of the walk (xsim_walk.hpp): a score is the fp32 sum itself.
// K >= 2: the running top-k lists live in LDS, one per row.  K = 1: per-lane lists in registers (16 VGPRs, no
// pressure there: 436.7 vs 439.6 ms with LDS lists at 262 144 x 1 M; profiles/r04_experiments.txt, experiment 2)
template <int K>
struct XsF16 {
  typedef f16 elem_t;
  typedef half8 frag_t;
  typedef f32x4 acc_t;
  static constexpr int BK = G2_BK;
  static constexpr bool LISTS = K >= 2;
  static constexpr int LDS_ABOVE = LISTS ? 256 * K * 8 : 4096;  // the row lists, or the row thresholds of top-1
  static constexpr bool TRACED = true;
#ifdef SMI_XSIM_TRACE
  static __device__ __forceinline__ unsigned long long* trace_buf() { return xs_trace_buf; }
#endif
  static __device__ __forceinline__ acc_t mfma(frag_t w, frag_t x, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, x, c, 0, 0, 0);
  }
  __device__ __forceinline__ void issue_tile(char*, int) {}
  struct tile_t {};
  __device__ __forceinline__ void fold_begin(int, tile_t&) {}
  __device__ __forceinline__ float row_max(const acc_t (&acc)[4][8], int mi, tile_t) const {
    float vmax = -INFINITY;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) vmax = fmaxf(vmax, acc[ni][mi][r]);
    return vmax;
  }
  __device__ __forceinline__ float score(const acc_t (&acc)[4][8], int ni, int mi, int r, tile_t) const { return acc[ni][mi][r]; }

  // ---- top-1: one running best per accumulator row block, in registers
  TopK<1> best[8];
  // Row thresholds shared by the 4 column waves (above the ring): thr[row][wc] = the best score wave wc holds for that row, a
  // lower bound of the row's best.  Published and read WITHOUT a barrier: the values only grow, so a stale one is still a
  // valid bound.  A lane's own best is a much weaker test -- with it some lane of nearly every 16-row block passes and the
  // whole wave walks the insertion path every tile (r02 experiment 24).
  __device__ __forceinline__ void init(const XsLane& L, char* above, int, int) {
    if constexpr (!LISTS) {
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) best[mi].init();
      float* thr = (float*)above;
      if (L.kg == 0) {
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) thr[L.row(mi) * 4 + L.wc] = -INFINITY;
      }
    }
  }
  __device__ __forceinline__ void top1_fold(const acc_t (&acc)[4][8], const XsLane L, char* above, int n0f, int ny) {
    float* thr = (float*)above;
    float rowthr[8];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      float my = best[mi].s[0];
      my = fmaxf(my, __shfl_xor(my, 16, 64));
      my = fmaxf(my, __shfl_xor(my, 32, 64));
      if (L.kg == 0) thr[L.row(mi) * 4 + L.wc] = my;
    }
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      const f32x4 t4 = *(const f32x4*)(thr + L.row(mi) * 4);
      rowthr[mi] = fmaxf(fmaxf(t4[0], t4[1]), fmaxf(t4[2], t4[3]));
    }
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      if (row_max(acc, mi, tile_t{}) >= rowthr[mi]) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = L.col(ni, r, n0f);
            if (n < ny) best[mi].push(acc[ni][mi][r], n);
          }
      }
    }
  }
  // a row's candidates sit in the 4 lane groups (kg) of 4 column waves: join the lane groups with xor-shuffles (both partners
  // end with the merged list), then the 4 waves through LDS; row r of the tile goes to ps / pi [o0 + r]
  __device__ __forceinline__ void top1_write(const XsLane& L, char* smem, size_t o0, float* __restrict__ ps,
                                             int* __restrict__ pi) {
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
      for (int step = 16; step <= 32; step <<= 1) {
        const float os = __shfl_xor(best[mi].s[0], step, 64);
        const int oi = __shfl_xor(best[mi].i[0], step, 64);
        best[mi].push(os, oi);
      }
    }
    __syncthreads();
    float* ls = (float*)smem;  // [256 rows][4 waves]
    int* li = (int*)(smem + 256 * 4 * 4);
    if (L.kg == 0) {
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        ls[L.row(mi) * 4 + L.wc] = best[mi].s[0];
        li[L.row(mi) * 4 + L.wc] = best[mi].i[0];
      }
    }
    __syncthreads();
    if (L.tid < 256) {
      TopK<1> t;
      t.init();
      for (int c = 0; c < 4; ++c) t.push(ls[L.tid * 4 + c], li[L.tid * 4 + c]);
      ps[o0 + L.tid] = t.s[0];
      pi[o0 + L.tid] = t.i[0];
    }
  }
};

template <int K>
__global__ __launch_bounds__(G2_THREADS) void xsim_tile256_kernel(const f16* __restrict__ Xn,
                                                                  const f16* __restrict__ Yn, int d,
                                                                  int ntx, int nty, int nchunks,
                                                                  int tiles_per_chunk, int ny,
                                                                  int nx_pad, float* __restrict__ ps,
                                                                  int* __restrict__ pi) {
  XsF16<K> p;
  xsim_walk<K>(p, Xn, Yn, d, ntx, nty, nchunks, tiles_per_chunk, ny, nx_pad, ps, pi);
}

// final merge over chunks; one thread per x row.  k_out <= K.
template <int K>
__global__ __launch_bounds__(256) void xsim_merge_kernel(const float* __restrict__ ps,
                                                         const int* __restrict__ pi, int nchunks,
                                                         int64_t nx, int nx_pad, int k_out,
                                                         int64_t y_off, int32_t* __restrict__ idx,
                                                         float* __restrict__ score) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= nx) return;
  TopK<K> t;
  t.init();
  for (int c = 0; c < nchunks; ++c) {
    const size_t o = ((size_t)c * nx_pad + row) * K;
#pragma unroll
    for (int j = 0; j < K; ++j) t.push(ps[o + j], pi[o + j]);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j < k_out) {
      const bool valid = t.i[j] != 0x7fffffff;
      idx[row * k_out + j] = valid ? (int32_t)(t.i[j] + y_off) : -1;
      score[row * k_out + j] = t.s[j];
    }
  }
}

hipError_t launch_xsim_merge(const float* ps, const int* pi, int nchunks, int64_t nx, int nx_pad, int k, int64_t y_off,
                             int32_t* idx, float* score, hipStream_t stream) {
  return xs_with_k(k, [&](auto K) {
    hipLaunchKernelGGL(xsim_merge_kernel<K()>, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, stream, ps, pi, nchunks, nx,
                       nx_pad, k, y_off, idx, score);
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------- normalise
// dst[r,:] = f16(src[r,:] / max(||src[r,:]||, 1e-12)), rows >= n_valid zeroed.
template <typename T>
__global__ __launch_bounds__(256) void l2norm_kernel(const T* __restrict__ src, f16* __restrict__ dst,
                                                     int64_t rows, int64_t rows_pad, int d) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows_pad) return;
  f16* o = dst + r * d;
  if (r >= rows) {
    for (int c = lane; c < d; c += 64) o[c] = (f16)0.f;
    return;
  }
  const T* s = src + r * d;
  // fast path (d = 1024 in SONAR): one pass, 16 B per lane per access, the row stays in registers
  constexpr int VEC = 16 / sizeof(T);      // elements per 16-B access
  constexpr int MAXV = 4;                  // up to d = 64 * VEC * MAXV
  if (d % (64 * VEC) == 0 && d <= 64 * VEC * MAXV && d % 512 == 0) {
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const int nv = d / (64 * VEC);
    vec_t v[MAXV];
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MAXV; ++k)
      if (k < nv) {
        v[k] = *(const vec_t*)(s + (k * 64 + lane) * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) q += (float)v[k][e] * (float)v[k][e];
      }
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(q)), 1e-12f);
    if constexpr (VEC == 8) {
#pragma unroll
      for (int k = 0; k < MAXV; ++k)
        if (k < nv) {
          half8 h;
#pragma unroll
          for (int e = 0; e < 8; ++e) h[e] = (f16)((float)v[k][e] * inv);
          *(half8*)(o + (k * 64 + lane) * 8) = h;
        }
    } else {  // fp32 source: two 16-B loads make one 16-B store -- pair the accesses of lanes' chunks
#pragma unroll
      for (int k = 0; k < MAXV; ++k)
        if (k < nv) {
          half4 h;
#pragma unroll
          for (int e = 0; e < 4; ++e) h[e] = (f16)((float)v[k][e] * inv);
          *(half4*)(o + (k * 64 + lane) * 4) = h;
        }
    }
    return;
  }
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = (float)s[c];
    q += v * v;
  }
  const float inv = 1.0f / fmaxf(sqrtf(wave_sum(q)), 1e-12f);
  for (int c = lane; c < d; c += 64) o[c] = (f16)((float)s[c] * inv);
}

hipError_t launch_l2_normalize(const void* src, int src_is_f32, f16* dst, int64_t rows, int d,
                               hipStream_t stream) {
  const int64_t rows_pad = (rows + G2_BM - 1) / G2_BM * G2_BM;
  if (rows_pad == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((rows_pad + 3) / 4);
  if (src_is_f32)
    hipLaunchKernelGGL(l2norm_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float*)src,
                       dst, rows, rows_pad, d);
  else
    hipLaunchKernelGGL(l2norm_kernel<f16>, dim3(blocks), dim3(256), 0, stream, (const f16*)src, dst,
                       rows, rows_pad, d);
  return hipGetLastError();
}

// ------------------------------------------------- k-way merge of per-shard top-k lists
// part_score / part_idx: [parts][n][k], every list sorted (score desc, index asc) -- what smi_xsim_topk
// returns.  out: the k best of the union in the same total order.  One thread per row; used to fold the
// per-rank partial y-side neighbour lists of the sharded margin scoring.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ ps, const int32_t* __restrict__ pi,
                                                         int parts, int64_t n, int k, float* __restrict__ os,
                                                         int32_t* __restrict__ oi) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int head[64];
  for (int p = 0; p < parts; ++p) head[p] = 0;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bi = 0x7fffffff, bp = -1;
    for (int p = 0; p < parts; ++p) {
      if (head[p] >= k) continue;
      const size_t o = ((size_t)p * n + r) * k + head[p];
      const float v = ps[o];
      const int id = pi ? pi[o] : p * k + head[p];
      if (bp < 0 || v > bv || (v == bv && id < bi)) {
        bv = v;
        bi = id;
        bp = p;
      }
    }
    if (bp >= 0) ++head[bp];
    os[r * k + j] = bv;
    if (oi) oi[r * k + j] = bp >= 0 && pi ? bi : -1;
  }
}

hipError_t launch_topk_merge(const float* ps, const int32_t* pi, int parts, int64_t n, int k, float* os, int32_t* oi,
                             hipStream_t stream) {
  if (parts < 1 || parts > 64 || k < 1 || k > 8 || n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ps, pi, parts, n, k,
                     os, oi);
  return hipGetLastError();
}

// ------------------------------------------------- margin re-scoring of the k-NN candidates
// LASER xsim (source/xsim.py: _score_margin / _score_knn): for x_i and its k nearest y candidates,
//   score(i, j) = margin(cos(x_i, y_j), (mean_kNN(x_i) + mean_kNN(y_j)) / 2),
// margin = ratio a / b, distance a - b, or (kind 2) the plain cosine a; the prediction is the candidate
// with the best score (first one on ties, as numpy's argmax).  mean_kNN(x_i) is the mean of x_i's own k
// forward scores, mean_kNN(y_j) the mean of y_j's k backward scores bwd[j][:].
// err_count (nullable) accumulates the rows whose prediction is not the aligned index i + x_off.
__global__ __launch_bounds__(256) void margin_select_kernel(const float* __restrict__ fs, const int32_t* __restrict__ fi,
                                                            int64_t nx, int k, const float* __restrict__ bwd,
                                                            int64_t ny, int kind, int64_t x_off,
                                                            int32_t* __restrict__ pred, float* __restrict__ pm,
                                                            int32_t* __restrict__ err_count) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int wrong = 0;
  if (r < nx) {
    float xm = 0.f;
    for (int j = 0; j < k; ++j) xm += fs[r * k + j];
    xm /= (float)k;
    float best = -INFINITY;
    int bj = 0;
    for (int j = 0; j < k; ++j) {
      const float a = fs[r * k + j];
      const int64_t y = fi[r * k + j];
      float m = a;
      if (kind != 2) {
        float ym = 0.f;
        if (y >= 0 && y < ny)
          for (int q = 0; q < k; ++q) ym += bwd[y * k + q];
        ym /= (float)k;
        const float b = 0.5f * (xm + ym);
        m = kind == 0 ? a / b : a - b;
      }
      if (j == 0 || m > best) {
        best = m;
        bj = j;
      }
    }
    const int p = fi[r * k + bj];
    pred[r] = p;
    if (pm) pm[r] = best;
    wrong = (int64_t)p != r + x_off;
  }
  if (err_count) {
    const unsigned long long bal = __ballot(wrong);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(err_count, (int)__popcll(bal));
  }
}

hipError_t launch_margin_select(const float* fs, const int32_t* fi, int64_t nx, int k, const float* bwd, int64_t ny,
                                int kind, int64_t x_off, int32_t* pred, float* pm, int32_t* err_count,
                                hipStream_t stream) {
  if (nx <= 0 || k < 1 || k > 8 || kind < 0 || kind > 2 || (kind != 2 && (!bwd || ny <= 0))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(margin_select_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, stream, fs, fi, nx, k, bwd,
                     ny, kind, x_off, pred, pm, err_count);
  return hipGetLastError();
}

// the fp16 pass sizes its lists by one chunk per GT_BN = 128 rows of Yn (XsimWs, xsim_walk.hpp)
size_t xsim_workspace_bytes(int64_t nx_pad, int64_t ny_pad, int k, int d) {
  return XsimWs(nullptr, nx_pad, ny_pad, round_k(k), (int64_t)d * sizeof(f16), GT_BN).bytes();
}

hipError_t launch_xsim_topk(const f16* Xn, int64_t nx, int64_t nx_pad, const f16* Yn, int64_t ny,
                            int64_t ny_pad, int d, int k, int64_t y_off, int32_t* idx, float* score,
                            void* ws, hipStream_t stream) {
  if (nx <= 0 || ny <= 0 || k < 1 || k > 8 || d % GT_BK || nx_pad % GT_BM || ny_pad % GT_BN ||
      ny_pad > 0x7fffff00LL || nx_pad > 0x7fffff00LL || nx_pad % G2_BM || ny_pad % G2_BN)
    return hipErrorInvalidValue;
  return xs_with_k(k, [&](auto K) {
    return xsim_run(
        Xn, nx, nx_pad, Yn, ny, ny_pad, (int64_t)d * sizeof(f16), GT_BN, k, y_off, idx, score, ws, stream,
        [&](dim3 grid, const XsimWs& w, int ntx, int nty, int nchunks, int tpc) {
          constexpr int lds = G2_LDS_BYTES + XsF16<K()>::LDS_ABOVE;
          return launch_with_lds<xsim_tile256_kernel<K()>>(grid, G2_THREADS, lds, stream, (const f16*)w.xtm, (const f16*)w.ytm, d,
                                                           ntx, nty, nchunks, tpc, (int)ny, (int)nx_pad, w.ps, w.pi);
        });
  });
}

// ------------------------------------------------- paged top-k
// A page: the k <= 16 best candidates strictly BEHIND a per-row exclusive ceiling (cs, ci) in the total order.  Lists of 16
// keys fill the LDS above the ring exactly ([256][16] x 8 B = 32 KiB: 160 KiB in all), so the ceilings stay in memory, as
// packed keys, and are read on the insertion path (xs_fold_lists).  Without ceilings the pass is the plain K = 16 walk.
constexpr int XS_PAGE = 16;
static_assert(G2_LDS_BYTES + 256 * XS_PAGE * 8 == 160 * 1024, "the lists of a page fill the LDS above the ring");
static_assert(7 * 128 * XS_PAGE < 65536, "the immediate offsets of xs_thresholds fit ds_read_b32's 16-bit field");

struct XsF16Page : XsF16<XS_PAGE> {
  static constexpr bool CEILING = true;
  const unsigned long long* __restrict__ ceil;  // [nx_pad]; from init on, of the tile's rows
  __device__ __forceinline__ void init(const XsLane&, char*, int m0, int) { ceil += m0; }
  __device__ __forceinline__ unsigned long long ceiling(int row) const { return ceil[row]; }
};

__global__ __launch_bounds__(G2_THREADS) void xsim_page_tile256_kernel(const f16* __restrict__ Xn, const f16* __restrict__ Yn,
                                                                       int d, int ntx, int nty, int nchunks,
                                                                       int tiles_per_chunk, int ny, int nx_pad,
                                                                       float* __restrict__ ps, int* __restrict__ pi,
                                                                       const unsigned long long* __restrict__ ceil) {
  XsF16Page p;
  p.ceil = ceil;
  xsim_walk<XS_PAGE>(p, Xn, Yn, d, ntx, nty, nchunks, tiles_per_chunk, ny, nx_pad, ps, pi);
}

// The ceiling of every row as ONE key, in the walk's terms (y row number = returned id - y_off): a candidate is behind the
// ceiling iff its key is smaller.  ci < 0: the row is exhausted, nothing is (key 0: no key is smaller).  A ceiling need not be
// a candidate: an id in front of the walk's first row admits every row that ties the score, one behind its last row none.
// The score's zero is taken as +0, as the fold takes a candidate's.  Rows from nx on are pad rows: exhausted.
__global__ __launch_bounds__(256) void xsim_ceiling_keys_kernel(const float* __restrict__ cs, const int32_t* __restrict__ ci,
                                                                int64_t nx, int64_t nx_pad, int64_t y_off,
                                                                unsigned long long* __restrict__ keys) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nx_pad) return;
  unsigned long long key = 0ull;
  if (r < nx && ci[r] >= 0) {
    const uint32_t o = xs_ord(cs[r] + 0.0f);
    const int64_t n = (int64_t)ci[r] - y_off;
    if (n < 0) key = o == 0xffffffffu ? ~0ull : (unsigned long long)(o + 1u) << 32;
    else if (n > 0x7ffffffeLL) key = (unsigned long long)o << 32;
    else key = xs_key_ord(o, (int)n);
  }
  keys[r] = key;
}

hipError_t launch_ceiling_keys(const float* ceil_score, const int32_t* ceil_idx, int64_t n, int64_t n_pad, int64_t id_offset,
                               unsigned long long* keys, hipStream_t stream) {
  hipLaunchKernelGGL(xsim_ceiling_keys_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, stream, ceil_score, ceil_idx, n,
                     n_pad, id_offset, keys);
  return hipGetLastError();
}

// the workspace of a page: XsimWs at lists of 16 (one chunk per 256 rows of y: what the walk fills) | ceiling keys [nx_pad]
struct XsimPageWs : XsimWs {
  unsigned long long* ceil;
  XsimPageWs(void* ws, int64_t nx_pad, int64_t ny_pad, int d) : XsimWs(ws, nx_pad, ny_pad, XS_PAGE, (int64_t)d * sizeof(f16), G2_BN) {
    ceil = take<unsigned long long>((size_t)nx_pad);
  }
};

size_t xsim_page_workspace_bytes(int64_t nx_pad, int64_t ny_pad, int d) { return XsimPageWs(nullptr, nx_pad, ny_pad, d).bytes(); }

hipError_t launch_xsim_topk_page(const f16* Xn, int64_t nx, int64_t nx_pad, const f16* Yn, int64_t ny, int64_t ny_pad, int d,
                                 int k, int64_t y_off, const float* ceil_score, const int32_t* ceil_idx, int32_t* idx,
                                 float* score, void* ws, hipStream_t stream) {
  if (nx <= 0 || ny <= 0 || k < 1 || k > XS_PAGE || d % G2_BK || ny_pad > 0x7fffff00LL || nx_pad > 0x7fffff00LL ||
      nx_pad % G2_BM || ny_pad % G2_BN || !ceil_score != !ceil_idx)
    return hipErrorInvalidValue;
  const XsimPageWs w(ws, nx_pad, ny_pad, d);
  const int ntx = (int)(nx_pad / G2_BM), nty = (int)(ny_pad / G2_BN);
  const int nchunks = xsim_chunks(nty);
  const int tpc = (nty + nchunks - 1) / nchunks;
  const int64_t row_bytes = (int64_t)d * sizeof(f16);
  hipError_t e = xsim_pack((const char*)Xn, w.xtm, nx_pad, row_bytes, stream);
  if (e != hipSuccess) return e;
  e = xsim_pack((const char*)Yn, w.ytm, ny_pad, row_bytes, stream);
  if (e != hipSuccess) return e;
  constexpr int lds = G2_LDS_BYTES + XsF16<XS_PAGE>::LDS_ABOVE;
  if (ceil_idx) {
    e = launch_ceiling_keys(ceil_score, ceil_idx, nx, nx_pad, y_off, w.ceil, stream);
    if (e != hipSuccess) return e;
    e = launch_with_lds<xsim_page_tile256_kernel>(dim3(ntx * nchunks), G2_THREADS, lds, stream, (const f16*)w.xtm,
                                                  (const f16*)w.ytm, d, ntx, nty, nchunks, tpc, (int)ny, (int)nx_pad, w.ps, w.pi,
                                                  (const unsigned long long*)w.ceil);
  } else {
    e = launch_with_lds<xsim_tile256_kernel<XS_PAGE>>(dim3(ntx * nchunks), G2_THREADS, lds, stream, (const f16*)w.xtm,
                                                      (const f16*)w.ytm, d, ntx, nty, nchunks, tpc, (int)ny, (int)nx_pad, w.ps,
                                                      w.pi);
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(xsim_merge_kernel<XS_PAGE>, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, stream, w.ps, w.pi, nchunks, nx,
                     (int)nx_pad, k, y_off, idx, score);
  return hipGetLastError();
}

// launch_topk_merge for the lists of a page (k <= 16): the IVF page merges its probes' parts with it
hipError_t launch_topk_merge_page(const float* ps, const int32_t* pi, int parts, int64_t n, int k, float* os, int32_t* oi,
                                  hipStream_t stream) {
  if (parts < 1 || parts > 64 || k < 1 || k > XS_PAGE || n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ps, pi, parts, n, k,
                     os, oi);
  return hipGetLastError();
}

}  // namespace smi

#ifdef SMI_XSIM_TRACE
extern "C" int smi_debug_xsim_trace(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(smi::xs_trace_buf), sizeof(smi::xs_trace_buf));
}
#endif
