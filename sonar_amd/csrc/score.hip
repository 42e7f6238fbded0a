// Teacher-forced scoring of target texts (smi_text_decoder_score, decoder_api.hip): the embedding of a sentence group's
// packed rows and the gather of each scored row's target log-probability from the logits GEMM's tile statistics.
// Everything in between runs on the decode step's kernels.
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

namespace smi {

// ------------------------------------------------------------------ x[r] = E[id] * scale + PE[j + pos_offset]
// Row r = s * seq + j (s < nseq, j < seq) of the group; rows nseq * seq <= r < rows_pad are zero.  id = tok[s][j] for
// j < lens[s], else `fill` (a valid id: what follows a sequence is never read).  tgt[r] = tok[s][j + 1] when that token is
// inside the length (the row is scored), else -1.  An id outside [0, vocab) inside a length raises *bad and is never
// used as an index.  One wave per row.
// T = f16: the MFMA path's table, the product rounded to fp16 as dec_embed_kernel does; T = float: the fp32 flex table.
template <typename T>
__global__ __launch_bounds__(256) void score_embed_kernel(const int64_t* __restrict__ tok, int ldt,
                                                          const int32_t* __restrict__ lens, const T* __restrict__ table,
                                                          const float* __restrict__ pe, float scale, int pos_offset,
                                                          float* __restrict__ x, int32_t* __restrict__ tgt, int nseq,
                                                          int seq, int rows_pad, int d, int64_t vocab, int fill,
                                                          int32_t* __restrict__ bad) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows_pad) return;
  float* o = x + (size_t)r * d;
  if (r >= nseq * seq) {  // GEMM padding rows: finite
    for (int c = lane; c < d; c += 64) o[c] = 0.f;
    if (lane == 0) tgt[r] = -1;
    return;
  }
  const int s = r / seq, j = r - s * seq, len = lens[s];
  const int64_t* row = tok + (size_t)s * ldt;
  int64_t id = fill;
  int32_t target = -1;
  bool oob = false;
  if (j < len) {
    const int64_t v = row[j];
    if (v >= 0 && v < vocab) id = v;
    else oob = true;
  }
  if (j + 1 < len) {
    const int64_t v = row[j + 1];
    if (v >= 0 && v < vocab) target = (int32_t)v;
    else oob = true;
  }
  if (lane == 0) {
    tgt[r] = target;
    if (oob) *bad = 1;
  }
  const T* e = table + (size_t)id * d;
  const float* p = pe + (size_t)(j + pos_offset) * d;
  if constexpr (std::is_same<T, f16>::value) {
    for (int c = lane * 8; c < d; c += 512) {
      const half8 ev = *(const half8*)(e + c);
      const f32x4 p0 = *(const f32x4*)(p + c);
      const f32x4 p1 = *(const f32x4*)(p + c + 4);
      f32x4 o0, o1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o0[i] = (float)(f16)((float)ev[i] * scale) + p0[i];
        o1[i] = (float)(f16)((float)ev[i + 4] * scale) + p1[i];
      }
      *(f32x4*)(o + c) = o0;
      *(f32x4*)(o + c + 4) = o1;
    }
  } else {
    for (int c = lane; c < d; c += 64) o[c] = e[c] * scale + p[c];
  }
}

hipError_t launch_score_embed(const int64_t* tok, int ldt, const int32_t* lens, const void* table, int table_f16,
                              const float* pe, float scale, int pos_offset, float* x, int32_t* tgt, int nseq, int seq,
                              int rows_pad, int d, int64_t vocab, int fill, int32_t* bad, hipStream_t stream) {
  if (nseq <= 0 || seq <= 0 || rows_pad < nseq * seq || fill < 0 || fill >= vocab) return hipErrorInvalidValue;
  if (table_f16 && d % 8) return hipErrorInvalidValue;
  const dim3 grid((rows_pad + 3) / 4);
  if (table_f16)
    hipLaunchKernelGGL(score_embed_kernel<f16>, grid, dim3(256), 0, stream, tok, ldt, lens, (const f16*)table, pe, scale,
                       pos_offset, x, tgt, nseq, seq, rows_pad, d, vocab, fill, bad);
  else
    hipLaunchKernelGGL(score_embed_kernel<float>, grid, dim3(256), 0, stream, tok, ldt, lens, (const float*)table, pe,
                       scale, pos_offset, x, tgt, nseq, seq, rows_pad, d, vocab, fill, bad);
  return hipGetLastError();
}

// ------------------------------------------------------------------ out[s][j] = logit(target) - lse
// For the rows c0 <= g < c0 + rows of one logits chunk (chunk-relative row rr = g - c0): lse = m + log sum_i s_i
// e^(mx_i - m) over the 256-column tiles i (maximum mx_i, exp-sum s_i: statistics [ntiles][stat_rows], scale 1),
// m = max_i mx_i; the target's logit is the one value read from the row (fp32 [rows][ldl]).  Unscored rows (tgt < 0)
// are left alone.
// 16 rows per workgroup, 16 slices of the tiles per row: a slice's 16 rows read one 64-B run of a tile's statistics.
constexpr int SG_ROWS = 16;

__global__ __launch_bounds__(256) void score_gather_kernel(const float* __restrict__ logits, int64_t ldl,
                                                           const float* __restrict__ tile_max,
                                                           const float* __restrict__ tile_sum, int ntiles, int stat_rows,
                                                           const int32_t* __restrict__ tgt, int c0, int rows, int seq,
                                                           float* __restrict__ out, int ldo) {
  __shared__ float sm[SG_ROWS][SG_ROWS + 1], ss[SG_ROWS][SG_ROWS + 1];
  const int lr = threadIdx.x % SG_ROWS, part = threadIdx.x / SG_ROWS;
  const int rr = blockIdx.x * SG_ROWS + lr;
  float m = -INFINITY, sum = 0.f;
  if (rr < rows) {
    for (int i = part; i < ntiles; i += SG_ROWS) {
      const float tm = tile_max[(size_t)i * stat_rows + rr], ts = tile_sum[(size_t)i * stat_rows + rr];
      if (tm > m) {
        sum = sum * expf(m - tm) + ts;
        m = tm;
      } else {
        sum += ts * expf(tm - m);
      }
    }
  }
  sm[lr][part] = m;
  ss[lr][part] = sum;
  __syncthreads();
  if (part != 0 || rr >= rows) return;
  const int g = c0 + rr, target = tgt[g];
  if (target < 0) return;
  float M = -INFINITY;
#pragma unroll
  for (int q = 0; q < SG_ROWS; ++q) M = fmaxf(M, sm[lr][q]);
  float S = 0.f;
#pragma unroll
  for (int q = 0; q < SG_ROWS; ++q) S += sm[lr][q] == -INFINITY ? 0.f : ss[lr][q] * expf(sm[lr][q] - M);
  const int s = g / seq;
  out[(size_t)s * ldo + (g - s * seq)] = logits[(size_t)rr * ldl + target] - (M + logf(S));
}

hipError_t launch_score_gather(const float* logits, int64_t ldl, const float* tile_max, const float* tile_sum, int ntiles,
                               int stat_rows, const int32_t* tgt, int c0, int rows, int seq, float* out, int ldo,
                               hipStream_t stream) {
  if (rows <= 0 || stat_rows < rows || ntiles <= 0 || seq <= 0 || ldo < seq) return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_gather_kernel, dim3((rows + SG_ROWS - 1) / SG_ROWS), dim3(256), 0, stream, logits, ldl, tile_max,
                     tile_sum, ntiles, stat_rows, tgt, c0, rows, seq, out, ldo);
  return hipGetLastError();
}

}  // namespace smi
