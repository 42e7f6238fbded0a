// Training of MLP heads over frozen SONAR embeddings: the forward pass of heads.hip on the shared GEMM engines, an fp32
// output layer with its loss, a bf16 MFMA kernel for the two backward products of every hidden layer, and AdamW.
//   recipe   examples/finetune_sonar_as_toxicity_classifier.ipynb part 4 (Linear-Tanh-Dropout-Linear, AdamW, clip 1.0)
//   heads    sonar/models/mutox/factory.py:15-38 (BCE with logits), sonar/models/blaser/model.py:63-80 (MSE)
// Storage contract: masters, moments and gradients fp32; hidden layers keep an fp16 shadow of W for
// launch_gemm_tn; activations fp16 [rows padded to 128][dim]; dz bf16; the backward products take bf16 operands with
// fp32 accumulation (fp16 operands are converted on the way into LDS).  No atomics anywhere: every reduction has one
// fixed order, so a run is reproducible bit for bit.
#include <cmath>
#include <vector>

#include "api_common.hpp"
#include "common.hpp"

using namespace smi;
using namespace smi_host;

namespace smi {

typedef unsigned long long u64;
typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------
// Dropout mask: a pure function of (seed, step, site, row, col).  mix = the finaliser of smp_hash (sampling.hip).
__host__ __device__ __forceinline__ bool ht_keep(u64 seed, u64 step_site, u64 row, u64 width, u64 col, float p) {
  const u64 key = (step_site << 40) + row * width + col;
  u64 z = seed + 0x9E3779B97F4A7C15ull * (key + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * 5.9604644775390625e-8f >= p;  // 24 bits * 2^-24: exact in fp32
}

// ---------------------------------------------------------------------------------------------------------------------
// head_bwd_gemm_kernel: 128x128 output tile, 4 waves of 64x64 (4x4 v_mfma_f32_16x16x32_bf16), contraction in steps of 32.
//   MODE 0: C[M,N] = sum_r P[r,M] Q[r,N]   (gW = dz^T A): both operands have the contraction index outermost
//   MODE 1: C[R,N] = sum_k P[R,k] Q[k,N]   (dA = dz W):   P is read by rows, Q transposed
// LDS image of a contraction-outermost operand: [32 k][128 columns] bf16, rows of 288 B (256 + 32 pad).  One
// ds_read_b64_tr_b16 gives lane (g = l>>4, i = l&15) the 4 elements k = 16s + 4g + (0..3) of column c0 + i, so element
// j = 4s + e of a fragment is k = 16s + 4g + e for BOTH operands (the MFMA only needs the two maps to agree).  The 32
// lanes of a half then read rows 16s .. 16s+7, 72 dwords apart = 8 banks apart, 32 B each: all 64 banks once.
// MODE 1's P image is [128 rows][32 k] with rows of 80 B; lane (g, i) takes k = 16s + 4g + (0..3) of row i as one
// ds_read_b64 (20 dwords between rows: the 16 rows of a group land on the 16 multiples of 4, g adds 2: conflict free).
// The N edge (N % 128 == 64) is handled by zero-filling the image, never by masking lanes of the transposed reads:
// every lane always supplies an in-bounds address and EXEC is all ones at every ds_read_b64_tr_b16.
constexpr int HB_TILE = 128, HB_KT = 32, HB_TR_ROW = 288, HB_ROW_ROW = 80;
constexpr int HB_TR_BYTES = HB_KT * HB_TR_ROW;     // 9216
constexpr int HB_ROW_BYTES = HB_TILE * HB_ROW_ROW;  // 10240

// 8 stored elements (fp16 or bf16 bits) -> 8 bf16 bits
template <bool IS_F16>
__device__ __forceinline__ u32x4 hb_to_bf16(u32x4 v) {
  if constexpr (!IS_F16) {
    return v;
  } else {
    const half8 h = __builtin_bit_cast(half8, v);
    bf16x8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (bf16)(float)h[e];  // v_cvt_pk_bf16_f32: RNE
    return __builtin_bit_cast(u32x4, b);
  }
}

__device__ __forceinline__ s16x4 hb_tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

template <int MODE, bool P16, bool Q16>
__global__ __launch_bounds__(256) void head_bwd_gemm_kernel(const void* __restrict__ Pv, const void* __restrict__ Qv,
                                                            int R, int M, int N, float* __restrict__ C) {
  __shared__ __attribute__((aligned(16))) char lds[HB_ROW_BYTES + HB_TR_BYTES];
  char* const As = lds;
  char* const Bs = lds + HB_ROW_BYTES;
  const unsigned short* P = (const unsigned short*)Pv;
  const unsigned short* Q = (const unsigned short*)Qv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, i = lane & 15;
  const int n_base = blockIdx.x * HB_TILE, m_base = blockIdx.y * HB_TILE;
  // contraction length and the leading dimensions: MODE 0 sums over the R rows of P [R][M] and Q [R][N]; MODE 1 sums over
  // the M columns of P [R][M] = rows of Q [M][N]
  const int KC = MODE == 0 ? R : M;

  // staging: two 16-B chunks per thread and operand
  u32x4 ra[2], rb[2];
  auto load = [&](int kk) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int id = tid + c * 256;
      if constexpr (MODE == 0) {
        const int row = id >> 4, ch = id & 15;  // P [R][M]: k rows, columns m_base + 8 ch (M % 128 == 0: in bounds)
        ra[c] = *(const u32x4*)(P + (size_t)(kk + row) * M + m_base + ch * 8);
      } else {
        const int row = id >> 2, ch = id & 3;   // P [R][M]: rows m_base + row, k columns kk + 8 ch
        ra[c] = *(const u32x4*)(P + (size_t)(m_base + row) * M + kk + ch * 8);
      }
      const int row = id >> 4, ch = id & 15;    // Q [KC][N]: columns beyond N are zero in the image
      const int col = n_base + ch * 8;
      u32x4 z = {0u, 0u, 0u, 0u};
      if (col < N) z = *(const u32x4*)(Q + (size_t)(kk + row) * N + col);
      rb[c] = z;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int id = tid + c * 256;
      if constexpr (MODE == 0)
        *(u32x4*)(As + (id >> 4) * HB_TR_ROW + (id & 15) * 16) = hb_to_bf16<P16>(ra[c]);
      else
        *(u32x4*)(As + (id >> 2) * HB_ROW_ROW + (id & 3) * 16) = hb_to_bf16<P16>(ra[c]);
      *(u32x4*)(Bs + (id >> 4) * HB_TR_ROW + (id & 15) * 16) = hb_to_bf16<Q16>(rb[c]);
    }
  };

  // fragment addresses of this lane (half s adds 16 k rows / 32 bytes of a P row)
  const int q = i >> 2, p = i & 3;
  const char* a_tr = As + (4 * g + q) * HB_TR_ROW + (wm * 64 + 4 * p) * 2;   // MODE 0, + t * 32 + s * 16 * HB_TR_ROW
  const char* a_row = As + (wm * 64 + i) * HB_ROW_ROW + 8 * g;              // MODE 1, + t * 16 * HB_ROW_ROW + s * 32
  const char* b_tr = Bs + (4 * g + q) * HB_TR_ROW + (wn * 64 + 4 * p) * 2;

  f32x4 acc[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

  load(0);
  for (int kk = 0; kk < KC; kk += HB_KT) {
    __syncthreads();  // the previous step's fragment reads are done
    stage();
    __syncthreads();
    if (kk + HB_KT < KC) load(kk + HB_KT);  // uniform: the next step's global loads fly under the MFMAs
    bf16x8 fa[4], fb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s16x4 lo, hi;
      if constexpr (MODE == 0) {
        lo = hb_tr_read(a_tr + t * 32);
        hi = hb_tr_read(a_tr + t * 32 + 16 * HB_TR_ROW);
      } else {
        lo = *(const s16x4*)(a_row + t * 16 * HB_ROW_ROW);
        hi = *(const s16x4*)(a_row + t * 16 * HB_ROW_ROW + 32);
      }
      fa[t] = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      const s16x4 blo = hb_tr_read(b_tr + t * 32);
      const s16x4 bhi = hb_tr_read(b_tr + t * 32 + 16 * HB_TR_ROW);
      fb[t] = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn)
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[tm], fb[tn], acc[tm][tn], 0, 0, 0);
  }

  // read-out: D column (n) on lane & 15, D row (m) = 4 (lane >> 4) + register
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int n = n_base + wn * 64 + tn * 16 + i;
      if (n < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m_base + wm * 64 + tm * 16 + 4 * g + r;
          C[(size_t)m * N + n] = acc[tm][tn][r];
        }
      }
    }
}

// dtypes: 1 fp16, 2 bf16 (smi_dtype).  MODE 0: P [R][M], Q [R][N] -> C [M][N];  MODE 1: P [R][M], Q [M][N] -> C [R][N].
hipError_t launch_head_bwd_gemm(int mode, const void* P, int p_dtype, const void* Q, int q_dtype, int R, int M, int N,
                                float* C, hipStream_t stream) {
  if ((mode != 0 && mode != 1) || !P || !Q || !C || R < 128 || M < 128 || N < 64 || R % 128 || M % 128 || N % 64)
    return hipErrorInvalidValue;
  if ((p_dtype != 1 && p_dtype != 2) || (q_dtype != 1 && q_dtype != 2)) return hipErrorInvalidValue;
  const dim3 grid((N + HB_TILE - 1) / HB_TILE, (mode == 0 ? M : R) / HB_TILE), block(256);
  const bool p16 = p_dtype == 1, q16 = q_dtype == 1;
#define HB_LAUNCH(MODE, A, B) \
  hipLaunchKernelGGL((head_bwd_gemm_kernel<MODE, A, B>), grid, block, 0, stream, P, Q, R, M, N, C)
  if (mode == 0) {
    if (p16 && q16) HB_LAUNCH(0, true, true);
    else if (p16) HB_LAUNCH(0, true, false);
    else if (q16) HB_LAUNCH(0, false, true);
    else HB_LAUNCH(0, false, false);
  } else {
    if (p16 && q16) HB_LAUNCH(1, true, true);
    else if (p16) HB_LAUNCH(1, true, false);
    else if (q16) HB_LAUNCH(1, false, true);
    else HB_LAUNCH(1, false, false);
  }
#undef HB_LAUNCH
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Batch gather: batch row r = dataset row (perm ? perm[offset + r] : offset + r), input dropout (site 0), pad rows zeroed.
template <typename T>
__global__ __launch_bounds__(256) void ht_gather_kernel(const T* __restrict__ x, const int64_t* __restrict__ perm,
                                                        int64_t offset, int rows, int rows_pad, int d, float p,
                                                        float scale, u64 seed, u64 step, f16* __restrict__ out) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows_pad) return;
  f16* o = out + (size_t)r * d;
  if (r >= rows) {
    for (int c = lane; c < d; c += 64) o[c] = (f16)0.f;
    return;
  }
  const int64_t src = perm ? perm[offset + r] : offset + r;
  const T* s = x + (size_t)src * d;
  for (int c = lane; c < d; c += 64) {
    float v = (float)s[c];
    if (p > 0.f) v = ht_keep(seed, step * 16ull, (u64)r, (u64)d, (u64)c, p) ? v * scale : 0.f;
    o[c] = (f16)v;
  }
}

// Hidden dropout (site l): a = f16(f32(h) * scale) where kept, 0 elsewhere.  Pad rows pass through (their dz is zero).
__global__ __launch_bounds__(256) void ht_dropout_kernel(const f16* __restrict__ h, f16* __restrict__ a, int rows,
                                                         int width, float p, float scale, u64 seed, u64 step_site) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * width) return;
  const u64 r = idx / width, c = idx % width;
  const float v = (float)h[idx];
  a[idx] = (f16)(ht_keep(seed, step_site, r, (u64)width, c, p) ? v * scale : 0.f);
}

// Output layer, one wave per row (the arithmetic of head_output_kernel for the logits): loss of the row, d = dL/dlogits
// already scaled by the mean's 1/count (dA = d W_out for the layer below: ht_output_dA_kernel).  loss 0 ce, 1 bce, 2 mse.
__global__ __launch_bounds__(256) void ht_output_kernel(const f16* __restrict__ a, int K, const float* __restrict__ w,
                                                        const float* __restrict__ b, int rows, int out_dim, int loss,
                                                        const void* __restrict__ targets,
                                                        const int64_t* __restrict__ perm, int64_t offset,
                                                        float inv_count, float* __restrict__ dlog,
                                                        float* __restrict__ row_loss) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const f16* x = a + (size_t)r * K;
  // logits: every output's sum runs over c = lane, lane + 64, ... in ascending order, as in head_output_kernel; the outputs
  // share one pass over the row so that its loads are issued once and eight steps at a time
  float z[8], d[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) z[o] = d[o] = 0.f;
#pragma unroll 8
  for (int c = lane; c < K; c += 64) {
    const float xv = (float)x[c];
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < out_dim) z[o] += xv * w[(size_t)o * K + c];
  }
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < out_dim) z[o] = wave_sum(z[o]) + b[o];
  const int64_t src = perm ? perm[offset + r] : offset + r;
  float L = 0.f;
  if (loss == 0) {
    int y = ((const int32_t*)targets)[src];
    y = min(max(y, 0), out_dim - 1);  // the host refuses labels out of range; never index past the row
    float mx = z[0];
#pragma unroll
    for (int o = 1; o < 8; ++o)
      if (o < out_dim) mx = fmaxf(mx, z[o]);
    float se = 0.f, zy = 0.f;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < out_dim) {
        d[o] = expf(z[o] - mx);
        se += d[o];
        if (o == y) zy = z[o];
      }
    L = logf(se) + mx - zy;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < out_dim) d[o] = (d[o] / se - (o == y ? 1.f : 0.f)) * inv_count;
  } else {
    const float* t = (const float*)targets + (size_t)src * out_dim;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < out_dim) {
        const float y = t[o];
        if (loss == 1) {
          const float e = expf(-fabsf(z[o]));
          L += fmaxf(z[o], 0.f) - z[o] * y + log1pf(e);
          const float s = z[o] >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
          d[o] = (s - y) * inv_count;
        } else {
          const float e = z[o] - y;
          L += e * e;
          d[o] = 2.f * e * inv_count;
        }
      }
  }
  if (lane == 0) {
    row_loss[r] = L;
#pragma unroll
    for (int o = 0; o < 8; ++o) dlog[(size_t)r * 8 + o] = d[o];
  }
}

// dA[r][c] = sum_o d[r][o] W_out[o][c] for the layer below, one thread per element (o ascending)
__global__ __launch_bounds__(256) void ht_output_dA_kernel(const float* __restrict__ dlog, const float* __restrict__ w,
                                                           int rows, int K, int out_dim, float* __restrict__ dA) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * K) return;
  const size_t r = idx / K, c = idx % K;
  float s = 0.f;
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < out_dim) s += dlog[r * 8 + o] * w[(size_t)o * K + c];
  dA[idx] = s;
}

// Row sums in a fixed order: a block owns 32 consecutive elements, partition q of HT_PARTS sums rows q, q + HT_PARTS, ...
// in ascending order (the loads of eight steps in flight), and the partitions are added in ascending q.
constexpr int HT_PARTS = 8;
template <typename F>
__device__ __forceinline__ float ht_row_sum(int rows, float* sh, F&& term) {
  const int q = threadIdx.x >> 5, e = threadIdx.x & 31;
  float s = 0.f;
#pragma unroll 8
  for (int r = q; r < rows; r += HT_PARTS) s += term(r);
  sh[q * 32 + e] = s;
  __syncthreads();
  float t = 0.f;
  if (q == 0) {
#pragma unroll
    for (int k = 0; k < HT_PARTS; ++k) t += sh[k * 32 + e];
  }
  return t;  // valid in partition 0
}

// gW_out[o][c] = sum_r d[r][o] a[r][c], gb_out[o] = sum_r d[r][o], loss = inv_count * sum_r row_loss[r]: element
// idx = blockIdx.x * 32 + (threadIdx.x & 31) of the list [gW (out*K), gb (out), loss (1)].
__global__ __launch_bounds__(256) void ht_output_grad_kernel(const f16* __restrict__ a, int K,
                                                             const float* __restrict__ dlog,
                                                             const float* __restrict__ row_loss, int rows, int out_dim,
                                                             float inv_count, float* __restrict__ gW,
                                                             float* __restrict__ gb, float* __restrict__ loss_out) {
  __shared__ float sh[HT_PARTS * 32];
  const int idx = blockIdx.x * 32 + (threadIdx.x & 31);
  const int nW = out_dim * K;
  const int kind = idx < nW ? 0 : (idx < nW + out_dim ? 1 : (idx == nW + out_dim ? 2 : 3));
  const int o = kind == 0 ? idx / K : (kind == 1 ? idx - nW : 0), c = kind == 0 ? idx % K : 0;
  const float s = ht_row_sum(rows, sh, [&](int r) {
    if (kind == 0) return dlog[(size_t)r * 8 + o] * (float)a[(size_t)r * K + c];
    if (kind == 1) return dlog[(size_t)r * 8 + o];
    return kind == 2 ? row_loss[r] : 0.f;
  });
  if (threadIdx.x >= 32) return;
  if (kind == 0) gW[idx] = s;
  else if (kind == 1) gb[o] = s;
  else if (kind == 2) *loss_out = s * inv_count;
}

// dz = (keep ? dA * scale : 0) * act'(h) -> bf16 (RNE); rows >= `rows` are written as zero (the pad rows of the hidden
// activations are act(bias), only a zero dz keeps them out of gW).
__global__ __launch_bounds__(256) void ht_dz_kernel(const float* __restrict__ dA, const f16* __restrict__ h, int rows,
                                                    int rows_pad, int width, int act, float p, float scale, u64 seed,
                                                    u64 step_site, bf16* __restrict__ dz) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows_pad * width) return;
  const u64 r = idx / width, c = idx % width;
  float v = 0.f;
  if (r < (u64)rows) {
    float t = dA[idx];
    if (p > 0.f) t = ht_keep(seed, step_site, r, (u64)width, c, p) ? t * scale : 0.f;
    const float hv = (float)h[idx];
    v = act == 1 ? t * (1.f - hv * hv) : (hv > 0.f ? t : 0.f);
  }
  dz[idx] = (bf16)v;
}

// gb[c] = sum_r dz[r][c] in fp32 (ht_row_sum's order), 32 columns per block
__global__ __launch_bounds__(256) void ht_colsum_kernel(const bf16* __restrict__ dz, int rows, int width,
                                                        float* __restrict__ gb) {
  __shared__ float sh[HT_PARTS * 32];
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);  // width % 128 == 0: always a column
  const float s = ht_row_sum(rows, sh, [&](int r) { return (float)dz[(size_t)r * width + c]; });
  if (threadIdx.x < 32) gb[c] = s;
}

// Gradient norm, two stages in a fixed order.  Stage 1: block b sums the squares of elements [b*4096, (b+1)*4096).
constexpr int HT_NORM_CHUNK = 4096;
__device__ __forceinline__ float ht_block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return s;
}
__global__ __launch_bounds__(256) void ht_sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                       float* __restrict__ partial) {
  __shared__ float sh[4];
  const int64_t base = (int64_t)blockIdx.x * HT_NORM_CHUNK;
  float s = 0.f;
  for (int k = 0; k < HT_NORM_CHUNK / 256; ++k) {
    const int64_t idx = base + k * 256 + threadIdx.x;
    const float v = idx < n ? g[idx] : 0.f;
    s += v * v;
  }
  s = ht_block_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// Stage 2 (one block): scal[0] = ||g||, scal[1] = clip scale = min(1, c / (||g|| + 1e-6)) (1 when clipping is off)
__global__ __launch_bounds__(256) void ht_norm_final_kernel(const float* __restrict__ partial, int nparts,
                                                            float max_norm, float* __restrict__ scal) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int k = threadIdx.x; k < nparts; k += 256) s += partial[k];
  s = ht_block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float nrm = sqrtf(s);
    scal[0] = nrm;
    scal[1] = max_norm > 0.f ? fminf(1.f, max_norm / (nrm + 1e-6f)) : 1.f;
  }
}

// AdamW with decoupled decay (torch.optim.AdamW, one parameter group) over the flat parameter vector; refreshes the
// fp16 shadow (RNE) of the first n_shadow elements (the trainer: everything below the fp32 output layer).
__global__ __launch_bounds__(256) void ht_adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       f16* __restrict__ shadow, int64_t n, int64_t n_shadow, float lr,
                                                       float wd, float b1, float b2, float eps, float bc1,
                                                       float rsqrt_bc2,
                                                       const float* __restrict__ scal) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const float gs = g[idx] * scal[1];
  float pv = p[idx] * (1.f - lr * wd);
  const float mv = b1 * m[idx] + (1.f - b1) * gs;
  const float vv = b2 * v[idx] + (1.f - b2) * gs * gs;
  const float denom = sqrtf(vv) * rsqrt_bc2 + eps;
  pv -= (lr / bc1) * (mv / denom);
  p[idx] = pv;
  m[idx] = mv;
  v[idx] = vv;
  if (idx < n_shadow) shadow[idx] = (f16)pv;
}

__global__ __launch_bounds__(256) void ht_shadow_kernel(const float* __restrict__ p, f16* __restrict__ shadow,
                                                        int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < n) shadow[idx] = (f16)p[idx];
}

}  // namespace smi

// ---------------------------------------------------------------------------------------------------------------------
struct smi_head_trainer {
  smi_head_trainer_config cfg;
  std::vector<int> dims;             // d_in, hidden..., out
  int nl = 0;                        // Linear layers (hidden + output)
  std::vector<int64_t> offW, offB;   // element offsets into the flat vectors, layer order W0 b0 W1 b1 ...
  int64_t n_params = 0;
  DevBuf P, G, M, V, shadow;         // flat fp32 masters / gradients / moments, fp16 shadow (same indexing)
  std::vector<DevBuf> h, a;          // per hidden layer: activation output, and its dropped copy when p_hidden > 0
  DevBuf x;                          // the gathered batch, fp16 [cap][d_in]
  DevBuf dA, dz, dlog, row_loss, partial, scal, losses;
  int cap = 0;                       // batch capacity, padded to 128
  int64_t loss_cap = 0, step = 0;    // steps taken = losses written
};

namespace {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// forward (training or inference), loss and backward of one batch into T->G; loss to *loss_dev.  `step1` is the 1-based
// step of the dropout masks.
int ht_forward_backward(smi_head_trainer* T, const void* x, int x_dtype, const void* targets, const int64_t* perm,
                        int64_t offset, int rows, int64_t step1, float* loss_dev, hipStream_t stream) {
  const auto& c = T->cfg;
  const int rows_pad = (rows + 127) / 128 * 128, nl = T->nl, nh = nl - 1;
  const float s_in = 1.0f / (1.0f - c.p_in), s_hid = 1.0f / (1.0f - c.p_hidden);
  const dim3 rgrid((rows_pad + 3) / 4), blk(256);
  f16* xb = T->x.as<f16>();
  if (x_dtype == SMI_F32)
    hipLaunchKernelGGL(ht_gather_kernel<float>, rgrid, blk, 0, stream, (const float*)x, perm, offset, rows, rows_pad,
                       T->dims[0], c.p_in, s_in, (u64)c.seed, (u64)step1, xb);
  else
    hipLaunchKernelGGL(ht_gather_kernel<f16>, rgrid, blk, 0, stream, (const f16*)x, perm, offset, rows, rows_pad,
                       T->dims[0], c.p_in, s_in, (u64)c.seed, (u64)step1, xb);
  HIP_TRY(hipGetLastError());
  float* Pm = T->P.as<float>();
  float* Gm = T->G.as<float>();
  const f16* Sh = T->shadow.as<f16>();
  const int epi = c.hidden_act == 0 ? EPI_RELU_F16 : EPI_TANH_F16;
  const f16* cur = xb;
  for (int l = 0; l < nh; ++l) {
    const int in = T->dims[l], od = T->dims[l + 1];
    HIP_TRY(launch_gemm_tn(epi, cur, Sh + T->offW[l], Pm + T->offB[l], T->h[l].p, rows_pad, od, in, od, stream));
    cur = T->h[l].as<f16>();
    if (c.p_hidden > 0.f) {
      hipLaunchKernelGGL(ht_dropout_kernel, dim3(blocks_for((int64_t)rows_pad * od)), blk, 0, stream, cur,
                         T->a[l].as<f16>(), rows_pad, od, c.p_hidden, s_hid, (u64)c.seed,
                         (u64)step1 * 16ull + (u64)(l + 1));
      HIP_TRY(hipGetLastError());
      cur = T->a[l].as<f16>();
    }
  }
  const int K = T->dims[nh], out = T->dims[nl];
  const float inv_count = 1.0f / (c.loss == 0 ? (float)rows : (float)rows * (float)out);
  float* dA = T->dA.as<float>();
  hipLaunchKernelGGL(ht_output_kernel, dim3((rows + 3) / 4), blk, 0, stream, cur, K, Pm + T->offW[nh], Pm + T->offB[nh],
                     rows, out, c.loss, targets, perm, offset, inv_count, T->dlog.as<float>(),
                     T->row_loss.as<float>());
  HIP_TRY(hipGetLastError());
  if (nh > 0) {
    hipLaunchKernelGGL(ht_output_dA_kernel, dim3(blocks_for((int64_t)rows * K)), blk, 0, stream, T->dlog.as<float>(),
                       Pm + T->offW[nh], rows, K, out, dA);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(ht_output_grad_kernel, dim3((unsigned)(((int64_t)out * K + out + 32) / 32)), blk, 0, stream, cur, K,
                     T->dlog.as<float>(), T->row_loss.as<float>(), rows, out, inv_count, Gm + T->offW[nh],
                     Gm + T->offB[nh], loss_dev);
  HIP_TRY(hipGetLastError());
  bf16* dz = T->dz.as<bf16>();
  for (int l = nh - 1; l >= 0; --l) {
    const int in = T->dims[l], od = T->dims[l + 1];
    hipLaunchKernelGGL(ht_dz_kernel, dim3(blocks_for((int64_t)rows_pad * od)), blk, 0, stream, dA, T->h[l].as<f16>(),
                       rows, rows_pad, od, c.hidden_act, c.p_hidden, s_hid, (u64)c.seed,
                       (u64)step1 * 16ull + (u64)(l + 1), dz);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ht_colsum_kernel, dim3(od / 32), blk, 0, stream, dz, rows, od, Gm + T->offB[l]);
    HIP_TRY(hipGetLastError());
    const f16* below = l == 0 ? xb : (c.p_hidden > 0.f ? T->a[l - 1].as<f16>() : T->h[l - 1].as<f16>());
    HIP_TRY(launch_head_bwd_gemm(0, dz, SMI_BF16, below, SMI_F16, rows_pad, od, in, Gm + T->offW[l], stream));
    if (l > 0) HIP_TRY(launch_head_bwd_gemm(1, dz, SMI_BF16, Sh + T->offW[l], SMI_F16, rows_pad, od, in, dA, stream));
  }
  return SMI_OK;
}

int ht_norm_and_update(float* P, const float* G, float* M, float* V, f16* shadow, int64_t n, int64_t n_shadow,
                       float* partial,
                       float* scal, int64_t step1, float lr, float wd, float b1, float b2, float eps,
                       float max_grad_norm, hipStream_t stream) {
  const int nparts = (int)((n + HT_NORM_CHUNK - 1) / HT_NORM_CHUNK);
  hipLaunchKernelGGL(ht_sumsq_kernel, dim3(nparts), dim3(256), 0, stream, G, n, partial);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ht_norm_final_kernel, dim3(1), dim3(256), 0, stream, partial, nparts, max_grad_norm, scal);
  HIP_TRY(hipGetLastError());
  const double bc1 = 1.0 - std::pow((double)b1, (double)step1), bc2 = 1.0 - std::pow((double)b2, (double)step1);
  hipLaunchKernelGGL(ht_adamw_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, P, G, M, V, shadow, n, n_shadow, lr, wd,
                     b1, b2, eps, (float)bc1, (float)(1.0 / std::sqrt(bc2)), scal);
  HIP_TRY(hipGetLastError());
  return SMI_OK;
}

int ht_check_batch(smi_head_trainer* T, const void* x, int x_dtype, const void* targets, int rows) {
  if (!T) return fail(SMI_ERR_INVALID_ARG, "null trainer handle");
  if (!x || !targets) return fail(SMI_ERR_INVALID_ARG, "null x / targets");
  if (x_dtype != SMI_F32 && x_dtype != SMI_F16) return fail(SMI_ERR_INVALID_ARG, "x dtype %d (fp32 or fp16)", x_dtype);
  if (rows < 1) return fail(SMI_ERR_INVALID_ARG, "rows %d < 1", rows);
  if (rows > T->cfg.max_batch)
    return fail(SMI_ERR_INVALID_ARG, "rows %d above the trainer's batch capacity %d", rows, T->cfg.max_batch);
  return SMI_OK;
}

int ht_grow_losses(smi_head_trainer* T, int64_t cap) {
  if (cap <= T->loss_cap) return SMI_OK;
  DevBuf bigger;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(bigger.alloc((size_t)cap * 4));
  HIP_TRY(hipMemcpy(bigger.p, T->losses.p, (size_t)T->step * 4, hipMemcpyDeviceToDevice));
  T->losses = std::move(bigger);
  T->loss_cap = cap;
  return SMI_OK;
}

// ce labels of the batch, read back and checked before anything is launched (only the synchronous callers do this)
int ht_check_labels(smi_head_trainer* T, const void* targets, const int64_t* perm, int64_t offset, int rows,
                    hipStream_t stream) {
  if (T->cfg.loss != 0) return SMI_OK;
  HIP_TRY(hipStreamSynchronize(stream));
  std::vector<int64_t> idx(rows);
  if (perm)
    HIP_TRY(hipMemcpy(idx.data(), perm + offset, sizeof(int64_t) * rows, hipMemcpyDeviceToHost));
  else
    for (int r = 0; r < rows; ++r) idx[r] = offset + r;
  int64_t lo = idx[0], hi = idx[0];
  for (int64_t v : idx) lo = std::min(lo, v), hi = std::max(hi, v);
  if (lo < 0) return fail(SMI_ERR_INVALID_ARG, "negative row index %lld", (long long)lo);
  std::vector<int32_t> lab(hi - lo + 1);
  HIP_TRY(hipMemcpy(lab.data(), (const int32_t*)targets + lo, sizeof(int32_t) * lab.size(), hipMemcpyDeviceToHost));
  const int out = T->dims[T->nl];
  for (int r = 0; r < rows; ++r) {
    const int32_t y = lab[idx[r] - lo];
    if (y < 0 || y >= out) return fail(SMI_ERR_INVALID_ARG, "label %d of batch row %d is outside 0..%d", y, r, out - 1);
  }
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_head_trainer_create(const smi_head_trainer_config* cfg, const smi_mlp_head_layer* layers,
                            smi_head_trainer** out) {
  if (!cfg || !layers || !out) return fail(SMI_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (cfg->n_layers < 1 || cfg->n_layers > 8 || cfg->input_dim <= 0)
    return fail(SMI_ERR_INVALID_ARG, "n_layers %d / input_dim %d", cfg->n_layers, cfg->input_dim);
  if (cfg->hidden_act < 0 || cfg->hidden_act > 1) return fail(SMI_ERR_INVALID_ARG, "bad activation code");
  if (cfg->loss < 0 || cfg->loss > 2) return fail(SMI_ERR_INVALID_ARG, "loss %d (0 ce, 1 bce, 2 mse)", cfg->loss);
  if (!(cfg->p_in >= 0.f && cfg->p_in < 1.f) || !(cfg->p_hidden >= 0.f && cfg->p_hidden < 1.f))
    return fail(SMI_ERR_INVALID_ARG, "dropout p_in %g / p_hidden %g must be in [0, 1)", cfg->p_in, cfg->p_hidden);
  if (cfg->max_batch < 1) return fail(SMI_ERR_INVALID_ARG, "max_batch %d < 1", cfg->max_batch);
  if (!(cfg->beta1 >= 0.f && cfg->beta1 < 1.f) || !(cfg->beta2 >= 0.f && cfg->beta2 < 1.f) || !(cfg->eps > 0.f) ||
      !(cfg->weight_decay >= 0.f))
    return fail(SMI_ERR_INVALID_ARG, "bad AdamW constants");
  if (cfg->input_dim % 64) return fail(SMI_ERR_UNSUPPORTED, "input_dim %d needs %% 64 == 0", cfg->input_dim);
  const int nl = cfg->n_layers;
  for (int l = 0; l < nl; ++l) {
    const int od = layers[l].out_dim;
    const bool last = l == nl - 1;
    if (od <= 0 || (last && od > 8))
      return fail(SMI_ERR_UNSUPPORTED, "layer %d: out_dim %d (the output layer supports 1..8)", l, od);
    if (!last && od % 128) return fail(SMI_ERR_UNSUPPORTED, "hidden layer %d: width %d needs %% 128 == 0", l, od);
  }
  if (cfg->loss == 0 && layers[nl - 1].out_dim < 2)
    return fail(SMI_ERR_INVALID_ARG, "cross-entropy needs at least 2 classes");
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  smi_head_trainer* T = new smi_head_trainer();
  T->cfg = *cfg;
  T->nl = nl;
  T->dims.push_back(cfg->input_dim);
  for (int l = 0; l < nl; ++l) T->dims.push_back(layers[l].out_dim);
  int64_t off = 0;
  int max_w = 0;
  for (int l = 0; l < nl; ++l) {
    T->offW.push_back(off);
    off += (int64_t)T->dims[l] * T->dims[l + 1];
    T->offB.push_back(off);
    off += T->dims[l + 1];
    if (l + 1 < nl) max_w = std::max(max_w, T->dims[l + 1]);
  }
  T->n_params = off;
  T->cap = (cfg->max_batch + 127) / 128 * 128;
  auto build = [&]() -> int {
    const size_t n = (size_t)off;
    HIP_TRY(T->P.alloc(n * 4));
    HIP_TRY(T->G.alloc(n * 4));
    HIP_TRY(T->M.alloc(n * 4));
    HIP_TRY(T->V.alloc(n * 4));
    HIP_TRY(T->shadow.alloc(n * 2));
    HIP_TRY(hipMemset(T->G.p, 0, n * 4));
    HIP_TRY(hipMemset(T->M.p, 0, n * 4));
    HIP_TRY(hipMemset(T->V.p, 0, n * 4));
    for (int l = 0; l < nl; ++l) {
      DevBuf w, b;
      const int64_t nw = (int64_t)T->dims[l] * T->dims[l + 1];
      int rc = upload(layers[l].w, nw, false, w, "trainer weight");
      if (rc == SMI_OK) rc = upload(layers[l].b, T->dims[l + 1], false, b, "trainer bias");
      if (rc != SMI_OK) return rc;
      HIP_TRY(hipMemcpy(T->P.as<float>() + T->offW[l], w.p, nw * 4, hipMemcpyDeviceToDevice));
      HIP_TRY(hipMemcpy(T->P.as<float>() + T->offB[l], b.p, (size_t)T->dims[l + 1] * 4, hipMemcpyDeviceToDevice));
    }
    hipLaunchKernelGGL(ht_shadow_kernel, dim3(blocks_for(off)), dim3(256), 0, nullptr, T->P.as<float>(),
                       T->shadow.as<f16>(), off);
    HIP_TRY(hipGetLastError());
    T->h.resize(nl - 1);
    T->a.resize(nl - 1);
    for (int l = 0; l + 1 < nl; ++l) {
      HIP_TRY(T->h[l].alloc((size_t)T->cap * T->dims[l + 1] * 2));
      if (cfg->p_hidden > 0.f) HIP_TRY(T->a[l].alloc((size_t)T->cap * T->dims[l + 1] * 2));
    }
    HIP_TRY(T->x.alloc((size_t)T->cap * T->dims[0] * 2));
    if (max_w) {
      HIP_TRY(T->dA.alloc((size_t)T->cap * max_w * 4));
      HIP_TRY(T->dz.alloc((size_t)T->cap * max_w * 2));
    }
    HIP_TRY(T->dlog.alloc((size_t)T->cap * 8 * 4));
    HIP_TRY(T->row_loss.alloc((size_t)T->cap * 4));
    HIP_TRY(T->partial.alloc((size_t)((off + HT_NORM_CHUNK - 1) / HT_NORM_CHUNK) * 4));
    HIP_TRY(T->scal.alloc(4 * 4));
    T->loss_cap = 4096;
    HIP_TRY(T->losses.alloc((size_t)T->loss_cap * 4));
    HIP_TRY(hipDeviceSynchronize());
    return SMI_OK;
  };
  const int rc = build();
  if (rc != SMI_OK) {
    delete T;
    return rc;
  }
  *out = T;
  return SMI_OK;
}

void smi_head_trainer_destroy(smi_head_trainer* t) {
  if (!t) return;
  (void)hipDeviceSynchronize();
  delete t;
}

int smi_head_trainer_step(smi_head_trainer* T, const void* x, int32_t x_dtype, const void* targets,
                          const int64_t* perm, int64_t offset, int32_t rows, float lr, float max_grad_norm,
                          float* loss_out, void* stream_v) {
  int rc = ht_check_batch(T, x, x_dtype, targets, rows);
  if (rc != SMI_OK) return rc;
  if (offset < 0) return fail(SMI_ERR_INVALID_ARG, "negative offset");
  if (!(lr >= 0.f)) return fail(SMI_ERR_INVALID_ARG, "lr %g", lr);
  hipStream_t stream = (hipStream_t)stream_v;
  if (loss_out && (rc = ht_check_labels(T, targets, perm, offset, rows, stream)) != SMI_OK) return rc;
  // a step past the reserved loss record grows it and waits for the device: smi_head_trainer_reserve sizes it up front
  if (T->step >= T->loss_cap && (rc = ht_grow_losses(T, T->loss_cap * 2)) != SMI_OK) return rc;
  const int64_t step1 = T->step + 1;
  float* loss_dev = T->losses.as<float>() + T->step;
  rc = ht_forward_backward(T, x, x_dtype, targets, perm, offset, rows, step1, loss_dev, stream);
  if (rc != SMI_OK) return rc;
  const auto& c = T->cfg;
  rc = ht_norm_and_update(T->P.as<float>(), T->G.as<float>(), T->M.as<float>(), T->V.as<float>(), T->shadow.as<f16>(),
                          T->n_params, T->offW[T->nl - 1], T->partial.as<float>(), T->scal.as<float>(), step1, lr, c.weight_decay, c.beta1,
                          c.beta2, c.eps, max_grad_norm, stream);
  if (rc != SMI_OK) return rc;
  T->step = step1;
  if (loss_out) {
    HIP_TRY(hipMemcpyAsync(loss_out, loss_dev, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  return SMI_OK;
}

int smi_head_trainer_gradients(smi_head_trainer* T, const void* x, int32_t x_dtype, const void* targets,
                               const int64_t* perm, int64_t offset, int32_t rows, float* loss_out, float* grads_out,
                               void* stream_v) {
  int rc = ht_check_batch(T, x, x_dtype, targets, rows);
  if (rc != SMI_OK) return rc;
  if (!grads_out) return fail(SMI_ERR_INVALID_ARG, "null grads_out");
  if (offset < 0) return fail(SMI_ERR_INVALID_ARG, "negative offset");
  hipStream_t stream = (hipStream_t)stream_v;
  if ((rc = ht_check_labels(T, targets, perm, offset, rows, stream)) != SMI_OK) return rc;
  float* loss_dev = T->scal.as<float>() + 2;  // not a step: its loss stays out of the record
  rc = ht_forward_backward(T, x, x_dtype, targets, perm, offset, rows, T->step + 1, loss_dev, stream);
  if (rc != SMI_OK) return rc;
  HIP_TRY(hipMemcpyAsync(grads_out, T->G.p, (size_t)T->n_params * 4, hipMemcpyDeviceToHost, stream));
  if (loss_out) HIP_TRY(hipMemcpyAsync(loss_out, loss_dev, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return SMI_OK;
}

int smi_head_trainer_reserve(smi_head_trainer* T, int64_t more_steps) {
  if (!T) return fail(SMI_ERR_INVALID_ARG, "null trainer handle");
  if (more_steps < 0 || more_steps > (int64_t)1 << 32) return fail(SMI_ERR_INVALID_ARG, "more_steps %lld", (long long)more_steps);
  return ht_grow_losses(T, T->step + more_steps);
}

int smi_head_trainer_losses(smi_head_trainer* T, int64_t first, int64_t count, float* out) {
  if (!T) return fail(SMI_ERR_INVALID_ARG, "null trainer handle");
  if (first < 0 || count < 0 || first + count > T->step)
    return fail(SMI_ERR_INVALID_ARG, "steps %lld..%lld of %lld taken", (long long)first, (long long)(first + count),
                (long long)T->step);
  if (count == 0) return SMI_OK;
  if (!out) return fail(SMI_ERR_INVALID_ARG, "null out");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, T->losses.as<float>() + first, (size_t)count * 4, hipMemcpyDeviceToHost));
  return SMI_OK;
}

int smi_head_trainer_export(smi_head_trainer* T, int32_t layer, float* w_out, float* b_out) {
  if (!T) return fail(SMI_ERR_INVALID_ARG, "null trainer handle");
  if (layer < 0 || layer >= T->nl) return fail(SMI_ERR_INVALID_ARG, "layer %d of %d", layer, T->nl);
  if (!w_out || !b_out) return fail(SMI_ERR_INVALID_ARG, "null output");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(w_out, T->P.as<float>() + T->offW[layer], (size_t)T->dims[layer] * T->dims[layer + 1] * 4,
                    hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b_out, T->P.as<float>() + T->offB[layer], (size_t)T->dims[layer + 1] * 4, hipMemcpyDeviceToHost));
  return SMI_OK;
}

// Inference on the current weights: the calls of smi_mlp_head_forward on the shadow / master buffers, no dropout.
int smi_head_trainer_forward(smi_head_trainer* T, const void* x_f16, int32_t rows, int32_t out_act, float* out,
                             void* stream_v) {
  if (!T) return fail(SMI_ERR_INVALID_ARG, "null trainer handle");
  if (!x_f16 || !out || rows <= 0) return fail(SMI_ERR_INVALID_ARG, "bad argument");
  if (out_act < 0 || out_act > 2) return fail(SMI_ERR_INVALID_ARG, "bad out_act %d", out_act);
  if (rows > T->cfg.max_batch)
    return fail(SMI_ERR_INVALID_ARG, "rows %d above the trainer's batch capacity %d", rows, T->cfg.max_batch);
  hipStream_t stream = (hipStream_t)stream_v;
  const int rows_pad = (rows + 127) / 128 * 128, nh = T->nl - 1;
  const int epi = T->cfg.hidden_act == 0 ? EPI_RELU_F16 : EPI_TANH_F16;
  const f16* cur = (const f16*)x_f16;
  for (int l = 0; l < nh; ++l) {
    HIP_TRY(launch_gemm_tn(epi, cur, T->shadow.as<f16>() + T->offW[l], T->P.as<float>() + T->offB[l], T->h[l].p,
                           rows_pad, T->dims[l + 1], T->dims[l], T->dims[l + 1], stream));
    cur = T->h[l].as<f16>();
  }
  HIP_TRY(launch_head_output(cur, T->dims[nh], T->P.as<float>() + T->offW[nh], T->P.as<float>() + T->offB[nh], rows,
                             T->dims[nh], T->dims[nh + 1], out_act, out, stream));
  return SMI_OK;
}

int smi_head_bwd_gemm(int32_t mode, const void* P, int32_t p_dtype, const void* Q, int32_t q_dtype, int32_t R,
                      int32_t M, int32_t N, float* out_f32, void* stream) {
  if (!P || !Q || !out_f32) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (mode != 0 && mode != 1) return fail(SMI_ERR_INVALID_ARG, "mode %d (0: P^T Q, 1: P Q)", mode);
  if ((p_dtype != SMI_F16 && p_dtype != SMI_BF16) || (q_dtype != SMI_F16 && q_dtype != SMI_BF16))
    return fail(SMI_ERR_INVALID_ARG, "operands are fp16 or bf16");
  if (R < 128 || M < 128 || N < 64 || R % 128 || M % 128 || N % 64)
    return fail(SMI_ERR_UNSUPPORTED, "R %d and M %d need %% 128 == 0, N %d needs %% 64 == 0", R, M, N);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(launch_head_bwd_gemm(mode, P, p_dtype, Q, q_dtype, R, M, N, out_f32, (hipStream_t)stream));
  return SMI_OK;
}

int smi_head_adamw(float* p, const float* g, float* m, float* v, void* shadow_f16, int64_t n, int64_t step, float lr,
                   float beta1, float beta2, float eps, float weight_decay, float max_grad_norm, float* norm_scale_out,
                   void* stream_v) {
  if (!p || !g || !m || !v || !shadow_f16) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (n < 1 || step < 1) return fail(SMI_ERR_INVALID_ARG, "n %lld / step %lld", (long long)n, (long long)step);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t stream = (hipStream_t)stream_v;
  DevBuf partial, scal;
  HIP_TRY(partial.alloc((size_t)((n + HT_NORM_CHUNK - 1) / HT_NORM_CHUNK) * 4));
  HIP_TRY(scal.alloc(16));
  const int rc = ht_norm_and_update(p, g, m, v, (f16*)shadow_f16, n, n, partial.as<float>(), scal.as<float>(), step, lr,
                                    weight_decay, beta1, beta2, eps, max_grad_norm, stream);
  if (rc != SMI_OK) return rc;
  HIP_TRY(hipStreamSynchronize(stream));
  if (norm_scale_out) HIP_TRY(hipMemcpy(norm_scale_out, scal.p, 8, hipMemcpyDeviceToHost));
  return SMI_OK;
}

}  // extern "C"
