// smi_gram: C = X^T Y over n rows of fp16, into fp64 (restated in tests/transforms_ref.py).  The second-moment
// matrix a PCA diagonalises and the cross-moment matrix an OPQ Procrustes step decomposes (sonar_amd/transforms.py), contracted
// over the rows of a corpus that is too long for one fp32 accumulator.
// Numerics contract (the whole of it; include/sonar_mi355.h repeats it):
//   * rows are cut into chunks of SMI_GRAM_CHUNK_ROWS consecutive rows, chunk c = rows [c * CHUNK, min(n, (c + 1) * CHUNK));
//   * inside a chunk every product of two fp16 values is exact in fp32 and the sums are the fp32 accumulation of
//     v_mfma_f32_16x16x32_f16 over the chunk's 32-row K steps in ascending order;
//   * a chunk's fp32 result is widened to fp64 and the chunks of a span (chunks_per_span(n) consecutive chunks, a function
//     of n alone) are added in ascending order, then the spans are added in ascending order: a fixed tree that depends on n;
//   * so the bits of out depend on (x, y, n) and the constant only: not on the CU count, the grid, the run, or the rows
//     beyond n in the allocation.  No atomics.  Inf and NaN propagate;
//   * with y == NULL only the tiles on or above the diagonal are computed and every element below the diagonal is a copy of
//     its mirror image: out is bitwise symmetric;
//   * the rows of a K step at or beyond the end of a span (so: at or beyond n) and the columns of a 128-wide tile at or beyond
//     d are zeros in the LDS image.  Nothing is read at or beyond row n.
// The kernel is head_bwd_gemm_kernel's mode 0 (head_train.hip) with fp16 fragments: both operands have the contraction index
// outermost, a K step is a [32 rows][128 columns] image per operand, fragments come through ds_read_b64_tr_b16 with every
// lane in bounds and EXEC all ones.
#include "api_common.hpp"
#include "common.hpp"

using namespace smi;
using namespace smi_host;

namespace smi {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int GR_CHUNK = SMI_GRAM_CHUNK_ROWS;
constexpr int GR_TILE = 128, GR_KT = 32, GR_ROW = 288;  // an image row: 256 B of columns + 32 B pad (conflict-free tr reads)
constexpr int GR_IMG = GR_KT * GR_ROW;                  // 9216
constexpr int GR_MAX_SPANS = 32;
static_assert(GR_CHUNK >= 1024 && GR_CHUNK <= 8192 && GR_CHUNK % GR_KT == 0, "chunk: whole K steps, in the published range");

// The split of the rows: a function of n alone (the contract's tree).
struct GramPlan {
  int chunks_per_span, n_spans, tiles_m, tiles_n, n_tiles;
  bool sym;
  size_t part_bytes() const { return (size_t)n_spans * n_tiles * GR_TILE * GR_TILE * sizeof(double); }
};
inline GramPlan gram_plan(int64_t n, int d1, int d2, bool sym) {
  GramPlan p;
  const int64_t chunks = (n + GR_CHUNK - 1) / GR_CHUNK;
  p.chunks_per_span = (int)((chunks + GR_MAX_SPANS - 1) / GR_MAX_SPANS);
  p.n_spans = (int)((chunks + p.chunks_per_span - 1) / p.chunks_per_span);
  p.tiles_m = (d1 + GR_TILE - 1) / GR_TILE;
  p.tiles_n = (d2 + GR_TILE - 1) / GR_TILE;
  p.sym = sym;
  p.n_tiles = sym ? p.tiles_m * (p.tiles_m + 1) / 2 : p.tiles_m * p.tiles_n;
  return p;
}

// tile t of the upper triangle of a T x T grid, row-major: (a, b) with b >= a, and back
__host__ __device__ __forceinline__ int gram_tri_index(int a, int b, int T) { return a * T - a * (a - 1) / 2 + (b - a); }

__device__ __forceinline__ s16x4 gr_tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// One work unit: tile blockIdx.x of C over span blockIdx.y of the rows -> part[span][tile][128][128] fp64.  Two waves per SIMD
// (224 VGPRs, the accumulators among them, no scratch): two workgroups per CU cover each other's barriers.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gram_kernel(
    const unsigned short* __restrict__ X, const unsigned short* __restrict__ Y, int n, int d1, int d2, int tiles_n, int sym,
    int span_rows, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) char lds[2 * GR_IMG];
  char* const As = lds;
  char* const Bs = lds + GR_IMG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, i = lane & 15;
  int ta, tb;
  if (sym) {
    int a = 0, rem = blockIdx.x;
    while (rem >= tiles_n - a) rem -= tiles_n - a, ++a;
    ta = a, tb = a + rem;
  } else {
    ta = blockIdx.x / tiles_n, tb = blockIdx.x % tiles_n;
  }
  const int m_base = ta * GR_TILE, n_base = tb * GR_TILE;
  const long long rs64 = (long long)blockIdx.y * span_rows;
  const int rs = (int)rs64;                                         // < n: the host launches no empty span
  const int re = (int)(rs64 + span_rows < n ? rs64 + span_rows : n);  // <= n: no row at or beyond it is addressed

  // staging: two 16-B pieces per thread and operand; rows beyond the span and columns beyond d are zeros in the image
  u32x4 ra[2], rb[2];
  auto load = [&](int kk) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int id = tid + c * 256;
      const int row = kk + (id >> 4), ch = id & 15;
      const int ca = m_base + ch * 8, cb = n_base + ch * 8;
      u32x4 za = {0u, 0u, 0u, 0u}, zb = {0u, 0u, 0u, 0u};
      if (row < re) {
        if (ca < d1) za = *(const u32x4*)(X + (size_t)row * d1 + ca);
        if (cb < d2) zb = *(const u32x4*)(Y + (size_t)row * d2 + cb);
      }
      ra[c] = za;
      rb[c] = zb;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int id = tid + c * 256;
      *(u32x4*)(As + (id >> 4) * GR_ROW + (id & 15) * 16) = ra[c];
      *(u32x4*)(Bs + (id >> 4) * GR_ROW + (id & 15) * 16) = rb[c];
    }
  };

  // fragment addresses (head_bwd_gemm_kernel): element j = 4 s + e of a fragment is k = 16 s + 4 g + e for both operands
  const int q = i >> 2, p = i & 3;
  const char* a_tr = As + (4 * g + q) * GR_ROW + (wm * 64 + 4 * p) * 2;  // + t * 32 + s * 16 * GR_ROW
  const char* b_tr = Bs + (4 * g + q) * GR_ROW + (wn * 64 + 4 * p) * 2;

  // the unit's fp64 partial, [128][128]: this thread's 64 elements of it are its own from the first chunk to the last (D column
  // on lane & 15, D row = 4 (lane >> 4) + register), so the running fp64 sums live there and not in 128 more registers
  double* const out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (GR_TILE * GR_TILE) +
                      (wm * 64 + 4 * g) * GR_TILE + wn * 64 + i;
  f32x4 acc[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

  load(rs);
  for (int kk = rs; kk < re; kk += GR_KT) {
    __syncthreads();  // the previous step's fragment reads are done
    stage();
    __syncthreads();
    if (kk + GR_KT < re) load(kk + GR_KT);  // uniform: the next step's global loads fly under the MFMAs
    half8 fa[4], fb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const s16x4 alo = gr_tr_read(a_tr + t * 32);
      const s16x4 ahi = gr_tr_read(a_tr + t * 32 + 16 * GR_ROW);
      fa[t] = __builtin_bit_cast(half8, (s16x8)__builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7));
      const s16x4 blo = gr_tr_read(b_tr + t * 32);
      const s16x4 bhi = gr_tr_read(b_tr + t * 32 + 16 * GR_ROW);
      fb[t] = __builtin_bit_cast(half8, (s16x8)__builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn)
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[tm], fb[tn], acc[tm][tn], 0, 0, 0);
    // the end of a chunk (spans begin on chunk boundaries) or of the rows: the fp32 sums go into the fp64 ones
    const int done = kk + GR_KT - rs;
    if (done % GR_CHUNK == 0 || kk + GR_KT >= re) {  // uniform
      const bool first = done <= GR_CHUNK;           // the span's first chunk writes, the later ones add: ascending order
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* const o = out + (tm * 16 + r) * GR_TILE + tn * 16;
            const double v = (double)acc[tm][tn][r];
            *o = first ? v : *o + v;
          }
          acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
          __builtin_amdgcn_sched_barrier(0);  // four fp64 values in flight at a time, not all 64 (128 registers)
        }
    }
  }
}

// out[i][j] = the spans' partials of that element added in ascending span order; with sym, an element below the diagonal
// takes the bits of its mirror image.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ part, int d1, int d2, int tiles_n, int sym,
                                                          int n_tiles, int n_spans, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)d1 * d2) return;
  int r = (int)(idx / d2), c = (int)(idx % d2);
  if (sym && r > c) {
    const int t = r;
    r = c, c = t;
  }
  const int ta = r / GR_TILE, tb = c / GR_TILE;
  const int tile = sym ? gram_tri_index(ta, tb, tiles_n) : ta * tiles_n + tb;
  const double* p = part + (size_t)tile * (GR_TILE * GR_TILE) + (r % GR_TILE) * GR_TILE + c % GR_TILE;
  double s = 0.0;
  for (int k = 0; k < n_spans; ++k) s += p[(size_t)k * n_tiles * (GR_TILE * GR_TILE)];
  out[idx] = s;
}

}  // namespace smi

namespace {

// the refusals that depend on the shape alone: a status and its text, or SMI_OK
int gram_shape_status(int64_t n, int32_t d1, int32_t d2, const char** why) {
  *why = nullptr;
  if (n < 1) return *why = "n < 1: empty input", SMI_ERR_INVALID_ARG;
  if (d1 < 64 || d2 < 64 || d1 % 64 || d2 % 64 || d1 > 8192 || d2 > 8192)
    return *why = "d1 and d2 must be multiples of 64 in [64, 8192]", SMI_ERR_UNSUPPORTED;
  if (n > 0x7fffff00LL) return *why = "n must not exceed 2^31 - 256", SMI_ERR_UNSUPPORTED;
  return SMI_OK;
}

}  // namespace

extern "C" {

int64_t smi_gram_ws_bytes(int64_t n, int32_t d1, int32_t d2) {
  const char* why;
  if (gram_shape_status(n, d1, d2, &why) != SMI_OK) return 0;
  // the cross form (y given); the symmetric form needs T (T + 1) / 2 of these T x T tile slots and smi_gram asks for no more
  return (int64_t)gram_plan(n, d1, d2, false).part_bytes();
}

int smi_gram(const void* x, const void* y, int64_t n, int32_t d1, int32_t d2, double* out, void* ws, int64_t ws_bytes,
             void* stream_v) {
  if (!x || !out) return fail(SMI_ERR_INVALID_ARG, "null x / out");
  const char* why;
  if (const int rc = gram_shape_status(n, d1, d2, &why)) return fail(rc, "smi_gram n=%lld d1=%d d2=%d: %s", (long long)n, d1, d2, why);
  const bool sym = y == nullptr;
  if (sym && d1 != d2) return fail(SMI_ERR_INVALID_ARG, "y == NULL is the symmetric form: d1 = %d, d2 = %d must be equal", d1, d2);
  const GramPlan p = gram_plan(n, d1, d2, sym);
  if (const int rc = check_ws(ws, ws_bytes, p.part_bytes(),
                              sym ? "smi_gram_ws_bytes(n, d, d) / T^2 * T (T + 1) / 2, T = ceil(d / 128)," : "smi_gram_ws_bytes(n, d1, d2)"))
    return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t stream = (hipStream_t)stream_v;
  hipLaunchKernelGGL(gram_kernel, dim3(p.n_tiles, p.n_spans), dim3(256), 0, stream, (const unsigned short*)x,
                     (const unsigned short*)(sym ? x : y), (int)n, d1, d2, p.tiles_n, sym ? 1 : 0,
                     p.chunks_per_span * GR_CHUNK, (double*)ws);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(gram_reduce_kernel, grid_for((int64_t)d1 * d2, 256), dim3(256), 0, stream, (const double*)ws, d1, d2,
                     p.tiles_n, sym ? 1 : 0, p.n_tiles, p.n_spans, out);
  HIP_TRY(hipGetLastError());
  return SMI_OK;
}

}  // extern "C"
