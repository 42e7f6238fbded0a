// Squared-Euclidean and inner-product search on rows as they are.  With b[j] = -1/2 ||y_j||^2,
//   argmax_j (x . y_j + b[j]) = argmin_j ||x - y_j||^2,
// so one per-row additive term on the y side turns the brute-force top-k of xsim.hip into an L2 search; the zero bias is
// maximum inner product, which needs no kernel of its own (smi_xsim_topk never needed unit rows).  Two things live here:
//  * smi_l2_prepare: the fp16 copy smi_xsim_normalize makes, without the division, and the half norms 1/2 ||row||^2 of the
//    ROUNDED rows, summed in fp64 in one fixed order (l2_half_norm, stated in the header);
//  * smi_l2_topk: the walk of xsim_walk.hpp over the policy XsF16Bias -- XsI8's mechanism (xsim_i8.hip: one fp32 per y row
//    rides the DMA stream into a slot of LDS, the fold takes a lane's 16 with four 16-byte LDS reads) with XsF16's element
//    types and MFMA.  The host side (xsim_run, the chunk merge, xs_with_k) is called as it is.
//
// Order and signed zero.  A score is fl32(acc + b).  acc starts from C = +0, so it is +0 or non-zero, never -0; +0 + (-0) = +0
// and a sum that cancels exactly is +0 under round-to-nearest: a zero score is +0 whatever the sign of a zero bias, and the
// keys of the LDS lists (which order by the score's bits) agree with the fp32 compare of the chunk merge.
#include "api_common.hpp"
#include "kernels.hpp"
#include "l2_rows.hpp"
#include "xsim_walk.hpp"

using namespace smi;
using namespace smi_host;

namespace smi {
namespace {

// ---------------------------------------------------------------- prepared rows and half norms (l2_half_norm: l2_rows.hpp)
// One wave per row, 16 bytes per lane per access (two loads make one store from an fp32 source).  Rows from `rows` on are
// zeroed, their half norms too.
template <typename T>
__global__ __launch_bounds__(256) void l2_prepare_kernel(const T* __restrict__ src, f16* __restrict__ dst,
                                                         float* __restrict__ half_norms, int64_t rows, int64_t rows_pad, int d) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows_pad) return;  // wave-uniform
  half8* o = (half8*)(dst + r * d);
  if (r >= rows) {
    for (int c = lane; c < d / 8; c += 64) o[c] = half8{0, 0, 0, 0, 0, 0, 0, 0};
    if (half_norms && lane == 0) half_norms[r] = 0.f;
    return;
  }
  const T* s = src + r * d;
  const float h = l2_half_norm(d, lane, [&](int c) {
    half8 v;
    if constexpr (sizeof(T) == 2) {
      v = *(const half8*)(s + c * 8);
    } else {
      const f32x4 a = *(const f32x4*)(s + c * 8), b = *(const f32x4*)(s + c * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = (f16)a[e];  // round to nearest even
        v[4 + e] = (f16)b[e];
      }
    }
    o[c] = v;
    return v;
  });
  if (half_norms && lane == 0) half_norms[r] = h;
}

// ---------------------------------------------------------------- top-k with a per-row bias
// The biased fp16 policy of the walk (xsim_walk.hpp).  yb: one fp32 per y row, row order, [ny_pad].
// The biases of a tile ride the DMA stream exactly as XsI8's y scales do (issue_tile, first in the group of the tile's first
// slice: the walk's counted waits hold as they are): waves 0 .. 3 copy its 256 biases (4 B per lane) into slot (tile & 7) of
// the 8 KiB above the lists.  8 slots suffice as there: nt = d / 32 >= 2 slices per tile here, so the stream is at most two
// tiles ahead of the deferred fold.  Every K keeps its lists in LDS (K = 1 too: one path).
template <int K>
struct XsF16Bias {
  typedef f16 elem_t;
  typedef half8 frag_t;
  typedef f32x4 acc_t;
  static constexpr int BK = G2_BK;
  static constexpr bool LISTS = true;
  static constexpr int BIAS = 256 * K * 8;  // above the ring, behind the lists: [8 slots][256] fp32
  static constexpr int LDS_ABOVE = BIAS + 8 * 1024;
  static constexpr bool TRACED = false;
  static __device__ __forceinline__ acc_t mfma(frag_t w, frag_t x, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, x, c, 0, 0, 0);
  }

  struct tile_t {
    f32x4 b[4];  // b[ni][r]: the biases of the lane's y columns in the tile being folded
  };
  const float* yb;
  const float* ybg;
  unsigned b_addr;
  int it, t_begin;
  __device__ __forceinline__ explicit XsF16Bias(const float* yb_) : yb(yb_) {}

  __device__ __forceinline__ void init(const XsLane& L, char* above, int, int t_begin_) {
    b_addr = (unsigned)(size_t)(above + BIAS) + L.col(0, 0) * 4;
    ybg = yb + (size_t)t_begin_ * G2_BN + (L.wave & 3) * 64 + L.lane;
    it = 0;
    t_begin = t_begin_;
  }
  __device__ __forceinline__ void issue_tile(char* above, int wave) {
    if (wave < 4)
      __builtin_amdgcn_global_load_lds(SMI_GLOBAL_PTR(ybg), SMI_LDS_PTR(above + BIAS + (it & 7) * 1024 + wave * 256), 4, 0, 0);
    ybg += G2_BN;
    ++it;
  }
  __device__ __forceinline__ void fold_begin(int n0f, tile_t& ts) { xs_read_cols16(b_addr + ((n0f / G2_BN - t_begin) & 7) * 1024, ts.b); }
  __device__ __forceinline__ float row_max(const acc_t (&acc)[4][8], int mi, const tile_t& ts) const {
    float vmax = -INFINITY;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) vmax = fmaxf(vmax, acc[ni][mi][r] + ts.b[ni][r]);
    return vmax;
  }
  __device__ __forceinline__ float score(const acc_t (&acc)[4][8], int ni, int mi, int r, const tile_t& ts) const {
    // (an opaque copy of the sum, as in XsI8::score: or hipcc keeps the 128 sums of row_max alive for the insertion path and spills)
    float a = acc[ni][mi][r];
    asm volatile("" : "+v"(a));
    return a + ts.b[ni][r];
  }
};

template <int K>
__global__ __launch_bounds__(G2_THREADS) void l2_tile256_kernel(const f16* __restrict__ Xt, const f16* __restrict__ Yt,
                                                                const float* __restrict__ yb, int d, int ntx, int nty,
                                                                int nchunks, int tiles_per_chunk, int ny, int nx_pad,
                                                                float* __restrict__ ps, int* __restrict__ pi) {
  XsF16Bias<K> p(yb);
  xsim_walk<K>(p, Xt, Yt, d, ntx, nty, nchunks, tiles_per_chunk, ny, nx_pad, ps, pi);
}

// out[s] = -h[ids[s]], 0 where ids[s] < 0; ids null: out[s] = -h[s].  The bias of a list slot from the half norm of the row it
// holds (smi_l2_slot_bias), and the bias of the centroids from their half norms (the k-means assignment).
__global__ __launch_bounds__(256) void l2_neg_gather_kernel(const int32_t* __restrict__ ids, int64_t n, const float* __restrict__ h,
                                                            float* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const int64_t id = ids ? ids[s] : s;
  out[s] = id < 0 ? 0.f : -h[id];
}

// the workspace is XsimWs over rows of d fp16 with one chunk per G2_BN = 256 rows of y: what the walk fills
constexpr int L2_CHUNK_ROWS = G2_BN;

}  // namespace

hipError_t launch_l2_prepare(const void* src, int src_is_f32, f16* dst, float* half_norms, int64_t rows, int d, hipStream_t stream) {
  const int64_t rows_pad = smi_xsim_padded_rows(rows);
  const dim3 grid = grid_for(rows_pad, 4);
  if (src_is_f32)
    hipLaunchKernelGGL(l2_prepare_kernel<float>, grid, dim3(256), 0, stream, (const float*)src, dst, half_norms, rows, rows_pad, d);
  else
    hipLaunchKernelGGL(l2_prepare_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)src, dst, half_norms, rows, rows_pad, d);
  return hipGetLastError();
}

hipError_t launch_l2_neg_gather(const int32_t* ids, int64_t n, const float* half_norms, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(l2_neg_gather_kernel, grid_for(n, 256), dim3(256), 0, stream, ids, n, half_norms, out);
  return hipGetLastError();
}

size_t l2_topk_ws_bytes(int64_t nx_pad, int64_t ny_pad, int k, int d) {
  return XsimWs(nullptr, nx_pad, ny_pad, round_k(k), (int64_t)d * sizeof(f16), L2_CHUNK_ROWS).bytes();
}

hipError_t launch_l2_topk(const f16* X, int64_t nx, int64_t nx_pad, const f16* Y, int64_t ny, int64_t ny_pad, int d, int k,
                          int64_t y_off, const float* y_bias, int32_t* idx, float* score, void* ws, hipStream_t stream) {
  return xs_with_k(k, [&](auto K) {
    return xsim_run(
        X, nx, nx_pad, Y, ny, ny_pad, (int64_t)d * sizeof(f16), L2_CHUNK_ROWS, k, y_off, idx, score, ws, stream,
        [&](dim3 grid, const XsimWs& w, int ntx, int nty, int nchunks, int tpc) {
          constexpr int lds = G2_LDS_BYTES + XsF16Bias<K()>::LDS_ABOVE;  // the ring, the row lists and 8 slots of y biases
          static_assert(lds <= 160 * 1024, "the ring, the lists and the bias slots fit the LDS of a CU");
          return launch_with_lds<l2_tile256_kernel<K()>>(grid, G2_THREADS, lds, stream, (const f16*)w.xtm, (const f16*)w.ytm,
                                                         y_bias, d, ntx, nty, nchunks, tpc, (int)ny, (int)nx_pad, w.ps, w.pi);
        });
  });
}

}  // namespace smi

extern "C" {

int smi_l2_prepare(const void* src, int32_t src_dtype, int64_t rows, int32_t d, void* dst_f16, float* half_norms, void* stream) {
  if (!src || !dst_f16) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (src_dtype != SMI_F32 && src_dtype != SMI_F16) return fail(SMI_ERR_INVALID_ARG, "bad dtype");
  if (rows <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  if (rows > 0x7fffff00LL) return fail(SMI_ERR_UNSUPPORTED, "rows=%lld: row numbers must fit int32", (long long)rows);
  if (d <= 0 || d % 8) return fail(SMI_ERR_UNSUPPORTED, "d=%d must be a multiple of 8", d);
  if (((uintptr_t)src | (uintptr_t)dst_f16) % 16) return fail(SMI_ERR_INVALID_ARG, "src and dst must be 16-byte aligned");
  if ((uintptr_t)half_norms % 4) return fail(SMI_ERR_INVALID_ARG, "half_norms must be 4-byte aligned");
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(launch_l2_prepare(src, src_dtype == SMI_F32, (f16*)dst_f16, half_norms, rows, d, (hipStream_t)stream));
  return SMI_OK;
}

int64_t smi_l2_topk_ws_bytes(int64_t nx, int64_t ny, int32_t k, int32_t d) {
  const KeepLastError keep;
  return check_topk_shape(nx, ny, k, 8, d) ? 0 : (int64_t)l2_topk_ws_bytes(smi_xsim_padded_rows(nx), smi_xsim_padded_rows(ny), k, d);
}

int smi_l2_topk(const void* x_f16, int64_t nx, const void* y_f16, int64_t ny, int32_t d, int32_t k, int64_t y_off,
                const float* y_bias, int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream) {
  if (!x_f16 || !y_f16 || !idx || !score) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (!y_bias) return fail(SMI_ERR_INVALID_ARG, "null y_bias: one fp32 per padded y row (zeros for the inner product)");
  if (int rc = check_topk_shape(nx, ny, k, 8, d)) return rc;
  if (((uintptr_t)x_f16 | (uintptr_t)y_f16 | (uintptr_t)y_bias) % 16)
    return fail(SMI_ERR_INVALID_ARG, "rows and y_bias must be 16-byte aligned");
  if (int rc = check_ws(ws, ws_bytes, (size_t)smi_l2_topk_ws_bytes(nx, ny, k, d), "smi_l2_topk_ws_bytes(nx, ny, k, d)")) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(launch_l2_topk((const f16*)x_f16, nx, smi_xsim_padded_rows(nx), (const f16*)y_f16, ny, smi_xsim_padded_rows(ny), d, k,
                         y_off, y_bias, idx, score, ws, (hipStream_t)stream));
  return SMI_OK;
}

int smi_l2_slot_bias(const int32_t* list_ids, int64_t slots, const float* half_norms, float* out, void* stream) {
  if (!list_ids || !half_norms || !out) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (slots <= 0) return fail(SMI_ERR_INVALID_ARG, "slots=%lld: empty input", (long long)slots);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(launch_l2_neg_gather(list_ids, slots, half_norms, out, (hipStream_t)stream));
  return SMI_OK;
}

}  // extern "C"
