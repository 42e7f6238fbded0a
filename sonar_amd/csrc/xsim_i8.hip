// Brute-force top-k on int8 rows: xsim.hip's walk on the integer MFMA.  For every row of X (the query side)
// the k best rows of Y (the stored side) by the score of the int8 IVF index (3.19, tests/ivf_i8_ref.py),
//   score = fl32(fl32((float)acc * s_y[n]) * s_x[m]),   acc = sum_j cx[m][j] * cy[n][j] in int32 (exact),
// codes and scales from smi_ivf_i8_encode over the padded output of smi_xsim_normalize.  The bits of a score depend on the two
// fp16 rows alone, so they are the bits IVFInt8Index.search returns for the same pair.
//
// The tile kernel is the walk of xsim_walk.hpp (why one byte geometry serves fp16 and int8 is said there) over the policy XsI8
// below.  What differs from the fp16 pass: the MFMA, nt = d / 64 slices per tile instead of d / 32, and the fold, which turns
// the int32 sums into scores.
//
// The fold.  A lane holds 8 x rows (wr * 128 + mi * 16 + l15; their scales sx[8] are loaded once per workgroup) against 16 y
// columns (wc * 64 + ni * 16 + 4 kg + r; the 256 scales of a y tile travel in the DMA stream with the tile's first slice into a
// slot of LDS, and a lane takes its 16 with four 16-byte LDS reads per tile: nothing the fold waits for is in flight, and the
// scales cost no registers outside the fold).  t = fl32((float)acc * s_y) is formed for all 128 sums; the test of a
// row against its threshold is made on fl32(max t * s_x): s_x >= 0 and a rounded product is monotone in t, so that IS the
// maximum of the row's 16 scores, and only the rows that pass multiply element by element.  The returned bits and the order are
// those of the plain fold.  Every K keeps its lists in LDS (xsim.hip's key lists; K = 1 too: one path).
//
// Order and signed zero: ivf_scan.hpp's rule.  A candidate enters when `score >= threshold` as an fp32 compare (-0 == +0
// there), and a list orders by the key of the score's BITS (topk_order.hpp), where -0 sorts below +0; the chunk merge compares
// as fp32 again (score descending, ties -- those made by the last rounding too -- to the lower index).  With exact sums a score
// of -0 needs a negative sum times a scale that underflows the product: codes of a scale-0 row are 0 and so is its sum, and the
// smallest scale of an fp16 row is 2^-24 / 127, so no row smi_ivf_i8_encode writes produces one (tests/ivf_i8_ref.edge_rows:
// zero rows score +0 against everything).  Columns n >= ny never enter a list: a pad row (codes 0, scale 0) scores +0 and would
// beat every negative score.
#include "api_common.hpp"
#include "kernels.hpp"
#include "xsim_walk.hpp"

using namespace smi;
using namespace smi_host;

namespace smi {
namespace {

constexpr int XI8_MAX_DIM = SMI_IVF_I8_MAX_DIM;
static_assert((int64_t)127 * 127 * XI8_MAX_DIM < (1LL << 31), "the int32 sum of a row pair cannot overflow");

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The int8 operand policy of the walk (xsim_walk.hpp).  xs / ys: the scales of the x and y rows, row order.
// The y scales of a tile ride the DMA stream (issue_tile, first in the group of the tile's first slice: the walk's counted
// waits hold as they are): waves 0 .. 3 copy its 256 scales (4 B per lane) into scale slot (tile & 7) above the lists.  A
// group of waves 0 .. 3 so holds 5 operations at every tile start (every group at nt = 1, every second one at nt = 2); what
// the earlier retirement costs at d <= 128 is unmeasured.  8 slots: the deferred fold of tile T reads its slot while, at one
// slice per tile, the scales of T + 4 are already on their way; T + 8's are issued after T + 4's first slice was read.
template <int K>
struct XsI8 {
  typedef int8_t elem_t;
  typedef i32x4 frag_t;  // 16 codes
  typedef i32x4 acc_t;
  static constexpr int BK = 64;
  static constexpr bool LISTS = true;          // K = 1 too: one path
  static constexpr int SCALES = 256 * K * 8;   // above the ring, behind the lists: [8 slots][256] fp32
  static constexpr int LDS_ABOVE = SCALES + 8 * 1024;
  static constexpr bool TRACED = false;
  static __device__ __forceinline__ acc_t mfma(frag_t w, frag_t x, acc_t c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(w, x, c, 0, 0, 0);
  }

  struct tile_t {
    f32x4 sy[4];  // sy[ni][r]: the scales of the lane's y columns in the tile being folded
  };
  const float *xs, *ys;
  float sx[8];      // the scales of this lane's x rows
  const float* ysg;
  unsigned sc_addr;
  int it, t_begin;
  __device__ __forceinline__ XsI8(const float* xs_, const float* ys_) : xs(xs_), ys(ys_) {}

  __device__ __forceinline__ void init(const XsLane& L, char* above, int m0, int t_begin_) {
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) sx[mi] = xs[L.row(mi, m0)];
    sc_addr = (unsigned)(size_t)(above + SCALES) + L.col(0, 0) * 4;
    ysg = ys + (size_t)t_begin_ * G2_BN + (L.wave & 3) * 64 + L.lane;
    it = 0;
    t_begin = t_begin_;
  }
  __device__ __forceinline__ void issue_tile(char* above, int wave) {
    if (wave < 4)
      __builtin_amdgcn_global_load_lds(SMI_GLOBAL_PTR(ysg), SMI_LDS_PTR(above + SCALES + (it & 7) * 1024 + wave * 256), 4, 0, 0);
    ysg += G2_BN;
    ++it;
  }
  __device__ __forceinline__ void fold_begin(int n0f, tile_t& ts) { xs_read_cols16(sc_addr + ((n0f / G2_BN - t_begin) & 7) * 1024, ts.sy); }
  // the largest score of the row's 16: s_x >= 0 and a rounded product is monotone in t = fl32(sum * s_y)
  __device__ __forceinline__ float row_max(const acc_t (&acc)[4][8], int mi, const tile_t& ts) const {
    float tmax = -INFINITY;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, __fmul_rn((float)acc[ni][mi][r], ts.sy[ni][r]));
    return __fmul_rn(tmax, sx[mi]);
  }
  __device__ __forceinline__ float score(const acc_t (&acc)[4][8], int ni, int mi, int r, const tile_t& ts) const {
    // (an opaque copy of the sum: or hipcc keeps the 128 products of row_max alive for the insertion path and spills)
    int a = acc[ni][mi][r];
    asm volatile("" : "+v"(a));
    return __fmul_rn(__fmul_rn((float)a, ts.sy[ni][r]), sx[mi]);
  }
};

// Xc / Yc: tile-major copies of the codes
template <int K>
__global__ __launch_bounds__(G2_THREADS) void xsim_i8_tile256_kernel(const int8_t* __restrict__ Xc, const float* __restrict__ xs,
                                                                     const int8_t* __restrict__ Yc, const float* __restrict__ ys,
                                                                     int d, int ntx, int nty, int nchunks, int tiles_per_chunk,
                                                                     int ny, int nx_pad, float* __restrict__ ps,
                                                                     int* __restrict__ pi) {
  XsI8<K> p(xs, ys);
  xsim_walk<K>(p, Xc, Yc, d, ntx, nty, nchunks, tiles_per_chunk, ny, nx_pad, ps, pi);
}

// The workspace is XsimWs (xsim_walk.hpp) over rows of d bytes with one chunk per G2_BN = 256 rows of y: chunks = min(ny_pad /
// 256, 8).  The caller sizes it with smi_xsim_workspace_bytes(nx, ny, k, d / 2), the fp16 pass's sizing call at half the
// dimension (no sizing call of its own): an int8 [rows, d] matrix IS an fp16 [rows, d / 2] matrix to everything but the MFMA,
// the workspace included.  That call holds the same bytes for both copies and lists for min(ny_pad / 128, 8) >= min(ny_pad /
// 256, 8) chunks of the same nx_pad * K entries: equal to this layout from ny_pad = 2048 on, larger by
// (min(ny_pad / 128, 8) - ny_pad / 256) * nx_pad * K * 8 bytes below.
constexpr int XI8_CHUNK_ROWS = G2_BN;

hipError_t xsim_i8_run(const int8_t* xc, const float* xs, int64_t nx, int64_t nx_pad, const int8_t* yc, const float* ys, int64_t ny,
                       int64_t ny_pad, int d, int k, int64_t y_off, int32_t* idx, float* score, void* ws, hipStream_t stream) {
  return xs_with_k(k, [&](auto K) {
    return xsim_run(
        xc, nx, nx_pad, yc, ny, ny_pad, d, XI8_CHUNK_ROWS, k, y_off, idx, score, ws, stream,
        [&](dim3 grid, const XsimWs& w, int ntx, int nty, int nchunks, int tpc) {
          constexpr int lds = G2_LDS_BYTES + XsI8<K()>::LDS_ABOVE;  // the ring, the row lists and 8 slots of y scales above it
          return launch_with_lds<xsim_i8_tile256_kernel<K()>>(grid, G2_THREADS, lds, stream, (const int8_t*)w.xtm, xs,
                                                              (const int8_t*)w.ytm, ys, d, ntx, nty, nchunks, tpc, (int)ny,
                                                              (int)nx_pad, w.ps, w.pi);
        });
  });
}

// the refusals a shape alone decides
int xi8_check_shape(int64_t nx, int64_t ny, int32_t k, int32_t d) {
  if (k < 1 || k > 8) return fail(SMI_ERR_UNSUPPORTED, "k=%d outside [1,8]", k);
  if (d <= 0 || d % 64) return fail(SMI_ERR_UNSUPPORTED, "d=%d must be a multiple of 64", d);
  if (d > XI8_MAX_DIM)
    return fail(SMI_ERR_UNSUPPORTED, "d=%d: above %d the int32 sum of int8 products could overflow", d, XI8_MAX_DIM);
  if (nx <= 0 || ny <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  if (nx > 0x7fffff00LL || ny > 0x7fffff00LL)
    return fail(SMI_ERR_UNSUPPORTED, "nx=%lld, ny=%lld: row numbers must fit int32", (long long)nx, (long long)ny);
  return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" {

int smi_xsim_topk_i8(const void* x_codes, const float* x_scales, int64_t nx, const void* y_codes, const float* y_scales, int64_t ny,
                     int32_t d, int32_t k, int64_t y_off, int32_t* idx, float* score, void* ws, int64_t ws_bytes, void* stream) {
  if (!x_codes || !x_scales || !y_codes || !y_scales || !idx || !score) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (int rc = xi8_check_shape(nx, ny, k, d)) return rc;
  if (((uintptr_t)x_codes | (uintptr_t)y_codes | (uintptr_t)x_scales | (uintptr_t)y_scales) % 16)
    return fail(SMI_ERR_INVALID_ARG, "codes and scales must be 16-byte aligned");
  const int64_t nx_pad = smi_xsim_padded_rows(nx), ny_pad = smi_xsim_padded_rows(ny);
  const size_t need = (size_t)smi_xsim_workspace_bytes(nx, ny, k, d / 2);
  if (int rc = check_ws(ws, ws_bytes, need, "smi_xsim_workspace_bytes(nx, ny, k, d / 2)")) return rc;
  if (XsimWs(nullptr, nx_pad, ny_pad, round_k(k), d, XI8_CHUNK_ROWS).bytes() > need)  // (cannot happen: see XI8_CHUNK_ROWS)
    return fail(SMI_ERR_INVALID_ARG, "the int8 layout exceeds smi_xsim_workspace_bytes(nx, ny, k, d / 2)");
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  const int8_t *xc = (const int8_t*)x_codes, *yc = (const int8_t*)y_codes;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(xsim_i8_run(xc, x_scales, nx, nx_pad, yc, y_scales, ny, ny_pad, d, k, y_off, idx, score, ws, st));
  return SMI_OK;
}

}  // extern "C"
