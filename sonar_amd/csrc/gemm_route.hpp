// Which GEMM engine a launch gets: ONE pure function of the request and of what it reads from the outside.  Host-only: no HIP
// header, no HIP call, no static or thread-local state -- tests/test_gemm_route_cpu.py replays a recorded table through it
// (smi_gemm_route) without a device.  launch_gemm_tn / launch_gemm_tn_splitk (gemm.hip) build a GemmRequest, call gemm_route
// and dispatch on route.engine; the engine files only turn a route into a kernel instantiation and launch it.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace smi {

enum GemmEpilogue {
  EPI_BIAS_F16 = 0, EPI_RELU_F16 = 1, EPI_RESID_F32 = 2, EPI_STORE_F32 = 3,
  EPI_RESID_HALF_F32 = 4, EPI_SILU_F16 = 5, EPI_GLU_F16 = 6, EPI_TANH_F16 = 7, EPI_RESID_F16 = 8,
  EPI_RESID_HALF_F16 = 9
};

// layout flags OR-ed into epi_sel (tile-major layout: common.hpp tm_offset)
constexpr int GEMM_IN_TM = 1 << 12;   // X and W are tile-major (M, N % 256 == 0)
constexpr int GEMM_OUT_TM = 1 << 13;  // fp16 output is tile-major with K = N (needs GEMM_IN_TM, ldo == N)

// GemmLnFold (kernels.hpp) as the router sees it.  Producer: part_in null, the residual epilogue read-modify-writes the tile-major
// stream and (SUMS: part_out given) leaves the rows' partial sums; consumer: part_in given, exact mean term or centred weights
enum GemmFoldKind { FOLD_NONE = 0, FOLD_PRODUCER = 1, FOLD_PRODUCER_SUMS = 2, FOLD_CONSUMER_EXACT = 3, FOLD_CONSUMER_CENTRED = 4 };
// GemmTileStats as the router sees it.  POSITIVE: both arrays given and scale > 0, what the 4-wave engine's fused pass needs;
// OTHER: present otherwise (the 8-wave engine's general pass)
enum GemmStatsKind { STATS_NONE = 0, STATS_POSITIVE = 1, STATS_OTHER = 2 };

struct GemmRequest {
  int epi, sel;  // epilogue; engine selector: 0 auto, 1 force the 128x128 family, 2 force 256x256
  bool in_tm, out_tm, has_bias;
  int M, N, K, ldo;
  int fold, fold_nparts;  // GemmFoldKind
  bool fold_has_c1;
  int stats, ksplit;      // GemmStatsKind
  bool slab_f16, splitk;  // splitk: the request of launch_gemm_tn_splitk (epi, sel, out_tm, ldo, fold, stats unused)
};

// What the decision reads from the outside (gemm.hip: gemm_env() is the only place that fills it)
struct GemmEnv {
  int num_cus, grid_cap, lone, lone16, lone_ks, g2_auto_min, g2_splitk_min, g2v2, g2v2_min, dec_m160, g2_raster;
};

enum GemmEngine {
  GEMM_NONE = 0,    // no engine takes the request
  GEMM_RING,        // gemm_tn_kernel: 128x128 tiles, ring = 0 (two stages, 2 workgroups per CU) or 4
  GEMM_LONE64,      // gemm_lone_kernel: 64x64 lone units
  GEMM_LONE16,      // gemm_lone16_kernel: k-sliced 64x64 units, unit = NKB
  GEMM_PP256,       // gemm_tn256_kernel: the 8-wave 256x256 ping-pong engine
  GEMM_V2,          // gemm_v2_kernel: the 4-wave engine, flag = FOLD
  GEMM_V2_RESID,    // gemm_v2_resid_kernel, flag = EMIT
  GEMM_V2_STATS,    // gemm_v2_stats_kernel
  GEMM_V2_LONE128, GEMM_V2_LONE160, GEMM_V2_LONE192,  // gemm_v2_lone_kernel, unit = rows, flag = SLAB
  GEMM_ENGINE_COUNT
};

struct GemmRoute {
  int engine;              // GemmEngine
  int epi, layout;         // template coordinates: EPI, LAYOUT (gemm.hip; the 4-wave engines: 2 tile-major out, 3 residual stream)
  int ring, unit, flag;    // ring depth | NKB or unit rows | FOLD / EMIT / SLAB
  int grid_x, grid_y, lds_bytes, ksplit, raster;
  int64_t part_stride;     // bytes between split-K slabs
};

// LDS sizes and limits of the engines as the router needs them; each engine file asserts them against its own header
constexpr int ROUTE_LDS_RING_STAGE = 32 << 10, ROUTE_LDS_LONE64 = 64 << 10, ROUTE_LDS_LONE16 = 64 << 10, ROUTE_LDS_PP256 = 160 << 10,
              ROUTE_LDS_V2 = 160 << 10, ROUTE_V2_MIN_SLICES = 8;
// tile edges (T) and K steps (BK) of the 256x256 engines and the tile-major block, the 128x128 ring, the 64x64 lone units
constexpr int ROUTE_T256 = 256, ROUTE_T128 = 128, ROUTE_T64 = 64, ROUTE_BK256 = 32, ROUTE_BK128 = 64;
constexpr int route_lds_v2_lone(int rows) { return (160 * 1024) / (rows * 64 + 16384) * (rows * 64 + 16384); }

namespace route_detail {

// 64x64 units, two workgroups per CU (64 KiB of LDS each): used while all units are resident at once.  Measured
// (profiles/r04_experiments.txt, experiment 11): at M = 256 / 512 every projection of the encoder is 25-35 % faster than on
// 128x128 tiles (more CUs stream operands, a unit has a quarter of the MFMAs and half the LDS traffic); past ~2 units
// per CU (M = 1280 x N = 3072: 960 units) the 128x128 ring wins again -- a 64x64 unit moves twice the operand bytes per
// flop through L2.
inline bool lone64_fits(int M, int N, int ks, const GemmEnv& e) { return (int64_t)(M / ROUTE_T64) * (N / ROUTE_T64) * ks <= 2 * (int64_t)e.num_cus; }
inline bool ring_fits(int M, int N, int ks, const GemmEnv& e) { return (int64_t)(M / ROUTE_T128) * (N / ROUTE_T128) * ks <= e.num_cus; }

inline bool is_resid_f16(int epi) { return epi == EPI_RESID_F16 || epi == EPI_RESID_HALF_F16; }
inline bool is_consumer(int fold) { return fold == FOLD_CONSUMER_EXACT || fold == FOLD_CONSUMER_CENTRED; }

// The 4-wave 256x256 engine (gemm_v2.hip) takes tile-major fp16 in / out launches with >= 8 K slices: the residual-stream
// epilogues (fold: producer side only), and bias | relu | silu | GLU with a bias and optionally a LayerNorm-fold consumer
// (silu and GLU: centred weights only).
inline bool v2_fits(const GemmRequest& q, const GemmEnv& e, int fold) {
  if (e.g2v2 == 0) return false;
  if (q.M % ROUTE_T256 || q.N % ROUTE_T256 || q.K % 128 || q.K / ROUTE_BK256 < ROUTE_V2_MIN_SLICES) return false;
  // from half a chip of tiles up (the automatic 256x256 threshold): measured same box with the threshold at 128 instead of
  // 512, decoder C5 3.62 -> 3.58 ms per step, C1 2.66 -> 2.63 ms (profiles/r06_experiments.txt, experiment 6)
  if ((int64_t)(q.M / ROUTE_T256) * (q.N / ROUTE_T256) < e.g2v2_min) return false;
  if (is_resid_f16(q.epi)) return !is_consumer(fold);  // tile-major residual stream; fold: producer side only
  if (q.epi != EPI_BIAS_F16 && q.epi != EPI_RELU_F16 && q.epi != EPI_SILU_F16 && q.epi != EPI_GLU_F16) return false;
  if (!q.has_bias) return false;
  if (fold != FOLD_NONE && (!is_consumer(fold) || !q.fold_has_c1 || q.fold_nparts < 1 || q.fold_nparts > 4)) return false;
  if (fold != FOLD_NONE && (q.epi == EPI_SILU_F16 || q.epi == EPI_GLU_F16) && fold != FOLD_CONSUMER_CENTRED) return false;
  return true;
}

// Rows per lone unit of the 4-wave engine (128 / 160 / 192) for a launch, or 0: the tallest of the three heights that divides M,
// keeps every unit on a CU of its own and puts MORE units on the chip than 256-row tiles would (M a multiple of 256: the
// tile-major image has 256-row blocks).
inline int v2_lone_rows(int M, int N, int K, int ksplit, const GemmEnv& e) {
  const int mode = e.dec_m160;
  if (mode == 0) return 0;
  if (M % ROUTE_T256 || N % ROUTE_T256 || K % ROUTE_BK256 || ksplit < 1 || (K / ROUTE_BK256) % ksplit) return 0;
  const int nt = K / ROUTE_BK256 / ksplit;
  // units with a K loop of >= 32 slices (K >= 1024 per unit): the attention-output projection's 16-slice units measured 18-19 %
  // SLOWER than the k-sliced 64x64 units they would replace (tools/probe_lone.py, profiles/r06r_probe_lone.log); DEC_M160=2 (tests)
  // takes every K loop the ring can run
  if (nt < (mode == 2 ? 8 : 32) || nt % 2) return 0;
  const int64_t units256 = (int64_t)(M / ROUTE_T256) * (N / ROUTE_T256) * ksplit;
  int best = 0;
  int64_t best_units = units256;
  for (int rows : {192, 160, 128}) {
    if (M % rows) continue;
    const int64_t units = (int64_t)(M / rows) * (N / ROUTE_T256) * ksplit;
    // at least half the chip: below that the k-sliced 64x64 units (gemm_lone16.hpp: M = 256, a batch of 5) are faster
    if (units <= e.num_cus && units >= (mode == 2 ? 1 : e.num_cus / 2) && units > best_units) {
      best = rows;
      best_units = units;
    }
  }
  return best;
}

inline GemmRoute none() { return GemmRoute{GEMM_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// mode: tile-major fp16 relu / bias output (ksplit 1), or slab: row-major fp16 split-K slabs [ksplit][M][N]
inline GemmRoute v2_lone(int rows, int epi, bool slab, const GemmRequest& q, int ksplit) {
  const int engine = rows == 128 ? GEMM_V2_LONE128 : rows == 160 ? GEMM_V2_LONE160 : GEMM_V2_LONE192;
  return GemmRoute{engine, epi, slab ? 1 : 2, 0, rows, slab, (q.M / rows) * (q.N / ROUTE_T256) * ksplit, 1, route_lds_v2_lone(rows),
                   ksplit, 0, slab ? (int64_t)q.M * q.N * 2 : 0};
}

// XCD-owned m-groups (see gemm_tn256_kernel): whole chip, >= 4 n-quads, and a number of m-groups (8 row tiles each) that
// deals evenly to the 8 XCDs -- otherwise the id-order raster balances better.  G2_RASTER=0 restores the id-order raster
// everywhere (A/B measurements).
inline int raster_of(const GemmEnv& e, int ksplit, int grid, int ntm, int ntn) {
  return (e.g2_raster && ksplit == 1 && grid == 256 && ntn % 4 == 0 && ntn >= 16 && ((ntm + 7) / 8) % 8 == 0) ? e.g2_raster : 0;
}

// the persistent 256x256 engines: one workgroup per CU at the most
inline GemmRoute persistent(int engine, int epi, int layout, int flag, const GemmRequest& q, const GemmEnv& e, int ksplit,
                            int64_t part_stride) {
  const int ntm = q.M / ROUTE_T256, ntn = q.N / ROUTE_T256;
  int grid = std::min(ntm * ntn * ksplit, e.num_cus);
  // the grid cap of the calling thread (set_gemm_grid_cap): the 8-wave engine and the logits GEMM of the 4-wave one
  if (e.grid_cap > 0 && (engine == GEMM_PP256 || engine == GEMM_V2_STATS)) grid = std::min(grid, e.grid_cap);
  const int raster = engine == GEMM_V2_STATS ? 0 : raster_of(e, ksplit, grid, ntm, ntn);
  return GemmRoute{engine, epi, layout, 0, 0, flag, grid, 1, engine == GEMM_PP256 ? ROUTE_LDS_PP256 : ROUTE_LDS_V2, ksplit, raster,
                   part_stride};
}
inline GemmRoute pp256(int epi, int layout, const GemmRequest& q, const GemmEnv& e, int ksplit = 1, int64_t ps = 0) {
  return persistent(GEMM_PP256, epi, layout, 0, q, e, ksplit, ps);
}
inline GemmRoute v2(const GemmRequest& q, const GemmEnv& e, int fold) {
  if (is_resid_f16(q.epi)) return persistent(GEMM_V2_RESID, q.epi, 3, fold == FOLD_PRODUCER_SUMS, q, e, 1, 0);
  return persistent(GEMM_V2, q.epi, 2, fold != FOLD_NONE, q, e, 1, 0);
}

// the 128x128 family: the k-sliced unit, the 64x64 lone unit, the ring with four stages or two
inline GemmRoute small(int epi, int layout, const GemmRequest& q, const GemmEnv& e, int ksplit = 1, int64_t part_stride = 0) {
  const int M = q.M, N = q.N, K = q.K;
  // the k-sliced unit (gemm_lone16.hpp): tile-major operands, K per unit 256 / 512 / 1024.  LONE16=0: the LDS-ring unit
  // for every lone launch (A/B runs; its results are bit-identical to the other 128x128-family engines, these are not)
  if ((epi == EPI_BIAS_F16 || epi == EPI_RELU_F16 || epi == EPI_STORE_F32) && (layout == 1 || layout == 2)) {
    const int klen = K / ksplit;
    if (e.lone && e.lone16 && lone64_fits(M, N, ksplit, e) && K % ksplit == 0 && (klen == 256 || klen == 512 || klen == 1024) &&
        (epi != EPI_STORE_F32 || layout == 1))
      return GemmRoute{GEMM_LONE16, epi, layout, 0, klen / 128, 0, (M / ROUTE_T64) * (N / ROUTE_T64), ksplit, ROUTE_LDS_LONE16, ksplit, 0, part_stride};
  }
  // LONE: 0 = round 3's ring for every lone-tile launch (A/B runs; read per launch: decode-time paths switch it per
  // call), otherwise 64x64 units of the lone-tile engine (gemm_lone.hpp) when a launch is small enough for them.
  // (GLU pairs two 32-column blocks of a wave: 128-column tiles only)
  if (epi != EPI_GLU_F16 && e.lone && lone64_fits(M, N, ksplit, e))
    return GemmRoute{GEMM_LONE64, epi, layout, 0, 64, 0, (M / ROUTE_T64) * (N / ROUTE_T64), ksplit, ROUTE_LDS_LONE64, ksplit, 0, part_stride};
  // every workgroup gets a CU of its own: hide the DMA latency with a deeper ring instead of a second workgroup
  const int ring = ring_fits(M, N, ksplit, e) ? 4 : 0;
  return GemmRoute{GEMM_RING, epi, layout, ring, 0, 0, (M / ROUTE_T128) * (N / ROUTE_T128), ksplit, (ring ? ring : 2) * ROUTE_LDS_RING_STAGE, ksplit, 0,
                   part_stride};
}

// LAYOUT of the 128x128 family and the 8-wave engine for an (epilogue, layout flags) pair, -1 where no kernel exists
inline int layout_of(int epi, bool in_tm, bool out_tm) {
  if (out_tm)  // fp16 outputs that feed the next GEMM; EPI_RESID_F16: the tile-major residual stream
    return epi == EPI_BIAS_F16 || epi == EPI_RELU_F16 || epi == EPI_SILU_F16 ? 2 : is_resid_f16(epi) ? 3 : -1;
  if (in_tm)
    return epi == EPI_RELU_F16 || epi == EPI_SILU_F16 || epi == EPI_TANH_F16 || epi < 0 || epi > EPI_RESID_HALF_F16 ? -1 : 1;
  return epi < 0 || epi > EPI_RESID_HALF_F16 ? -1 : 0;
}

// Split-K GEMM into `ksplit` slabs (launch_gemm_tn_splitk)
inline GemmRoute route_splitk(const GemmRequest& q, const GemmEnv& e) {
  const int M = q.M, N = q.N, K = q.K, ksplit = q.ksplit;
  if (M % ROUTE_T128 || N % ROUTE_T128 || ksplit < 1 || K % ROUTE_BK128 || M <= 0) return none();
  if (q.in_tm && (M % ROUTE_T256 || N % ROUTE_T256)) return none();
  // the 256x256 ping-pong engine is far more efficient per CU than the 128x128 one (decoder FFN inner:
  // 160 tiles on 256 CUs still beat 640 small tiles); use it when the units roughly fill the chip once
  // and every unit has a real K loop (its K parts may be unequal)
  const int units256 = (M / ROUTE_T256) * (N / ROUTE_T256) * ksplit;
  const int64_t ps = (int64_t)M * N * (q.slab_f16 ? 2 : 4);
  const bool big = M % ROUTE_T256 == 0 && N % ROUTE_T256 == 0 && (K / ROUTE_BK256) / ksplit >= 16 && units256 >= e.g2_splitk_min && units256 <= e.num_cus;
  if (!big && K % (ROUTE_BK128 * ksplit)) return none();  // the 128x128 engine splits K evenly
  const int epi = q.slab_f16 ? EPI_BIAS_F16 : EPI_STORE_F32, layout = q.in_tm ? 1 : 0;
  if (q.slab_f16 && q.in_tm) {
    // a decode step's FFN-output projection (M = 1280 rows): 8 x 4 tiles x 8 K parts = 256 lone units (gemm_v2_lone.hip)
    if (const int rows = v2_lone_rows(M, N, K, ksplit, e)) return v2_lone(rows, EPI_BIAS_F16, true, q, ksplit);
  }
  return big ? pp256(epi, layout, q, e, ksplit, ps) : small(epi, layout, q, e, ksplit, ps);
}

}  // namespace route_detail

inline GemmRoute gemm_route(const GemmRequest& q, const GemmEnv& e) {
  using namespace route_detail;
  if (q.splitk) return route_splitk(q, e);
  const int epi = q.epi, sel = q.sel, M = q.M, N = q.N, K = q.K;
  const bool in_tm = q.in_tm, out_tm = q.out_tm;
  if (M % ROUTE_T128 || N % ROUTE_T128 || K % ROUTE_BK128 || M <= 0) return none();
  if (in_tm && (M % ROUTE_T256 || N % ROUTE_T256)) return none();
  if (out_tm && (!in_tm || q.ldo != (epi == EPI_GLU_F16 ? N / 2 : N))) return none();
  const bool can256 = M % ROUTE_T256 == 0 && N % ROUTE_T256 == 0;
  if (sel == 2 && !can256) return none();
  // the 256x256 ping-pong engine is ~1.5x more efficient per CU than the 128x128 one but has a 21 us
  // floor for a K = 1024 tile and one workgroup per CU; measured crossover (tools/probe_engines.py):
  // 128 tiles tie, 160 tiles win; round 4 (tools/probe_engines_mid.py, M = 1024 x N = 8192 = 128 tiles, tile-major operands): 25.8 vs
  // 28.6 us hot, 31.8 vs 33.8 us on cold weights -> use it from 128 tiles (half the CUs) up
  // (G2_AUTO_MIN overrides the threshold, read per launch: tests that compare runs of different row counts bit for bit
  // pin the engine family with it)
  const bool use256 = sel == 2 || (sel == 0 && can256 && (int64_t)(M / ROUTE_T256) * (N / ROUTE_T256) >= e.g2_auto_min);
  if (q.fold != FOLD_NONE) {  // LayerNorm fold: 256x256 engines, tile-major stream
    if (!can256 || sel == 1 || !in_tm || q.stats != STATS_NONE) return none();
    if (is_consumer(q.fold)) {  // tile-major outputs (bias / relu / silu; GLU on the 4-wave engine) or row-major ones (bias / GLU; centred weights)
      if (!q.fold_has_c1 || q.fold_nparts < 1 || q.fold_nparts > 4) return none();
      const bool centred = q.fold == FOLD_CONSUMER_CENTRED;
      if (out_tm) {
        // the 4-wave engine where it applies: >= 8 K slices, G2V2_MIN tiles
        if (v2_fits(q, e, q.fold)) return v2(q, e, q.fold);
        if (epi == EPI_BIAS_F16 || epi == EPI_RELU_F16 || (epi == EPI_SILU_F16 && centred)) return pp256(epi, 2, q, e);
        return none();
      }
      if (centred && (epi == EPI_BIAS_F16 || epi == EPI_GLU_F16)) return pp256(epi, 1, q, e);
      return none();
    }
    // producer: the tile-major residual epilogue (part_out may be null: plain read-modify-write of the stream)
    if (!out_tm || !is_resid_f16(epi)) return none();
    return v2_fits(q, e, q.fold) ? v2(q, e, q.fold) : pp256(epi, 3, q, e);
  }
  if (q.stats != STATS_NONE) {  // tile statistics: the 256x256 engines' tile-major fp16 store or the 8-wave one's fp32 store, without a bias
    if (epi == EPI_BIAS_F16 && out_tm && in_tm && can256 && sel != 1 && !q.has_bias) {
      // the 4-wave engine's fused pass: G2V2 = 1 (2: everything but the logits), scale > 0, >= 8 K slices, G2V2_MIN tiles
      if (e.g2v2 == 1 && q.stats == STATS_POSITIVE && K % 128 == 0 && K / ROUTE_BK256 >= ROUTE_V2_MIN_SLICES &&
          (int64_t)(M / ROUTE_T256) * (N / ROUTE_T256) >= e.g2v2_min)
        return persistent(GEMM_V2_STATS, EPI_BIAS_F16, 2, 0, q, e, 1, 0);
      return pp256(EPI_BIAS_F16, 2, q, e);
    }
    if (epi != EPI_STORE_F32 || out_tm || !can256 || sel == 1 || q.has_bias) return none();
    return pp256(EPI_STORE_F32, in_tm ? 1 : 0, q, e);
  }
  if (out_tm) {
    // a decode step's FFN-inner projection (M = 1280 rows): 256 lone units of 160 x 256 instead of 160 of 256 x 256
    // (and the small-batch encoder's fused QKV projection: bias, tile-major out)
    if ((epi == EPI_RELU_F16 || epi == EPI_BIAS_F16) && sel != 1) {
      if (const int rows = v2_lone_rows(M, N, K, 1, e)) return v2_lone(rows, epi, false, q, 1);
    }
    if (use256 && v2_fits(q, e, FOLD_NONE)) return v2(q, e, FOLD_NONE);
  }
  const int layout = layout_of(epi, in_tm, out_tm);
  if (layout < 0) return none();
  return use256 ? pp256(epi, layout, q, e) : small(epi, layout, q, e);
}

// How many K parts launch_gemm_tn_splitk should be given for a decode-time projection (M = beam x batch rows,
// N = model_dim): as many as keep EVERY unit on a CU of its own -- one round of lone tiles is the fastest a
// latency-bound launch gets -- without starving a unit of K loop.  <= max_parts (the slab buffer).
inline int gemm_splitk_parts(int M, int N, int K, int max_parts, const GemmEnv& e) {
  using namespace route_detail;
  if (M % ROUTE_T256 == 0 && N % ROUTE_T256 == 0) {
    const int tiles = (M / ROUTE_T256) * (N / ROUTE_T256);
    const int ks = std::min(std::min(max_parts, e.num_cus / std::max(tiles, 1)), (K / ROUTE_BK256) / 16);
    if (ks >= 1 && tiles * ks >= 96) return ks;
  }
  if (e.lone) {
    // Lone-tile units: the part count with the cheapest launch by a two-term model -- K tiles per unit x the time of one
    // K tile (measured: 0.15 us for a 64x64 unit with a CU of its own, 0.25 us with two per CU, 0.41 us for a 128x128
    // ring unit), plus what every part adds around the launch (its slab is written here and read by the consumer:
    // 8 bytes per output element at ~20 TB/s, it is L2 / Infinity-Cache traffic); a unit keeps at least 4 K tiles.
    // LONE_KS overrides (A/B runs).
    if (const int v = e.lone_ks) {
      if (v >= 1 && v <= max_parts && K % (ROUTE_BK128 * v) == 0 && (lone64_fits(M, N, v, e) || ring_fits(M, N, v, e))) return v;
    }
    int best = 1;
    double best_cost = 1e30;
    for (int ks = 1; ks <= max_parts; ks *= 2) {
      if (K % (ROUTE_BK128 * ks) || (ks > 1 && K / ks < 4 * ROUTE_BK128)) break;
      double t_tile;
      if (lone64_fits(M, N, ks, e))
        t_tile = (int64_t)(M / ROUTE_T64) * (N / ROUTE_T64) * ks <= e.num_cus ? 0.15 : 0.25;
      else if (ring_fits(M, N, ks, e))
        t_tile = 0.41;
      else
        break;
      const double cost = (K / ks / ROUTE_BK128) * t_tile + ks * ((double)M * N * 8.0 / 20e6);
      if (cost < best_cost) {
        best_cost = cost;
        best = ks;
      }
    }
    return best;
  }
  const int tiles = (M / ROUTE_T128) * (N / ROUTE_T128);
  int ks = 1;
  while (ks * 2 <= max_parts && tiles * ks * 2 <= e.num_cus && K % (ROUTE_BK128 * ks * 2) == 0 && K / (ks * 2) >= 2 * ROUTE_BK128) ks *= 2;
  return ks;
}

}  // namespace smi
