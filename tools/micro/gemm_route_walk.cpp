// Stand-alone host walk of the GEMM router over the recorded table:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I sonar_amd/csrc tools/micro/gemm_route_walk.cpp -o route_walk
//   ./route_walk tests/golden/gemm_routes.json
// Fills GemmRequest / GemmEnv directly (no library, no HIP), calls gemm_route / gemm_splitk_parts for every case line and compares
// with the recorded answer.  Second pass: for every distinct route on a persistent 256x256 engine (GEMM_PP256, GEMM_V2,
// GEMM_V2_RESID, GEMM_V2_STATS) it replays the tile walk of all grid_x workgroups with gemm_walk.hpp, as the kernels spell it,
// and checks that every (tile_m, tile_n, K part) is visited exactly once and nothing out of range is produced; the same for a
// few synthetic grids with a partial last m-group under rasters 1 and 2.  Exit status 1 on a mismatch or a missed walk.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "gemm_route.hpp"
#include "gemm_walk.hpp"

using namespace smi;

static std::vector<long long> ints_after(const char* s, const char* key) {  // the JSON int list that follows `key`
  std::vector<long long> v;
  const char* p = strstr(s, key);
  if (!p) return v;
  for (p += strlen(key); *p && *p != ']';) {
    char* e;
    v.push_back(strtoll(p, &e, 10));
    p = *e == ',' ? e + 1 : e;
  }
  return v;
}

// The walk of all `grid` workgroups over ntm x ntn tiles x ksplit K parts.  parts: gemm_tn256_kernel (ids over the K parts,
// kz = id / tiles under raster 0); else the 4-wave kernels; stats_walk: gemm_v2_stats_kernel (raster 0 without a seek).
static bool walk_ok(int ntm, int ntn, int ksplit, int raster, int grid, bool parts, bool stats_walk) {
  const int nout = ntm * ntn, nq = ntn / 4;
  const int nvirt = raster ? walk_nvirt(ntm, nq) : nout * ksplit;
  std::vector<int> seen((size_t)nout * ksplit, 0);
  bool ok = true;
  for (int b = 0; b < grid && ok; ++b) {
    int tile_m = 0, tile_n = 0;
    auto seek = [&](int t) {
      while (t < nvirt && !(parts ? walk_coords_parts(t, raster, ntm, ntn, nq, nout, tile_m, tile_n)
                                  : walk_coords(t, raster, ntm, ntn, nq, tile_m, tile_n)))
        t += grid;
      return t;
    };
    int tile = xcd_remap(b, grid);
    if (!stats_walk) tile = seek(tile);
    while (tile < nvirt) {
      if (stats_walk) walk_grouped(tile, ntm, ntn, tile_m, tile_n);
      const int kz = raster ? 0 : tile / nout;
      if (tile_m < 0 || tile_m >= ntm || tile_n < 0 || tile_n >= ntn || kz < 0 || kz >= ksplit) {
        fprintf(stderr, "walk out of range: tile (%d, %d, part %d) of %d x %d x %d, raster %d, grid %d\n", tile_m, tile_n, kz, ntm, ntn,
                ksplit, raster, grid);
        return false;
      }
      ++seen[((size_t)kz * ntm + tile_m) * ntn + tile_n];
      tile = stats_walk ? tile + grid : seek(tile + grid);
    }
  }
  for (int v : seen) ok = ok && v == 1;
  if (!ok) fprintf(stderr, "walk misses or repeats a tile: %d x %d x %d, raster %d, grid %d\n", ntm, ntn, ksplit, raster, grid);
  return ok;
}

static std::set<std::tuple<int, int, int, int, int, int>> walked;  // (kind, ntm, ntn, ksplit, raster, grid) already replayed
static long nwalks = 0, bad_walks = 0;

static void check_walk(const GemmRoute& r, int M, int N) {
  if (r.engine != GEMM_PP256 && r.engine != GEMM_V2 && r.engine != GEMM_V2_RESID && r.engine != GEMM_V2_STATS) return;
  const bool parts = r.engine == GEMM_PP256, stats_walk = r.engine == GEMM_V2_STATS;
  const int ksplit = r.ksplit > 0 ? r.ksplit : 1, raster = stats_walk ? 0 : r.raster;
  if (!walked.emplace(parts ? 0 : stats_walk ? 2 : 1, M / ROUTE_T256, N / ROUTE_T256, ksplit, raster, r.grid_x).second) return;
  ++nwalks;
  if (!walk_ok(M / ROUTE_T256, N / ROUTE_T256, ksplit, raster, r.grid_x, parts, stats_walk)) ++bad_walks;
}

static std::vector<long long> route_fields(const GemmRequest& q, const GemmEnv& env) {
  const GemmRoute r = gemm_route(q, env);
  if (r.engine == GEMM_NONE) return {0};
  check_walk(r, q.M, q.N);
  return {r.engine, r.epi, r.layout, r.ring, r.unit, r.flag, r.grid_x, r.grid_y, r.lds_bytes, r.ksplit, r.raster, r.part_stride};
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  // the switch names of the table's header, in its order
  const char* known[] = {"DEC_M160", "G2V2", "G2V2_MIN", "G2_AUTO_MIN", "G2_RASTER", "G2_SPLITK_MIN", "LONE", "LONE16", "LONE_KS"};
  std::vector<int> order;
  std::vector<char> line(1 << 16);
  long ncases = 0, bad = 0;
  std::vector<long long> gm, gn, gk;            // the grid of the [3 | 4, ...] lines
  std::vector<std::vector<long long>> answers;  // [2, ...] lines, numbered from 1
  while (fgets(line.data(), (int)line.size(), f)) {
    if (strstr(line.data(), "\"grid\":{")) {
      gm = ints_after(line.data(), "\"m\":["), gn = ints_after(line.data(), "\"n\":["), gk = ints_after(line.data(), "\"k\":[");
    }
    if (const char* sw = strstr(line.data(), "\"switches\":[")) {
      for (const char* p = sw; (p = strchr(p, '"')) && *(p + 1) != ']';) {
        const char* e = strchr(p + 1, '"');
        if (!e) break;
        const std::string name(p + 1, e);
        for (int i = 0; i < 9; ++i)
          if (name == known[i]) order.push_back(i);
        p = e + 1;
      }
      continue;
    }
    if (line[0] != '[') continue;
    std::vector<long long> v;
    for (char* p = line.data() + 1; *p && *p != ']';) {
      char* e;
      v.push_back(strtoll(p, &e, 10));
      p = *e == ',' ? e + 1 : e;
    }
    if (v.empty() || order.size() != 9) return 2;
    if (v[0] >= 2) {  // default switches over the whole grid (format.grid_lines)
      if (v[0] == 2) {
        answers.emplace_back(v.begin() + 1, v.end());
        continue;
      }
      const size_t first = v[0] == 3 ? 7 : 3;
      std::vector<long long> want;
      for (size_t i = first; i < v.size(); ++i)
        if (v[i] < 0) want.insert(want.end(), (size_t)-v[i], want.back()); else want.push_back(v[i]);
      if (want.size() != gm.size() * gn.size() * gk.size() || want.empty()) return 2;
      const GemmEnv env{(int)v[v[0] == 3 ? 5 : 2], 0, 1, 1, 0, 128, 96, 1, 128, 1, 2};
      size_t at = 0;
      for (long long m : gm)
        for (long long n : gn)
          for (long long k : gk) {
            const long long w = want[at++];
            bool ok;
            if (v[0] == 4) {
              ok = gemm_splitk_parts((int)m, (int)n, (int)k, (int)v[1], env) == w;
            } else {
              GemmRequest q{};
              const int es = (int)v[1];
              q.epi = es & 0xff, q.sel = (es >> 8) & 0xf, q.in_tm = es & GEMM_IN_TM, q.out_tm = es & GEMM_OUT_TM;
              q.M = (int)m, q.N = (int)n, q.K = (int)k, q.ldo = !v[3] && v[6] == EPI_GLU_F16 ? (int)n / 2 : (int)n, q.has_bias = v[2] != 0;
              q.ksplit = v[3] ? (int)v[3] : 1, q.slab_f16 = v[4] == 1, q.splitk = v[3] != 0;
              std::vector<long long> exp{0};
              if (w) {
                if (w > (long long)answers.size()) return 2;
                exp = answers[w - 1];
                exp.insert(exp.begin() + 1, v[6]);
              }
              ok = route_fields(q, env) == exp;
            }
            ++ncases;
            if (!ok && ++bad <= 10) fprintf(stderr, "MISMATCH at m=%lld n=%lld k=%lld of %.60s...\n", m, n, k, line.data());
          }
      continue;
    }
    if (v.size() < 16) return 2;
    GemmEnv env{(int)v[12], 0, 1, 1, 0, 128, 96, 1, 128, 1, 2};  // the defaults of gemm_env()
    if (v[13] >= 0) {
      int* slot[] = {&env.dec_m160, &env.g2v2, &env.g2v2_min, &env.g2_auto_min, &env.g2_raster, &env.g2_splitk_min, &env.lone, &env.lone16,
                     &env.lone_ks};
      *slot[order[v[13]]] = (int)v[14];
    }
    std::vector<long long> got;
    if (v[0] == 1) {
      got.push_back(gemm_splitk_parts((int)v[2], (int)v[3], (int)v[4], (int)v[10], env));
    } else {
      GemmRequest q{};
      const int es = (int)v[1];
      q.epi = es & 0xff, q.sel = (es >> 8) & 0xf, q.in_tm = es & GEMM_IN_TM, q.out_tm = es & GEMM_OUT_TM;
      q.M = (int)v[2], q.N = (int)v[3], q.K = (int)v[4], q.ldo = (int)v[5], q.has_bias = v[6] != 0;
      q.fold = (int)v[7], q.fold_nparts = (int)v[8], q.fold_has_c1 = v[7] >= FOLD_CONSUMER_EXACT, q.stats = (int)v[9];
      q.ksplit = v[10] ? (int)v[10] : 1, q.slab_f16 = v[11] == 1, q.splitk = v[10] != 0;
      got = route_fields(q, env);
    }
    ++ncases;
    if (got != std::vector<long long>(v.begin() + 15, v.end())) {
      if (++bad <= 10) fprintf(stderr, "MISMATCH %s", line.data());
    }
  }
  fclose(f);
  // synthetic: 57 row tiles (the last m-group, owned by XCD 7, has one tile: 7 of every 8 of its slots are skipped) x 16 column tiles
  for (int raster = 1; raster <= 2; ++raster)
    for (int grid : {256, 240, 64})
      for (int parts = 0; parts < 2; ++parts) {
        ++nwalks;
        if (!walk_ok(57, 16, 1, raster, grid, parts != 0, false)) ++bad_walks;
      }
  printf("%ld cases, %ld mismatches; %ld walks, %ld bad\n", ncases, bad, nwalks, bad_walks);
  return bad || !ncases || bad_walks || !nwalks ? 1 : 0;
}
