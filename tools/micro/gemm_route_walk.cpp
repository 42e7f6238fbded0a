// Stand-alone host walk of the GEMM router over the recorded table:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I sonar_amd/csrc tools/micro/gemm_route_walk.cpp -o route_walk
//   ./route_walk tests/golden/gemm_routes.json
// Fills GemmRequest / GemmEnv directly (no library, no HIP), calls gemm_route / gemm_splitk_parts for every case line and compares
// with the recorded answer.  Exit status 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gemm_route.hpp"

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

static std::vector<long long> route_fields(const GemmRequest& q, const GemmEnv& env) {
  const GemmRoute r = gemm_route(q, env);
  if (r.engine == GEMM_NONE) return {0};
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
  printf("%ld cases, %ld mismatches\n", ncases, bad);
  return bad || !ncases ? 1 : 0;
}
