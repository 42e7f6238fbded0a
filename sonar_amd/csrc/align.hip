// Dynamic time warping over the cosine-distance matrix of two row sequences, for a ragged batch of document pairs
// (the contract is restated loop for loop in tests/alignment_ref.py).
//
//   D[0][0] = c[0][0];  D[i][j] = fl32(min(D[i-1][j], D[i][j-1], D[i-1][j-1]) + c[i][j])
// over the predecessors that exist and are admissible, ties to the first of up, left, diagonal.  radius r >= 1 admits
// cell (i, j) iff |i (ny-1) - j (nx-1)| <= r max(nx-1, ny-1, 1).
//
// Kernels, all batched over the pairs of the offset arrays:
//   dtw_plan_kernel       per-pair offsets into the workspace sections and the path (prefix sums over the device offsets)
//   dtw_cost_kernel       c = 1 - x . y from normalised fp16 rows, fp32 FMA chain in ascending k, 64 x 64 tile per block
//   dtw_skew_kernel       row-major cost -> the wavefront layout skew[strip][s][t] = c[64 strip + t][s - t]
//   dtw_dp_kernel         one workgroup per pair, one wave per 64-row strip: lane t owns row 64 strip + t and handles column
//                         s - t at step s.  Up and diagonal come from lane t-1 by one DPP wave shift per step, left is the
//                         lane's own register; lane 0 takes them from the previous strip's bottom row (a line of ny floats in
//                         global memory, handed on between the waves of the workgroup).  The 2-bit direction codes are packed
//                         16 steps per dword and stored as codes[strip][s / 16][t]: one 256-byte store per wave per 16 steps.
//   dtw_backtrack_kernel  one wave per pair walks the codes from (nx-1, ny-1) to (0, 0): a 256-byte line of code words covers
//                         16 steps of all 64 rows of a strip, so the wave loads it once and walks inside it by readlane.
// D is never stored: only the codes, the line and the lanes' registers.
//
// Waves of the DP workgroup run in ticks of one phase (64 steps, phase a = steps 64a .. 64a+63 of the strip) between two
// barriers.  Column j of a strip's bottom row is written at step j + 63, i.e. in phase <= j / 64 + 1, and read by the next
// strip at step j: a strip may run phase a once its predecessor has completed phase a + 1 (or all of its phases).  The line is
// used in place: a strip reads column j before it overwrites it, and its successor reads it only after that.
#include <algorithm>

#include "api_common.hpp"
#include "common.hpp"

namespace smi {

namespace {

constexpr int DW = 8;        // waves (strips in flight) per DP workgroup
constexpr int DT = DW * 64;  // its threads
constexpr int CT = 64;       // cost tile edge
constexpr int CK = 32;       // k slice of the cost kernel
constexpr int CS = CK + 4;   // LDS row stride in floats: 16-byte aligned rows, 16 rows x 4 dwords cover the 64 banks once
constexpr int NONE = 3;      // direction code of a cell without predecessor (the origin); 0 up, 1 left, 2 diagonal

__device__ __forceinline__ float inf() { return __uint_as_float(0x7f800000u); }

// DPP wave shifts across all 64 lanes (GFX9): lane i takes src of lane i - 1 (shr) / i + 1 (shl); the lane without a
// source (0 / 63) keeps `old`.
__device__ __forceinline__ float wave_shr1(float old, float src) {
  return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp((int)__float_as_uint(old), (int)__float_as_uint(src), 0x138,
                                                                0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float old, float src) {
  return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp((int)__float_as_uint(old), (int)__float_as_uint(src), 0x130,
                                                                0xf, 0xf, false));
}

// band half-width in units of the cross product; < 0: full matrix.  radius >= max(nx-1, ny-1, 1) admits every cell
// (|i (ny-1) - j (nx-1)| <= (nx-1)(ny-1)), so the product below stays under 2^62.
__device__ __forceinline__ int64_t band_width(int64_t nx, int64_t ny, int64_t radius) {
  const int64_t m = max(max(nx - 1, ny - 1), (int64_t)1);
  return radius <= 0 || radius >= m ? -1 : radius * m;
}

// admissible columns [lo, hi] of row i; lo > hi for a row outside the matrix
__device__ __forceinline__ void row_range(int64_t i, int64_t nx, int64_t ny, int64_t W, int& lo, int& hi) {
  if (i < 0 || i >= nx) {
    lo = 1;
    hi = 0;
  } else if (W < 0 || nx == 1) {
    lo = 0;
    hi = (int)(ny - 1);
  } else {
    const int64_t a = i * (ny - 1), q = nx - 1;
    lo = a - W <= 0 ? 0 : (int)((a - W + q - 1) / q);
    hi = (int)min((a + W) / q, ny - 1);
  }
}

// plan[4 b ..]: offsets of pair b into the row-major cost, the skewed cost, the code words and the path entries
__global__ __launch_bounds__(256) void dtw_plan_kernel(const int64_t* __restrict__ xoff, const int64_t* __restrict__ yoff,
                                                       int B, int64_t* __restrict__ plan) {
  __shared__ int64_t part[4][256];
  const int per = (B + 255) / 256;
  const int lo = min(per * (int)threadIdx.x, B), hi = min(lo + per, B);
  int64_t sum[4] = {0, 0, 0, 0};
  for (int pass = 0; pass < 2; ++pass) {
    for (int b = lo; b < hi; ++b) {
      const int64_t nx = xoff[b + 1] - xoff[b], ny = yoff[b + 1] - yoff[b];
      if (pass)
        for (int q = 0; q < 4; ++q) plan[4 * (int64_t)b + q] = sum[q];
      if (nx <= 0 || ny <= 0) continue;
      sum[0] += nx * ny;
      sum[1] += dtw_strips(nx) * dtw_steps(ny) * 64;
      sum[2] += dtw_strips(nx) * (dtw_steps(ny) / 16) * 64;
      sum[3] += nx + ny - 1;
    }
    if (pass) break;
    for (int q = 0; q < 4; ++q) part[q][threadIdx.x] = sum[q];
    __syncthreads();
    for (int q = 0; q < 4; ++q) {
      sum[q] = 0;
      for (int i = 0; i < (int)threadIdx.x; ++i) sum[q] += part[q][i];
    }
  }
}

// c[i][j] = 1 - sum_k x[i][k] y[j][k]: one FMA chain per cell in ascending k (the fp16 products are exact in fp32), whatever
// the pair's place in the batch.  Thread (tx, ty) owns rows ty + 16 r and columns tx + 16 c of the tile.
__global__ __launch_bounds__(256) void dtw_cost_kernel(const f16* __restrict__ xn, const f16* __restrict__ yn, int d,
                                                       const int64_t* __restrict__ xoff, const int64_t* __restrict__ yoff,
                                                       const int64_t* __restrict__ plan, float* __restrict__ cost) {
  __shared__ __attribute__((aligned(16))) float xs[CT * CS];
  __shared__ __attribute__((aligned(16))) float ys[CT * CS];
  const int b = blockIdx.y;
  const int64_t nx = xoff[b + 1] - xoff[b], ny = yoff[b + 1] - yoff[b];
  if (nx <= 0 || ny <= 0) return;
  const int64_t tiles_j = (ny + CT - 1) / CT;
  const int64_t i0 = (int64_t)(blockIdx.x / tiles_j) * CT, j0 = (int64_t)(blockIdx.x % tiles_j) * CT;
  if (i0 >= nx) return;
  const f16* xb = xn + xoff[b] * d;
  const f16* yb = yn + yoff[b] * d;
  const int tid = threadIdx.x, lr = tid >> 2, lc = (tid & 3) * 8, tx = tid & 15, ty = tid >> 4;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int k0 = 0; k0 < d; k0 += CK) {
    half8 xv = {0, 0, 0, 0, 0, 0, 0, 0}, yv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i0 + lr < nx) xv = *(const half8*)(xb + (i0 + lr) * d + k0 + lc);
    if (j0 + lr < ny) yv = *(const half8*)(yb + (j0 + lr) * d + k0 + lc);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xs[lr * CS + lc + e] = (float)xv[e];
      ys[lr * CS + lc + e] = (float)yv[e];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < CK; kk += 4) {
      f32x4 a[4], w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = *(const f32x4*)(xs + (ty + 16 * r) * CS + kk);
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = *(const f32x4*)(ys + (tx + 16 * c) * CS + kk);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_fmaf(a[r][e], w[c][e], acc[r][c]);
    }
  }
  float* out = cost + plan[4 * (int64_t)b];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + ty + 16 * r;
    if (i >= nx) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = j0 + tx + 16 * c;
      if (j < ny) out[i * ny + j] = 1.0f - acc[r][c];
    }
  }
}

// skew[strip][s][t] = c[64 strip + t][s - t], +inf where that cell does not exist.  Block = 4 steps x 64 lanes.
__global__ __launch_bounds__(256) void dtw_skew_kernel(const float* __restrict__ cost, const int64_t* __restrict__ xoff,
                                                       const int64_t* __restrict__ yoff, const int64_t* __restrict__ plan,
                                                       float* __restrict__ skew) {
  const int b = blockIdx.y;
  const int64_t nx = xoff[b + 1] - xoff[b], ny = yoff[b + 1] - yoff[b];
  if (nx <= 0 || ny <= 0) return;
  const int64_t S = dtw_steps(ny);
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // strip * S + s
  if (unit >= dtw_strips(nx) * S) return;
  const int t = threadIdx.x & 63;
  const int64_t i = unit / S * 64 + t, j = unit % S - t;
  float v = inf();
  if (i < nx && j >= 0 && j < ny) v = cost[plan[4 * (int64_t)b] + i * ny + j];
  skew[plan[4 * (int64_t)b + 1] + unit * 64 + t] = v;
}

__global__ __launch_bounds__(DT) void dtw_dp_kernel(const int64_t* __restrict__ xoff, const int64_t* __restrict__ yoff,
                                                    const int64_t* __restrict__ plan, int64_t radius,
                                                    const float* __restrict__ skew, uint32_t* __restrict__ codes,
                                                    float* line, float* __restrict__ distance) {
  __shared__ int st_strip[DW], st_next[DW], n_done;
  const int b = blockIdx.x;
  const int64_t nx = xoff[b + 1] - xoff[b], ny = yoff[b + 1] - yoff[b];
  if (nx <= 0 || ny <= 0) return;  // the backtrack kernel reports the empty pair
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, pw = (w + DW - 1) % DW;
  const int nstrips = (int)dtw_strips(nx);
  const int64_t S = dtw_steps(ny), G = S / 16;
  const int64_t W = band_width(nx, ny, radius);
  const float* sk = skew + plan[4 * (int64_t)b + 1];
  uint32_t* cd = codes + plan[4 * (int64_t)b + 2];
  float* ln = line + (yoff[b] - yoff[0]);
  if (lane == 0) {
    st_strip[w] = w;
    st_next[w] = 0;
  }
  if (threadIdx.x == 0) n_done = max(DW - nstrips, 0);

  int k = w;                         // this wave's strip
  bool fresh = true, first = true;   // strip k not set up yet / its first phase not run yet
  int a = 0, a_hi = 0, s_lo = 0, s_hi = 0, jlo = 1, jhi = 0, plo = 1, phi = 0;
  float cur = inf(), diag = inf();
  for (;;) {
    __syncthreads();  // the states and line columns of the last tick are visible
    const int ps = __builtin_amdgcn_readfirstlane(st_strip[pw]), pn = __builtin_amdgcn_readfirstlane(st_next[pw]);
    const int nd = __builtin_amdgcn_readfirstlane(n_done);
    __syncthreads();  // everybody has read them
    if (nd == DW) break;
    if (k >= nstrips) continue;
    if (fresh) {
      const int64_t r0 = (int64_t)k * 64;
      row_range(r0 + lane, nx, ny, W, jlo, jhi);
      row_range(r0 + lane - 1, nx, ny, W, plo, phi);
      int lo0, hi0, lo1, hi1;
      const int tl = (int)(min(r0 + 63, nx - 1) - r0);
      row_range(r0, nx, ny, W, lo0, hi0);
      row_range(r0 + tl, nx, ny, W, lo1, hi1);
      s_lo = lo0;
      s_hi = hi1 + tl;
      a = s_lo >> 6;
      a_hi = s_hi >> 6;
      cur = diag = inf();
      fresh = false;
    }
    if (k > 0 && !(ps > k - 1 || (ps == k - 1 && pn >= a + 2))) continue;

    // ---- phase a of strip k: groups of 16 steps
    const int64_t r = (int64_t)k * 64 + lane;
    const int g0 = max(4 * a, s_lo >> 4), g1 = min(4 * a + 3, s_hi >> 4);
    float bvec = inf();  // lane l: column 16 g0 + l of the previous strip's bottom row; shifted down one lane per step
    if (k > 0) {
      const int64_t col = (int64_t)16 * g0 + lane;
      if (col < ny) bvec = ln[col];
      if (first && lane == 0 && g0 > 0) diag = ln[16 * g0 - 1];
    }
    first = false;
    const float* skp = sk + (int64_t)k * S * 64 + lane;
    uint32_t* cdp = cd + (int64_t)k * G * 64 + lane;
    float cs[16], nxt[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) cs[u] = skp[((int64_t)g0 * 16 + u) * 64];
    for (int g = g0; g <= g1; ++g) {
      const int64_t gn = min((int64_t)g + 1, G - 1);
#pragma unroll
      for (int u = 0; u < 16; ++u) nxt[u] = skp[(gn * 16 + u) * 64];
      uint32_t word = 0;
      float ovec = 0.f;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int j = 16 * g + u - lane;
        const float up = wave_shr1(bvec, cur);  // lane 0: the line
        bvec = wave_shl1(bvec, bvec);
        const float left = cur;
        const bool up_ok = j >= plo && j <= phi, dg_ok = j - 1 >= plo && j - 1 <= phi, lf_ok = j - 1 >= jlo;
        float best = inf();
        uint32_t code = NONE;
        if (up_ok) {
          best = up;
          code = 0;
        }
        if (lf_ok && (code == NONE || left < best)) {
          best = left;
          code = 1;
        }
        if (dg_ok && (code == NONE || diag < best)) {
          best = diag;
          code = 2;
        }
        const float v = (r == 0 && j == 0) ? cs[u] : best + cs[u];
        if (j >= jlo && j <= jhi) {
          cur = v;
          word |= code << (2 * u);
          if (r == nx - 1 && j == ny - 1) distance[b] = v;
        }
        diag = up;
        ovec = wave_shl1(cur, ovec);  // lane 63 takes its cur, lane 48 + u' ends up with step u' of this group
      }
      cdp[(int64_t)g * 64] = word;
      if (k < nstrips - 1 && lane >= 48) {
        const int64_t col = (int64_t)16 * g - 63 + (lane - 48);
        if (col >= 0 && col < ny) ln[col] = ovec;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) cs[u] = nxt[u];
    }
    if (++a > a_hi) {
      k += DW;
      fresh = first = true;
      a = 0;
      if (k >= nstrips && lane == 0) atomicAdd(&n_done, 1);
    }
    if (lane == 0) {
      st_strip[w] = k;
      st_next[w] = a;
    }
  }
}

// One wave per pair.  Writes the path backwards from the end of the pair's nx + ny - 1 entries, then moves it to the front.
__global__ __launch_bounds__(64) void dtw_backtrack_kernel(const int64_t* __restrict__ xoff, const int64_t* __restrict__ yoff,
                                                           const int64_t* __restrict__ plan,
                                                           const uint32_t* __restrict__ codes, int2* path,
                                                           int32_t* __restrict__ path_len, float* __restrict__ distance) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t nx = xoff[b + 1] - xoff[b], ny = yoff[b + 1] - yoff[b];
  if (nx <= 0 || ny <= 0) {
    if (lane == 0) {
      path_len[b] = 0;
      distance[b] = inf();
    }
    return;
  }
  const int64_t cap = nx + ny - 1, G = dtw_steps(ny) / 16;
  const uint32_t* cd = codes + plan[4 * (int64_t)b + 2];
  int2* out = path + plan[4 * (int64_t)b + 3];
  int64_t i = nx - 1, j = ny - 1, n = 0;
  bool done = false;
  while (!done) {
    const int64_t strip = i >> 6, g = (j + (i & 63)) >> 4;
    const uint32_t word = cd[(strip * G + g) * 64 + lane];  // 16 steps of the strip's 64 rows
    for (;;) {
      if (lane == 0) out[cap - 1 - n] = make_int2((int)i, (int)j);
      ++n;
      const int t = (int)(i & 63), s = (int)(j + t);
      const uint32_t code = ((uint32_t)__builtin_amdgcn_readlane((int)word, t) >> (2 * (s & 15))) & 3u;
      if ((i == 0 && j == 0) || code == NONE || n >= cap) {
        done = true;
        break;
      }
      if (code != 1) --i;
      if (code != 0) --j;
      if (i < 0 || j < 0) {  // no computed cell points outside the matrix; never walk out of the buffers
        done = true;
        break;
      }
      if ((i >> 6) != strip || ((j + (i & 63)) >> 4) != g) break;
    }
  }
  __syncthreads();  // lane 0's entries are visible to the wave
  const int64_t shift = cap - n;
  if (shift > 0) {
    for (int64_t p0 = 0; p0 < n; p0 += 64) {
      const int64_t p = p0 + lane;
      int2 v = make_int2(0, 0);
      if (p < n) v = out[p + shift];
      __syncthreads();
      if (p < n) out[p] = v;
    }
  }
  if (lane == 0) path_len[b] = (int32_t)n;
}

// workspace: plan int64 [4 B] | line fp32 [sum ny] | codes u32 | skewed cost fp32 | row-major cost fp32 (smi_dtw_align only)
struct DtwWs : smi_host::WsLayout {
  int64_t* plan;
  float *line, *skew, *cost;
  uint32_t* codes;
  DtwWs(void* ws, int n_pairs, const DtwSizes& sz, bool with_cost) : smi_host::WsLayout(ws) {
    plan = take<int64_t>(4 * (size_t)n_pairs);
    line = take<float>(sz.line);
    codes = take<uint32_t>(sz.codes);
    skew = take<float>(sz.skew);
    cost = take<float>(with_cost ? sz.cells : 0);
  }
};

}  // namespace

size_t dtw_workspace_bytes(int n_pairs, const DtwSizes& sz, bool with_cost) {
  return DtwWs(nullptr, n_pairs, sz, with_cost).bytes();
}

hipError_t launch_dtw(const f16* xn, const f16* yn, int d, const float* cost, int n_pairs, const DtwSizes& sz,
                      const int64_t* xoff, const int64_t* yoff, int64_t radius, int32_t* path, int32_t* path_len,
                      float* distance, void* ws, hipStream_t stream) {
  const DtwWs w(ws, n_pairs, sz, !cost);
  hipLaunchKernelGGL(dtw_plan_kernel, dim3(1), dim3(256), 0, stream, xoff, yoff, n_pairs, w.plan);
  if (sz.cells > 0) {
    if (!cost) {
      hipLaunchKernelGGL(dtw_cost_kernel, dim3((unsigned)sz.max_tiles, (unsigned)n_pairs), dim3(256), 0, stream, xn, yn, d,
                         xoff, yoff, w.plan, w.cost);
      cost = w.cost;
    }
    hipLaunchKernelGGL(dtw_skew_kernel, dim3((unsigned)((sz.max_units + 3) / 4), (unsigned)n_pairs), dim3(256), 0, stream,
                       cost, xoff, yoff, w.plan, w.skew);
    hipLaunchKernelGGL(dtw_dp_kernel, dim3((unsigned)n_pairs), dim3(DT), 0, stream, xoff, yoff, w.plan, radius, w.skew, w.codes,
                       w.line, distance);
  }
  hipLaunchKernelGGL(dtw_backtrack_kernel, dim3((unsigned)n_pairs), dim3(64), 0, stream, xoff, yoff, w.plan, w.codes,
                     (int2*)path, path_len, distance);
  return hipGetLastError();
}

}  // namespace smi
