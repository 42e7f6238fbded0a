// Device side of the EmbeddingToText hot path: one incremental decoder step and the
// beam-search bookkeeping, all on the GPU (no host round trip per step, no KV-cache copy).
//
// Reference behaviour restated here:
//  * decoder frontend / layer / final LN / tied projection:
//      sonar/models/sonar_text/factory.py:229-315, sonar/nn/conditional_decoder_model.py:66-94
//  * the sentence embedding is a length-1 encoder output
//      (sonar/models/sonar_translation/model.py:48-53): the cross-attention softmax is 1,
//      so cross_attn(x) = W_o (W_v e + b_v) + b_o, a per-sentence per-layer constant that is
//      precomputed once per generate() call (the reference recomputes q/k/softmax every step);
//  * beam search: fairseq2 ~=0.4 BeamSearchSeq2SeqGenerator + StandardBeamSearchAlgorithm
//      (SURVEY a24): fp32 log-softmax, PAD never, EOS blocked below min length and forced at
//      max length, top-(2*beam) over beam x vocab, EOS candidates among the first `beam`
//      finish (score / (len-1)^len_penalty), the rest continue.
//
// Beam re-indexing: every step's fused q|k|v GEMM output IS the cache slab of that position
// (kv[layer][pos][row][3d]); a hypothesis is an ancestry table anc[row][pos] -> row slot that
// produced that position.  Reordering beams copies 4 B per (row, pos) instead of 4 KB per
// (row, pos, layer) -- fairseq2's index_select on the whole cache is ~7 GB/step at t = 64.
#include <cstdlib>

#include "common.hpp"
#include <type_traits>

#include "kernels.hpp"
#include "ln_core.hpp"
#include "step_proc.hpp"
#include "topk_order.hpp"

namespace smi {

// ------------------------------------------------------------- embed one position
// x[r,:] = E[tok[r]] * scale + PE[pos + off]; one wave per row.
__global__ __launch_bounds__(256) void dec_embed_kernel(const int32_t* __restrict__ tok,
                                                        const f16* __restrict__ table,
                                                        const float* __restrict__ pe_row, float scale,
                                                        float* __restrict__ x, int rows, int d,
                                                        int64_t vocab) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  int64_t t = tok[r];
  t = t < 0 ? 0 : (t >= vocab ? vocab - 1 : t);
  const f16* e = table + (size_t)t * d;
  float* o = x + (size_t)r * d;
  for (int c = lane * 8; c < d; c += 512) {
    const half8 ev = *(const half8*)(e + c);
    const f32x4 p0 = *(const f32x4*)(pe_row + c);
    const f32x4 p1 = *(const f32x4*)(pe_row + c + 4);
    f32x4 o0, o1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o0[i] = (float)(f16)((float)ev[i] * scale) + p0[i];
      o1[i] = (float)(f16)((float)ev[i + 4] * scale) + p1[i];
    }
    *(f32x4*)(o + c) = o0;
    *(f32x4*)(o + c + 4) = o1;
  }
}

hipError_t launch_dec_embed(const int32_t* tok, const f16* table, const float* pe_row, float scale,
                            float* x, int rows, int d, int64_t vocab, hipStream_t stream) {
  hipLaunchKernelGGL(dec_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, tok, table, pe_row,
                     scale, x, rows, d, vocab);
  return hipGetLastError();
}

// ---------------------- x += sum_z parts[z] (+ c[row / group]); h = LN(x)  (fused)
// parts: split-K slabs of the preceding projection GEMM (fp32 [nparts][rows_pad][d]); c: the
// per-sentence cross-attention constant.  Either may be null.
__device__ unsigned g_prefetch_sink;  // never written in practice (common.hpp: prefetch_range)

// NP: the number of slabs when it is one of 0 / 1 / 2 / 4 / 8 (straight-line loads), -1: any number (rounds of ZB).
// PT: slab element type (float, or f16: an fp16 model's split-K projections store fp16 partials; the sum is formed in fp32).
template <int NV, typename XT, int NP, typename PT>
__global__ __launch_bounds__(256) void sum_ln_kernel(XT* __restrict__ x, const PT* __restrict__ parts,
                                                     int nparts, size_t part_stride,
                                                     const float* __restrict__ c, int group,
                                                     const float* __restrict__ w,
                                                     const float* __restrict__ b, float eps,
                                                     f16* __restrict__ h, int rows, int h_tm,
                                                     const void* __restrict__ pf, size_t pf_bytes, int main_blocks) {
  constexpr int D = NV * 256;
  if ((int)blockIdx.x >= main_blocks) {  // surplus workgroups: weight prefetch for a later GEMM (common.hpp)
    prefetch_range(pf, pf_bytes, blockIdx.x - main_blocks, gridDim.x - main_blocks, &g_prefetch_sink);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  XT* xr = x + (size_t)r * D;
  // The kernel is one dependent chain per wave (loads -> two wave reductions -> store) at ~1 wave per SIMD, so EVERY
  // load -- the row, the constant, the slabs, the LayerNorm weights -- is issued before the first use of any of them
  // and without a branch in between: one memory round trip instead of three (round 4: the fp16 -> fp32 conversion
  // of the row used to sit in front of the slab loads, the slab loads were separated by wave-uniform branches and the
  // weights were fetched after the reductions; r04 experiment 12).  The constant is read through a pointer that
  // falls back to a valid address and zeroed by a select.
  // The summation order (x, slabs ascending, constant) is fixed.  XT = f16: the residual stream is fp16 (the text
  // encoder's small-batch path): fp32 adds, ONE rounding when the row is written back; LayerNorm sees the rounded row.
  typedef typename std::conditional<sizeof(XT) == 2, half4, f32x4>::type XV;
  XV xv[NV];
  f32x4 v[NV], cv[NV], wv[NV], bv[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) xv[k] = *(const XV*)(xr + k * 256 + lane * 4);
  const float* cp = c ? c + (size_t)(r / group) * D + lane * 4 : w + lane * 4;
#pragma unroll
  for (int k = 0; k < NV; ++k) cv[k] = *(const f32x4*)(cp + k * 256);
  const PT* pr = parts + (size_t)r * D + lane * 4;
  typedef typename std::conditional<sizeof(PT) == 2, half4, f32x4>::type PV;
  auto widen = [](const PV& v) {
    if constexpr (sizeof(PT) == 2)
      return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    else
      return v;
  };
  constexpr int NPC = NP > 0 ? NP : 1;
  PV p[NPC][NV];
  if constexpr (NP > 0) {
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int k = 0; k < NV; ++k) p[j][k] = *(const PV*)(pr + (size_t)j * part_stride + k * 256);
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    wv[k] = *(const f32x4*)(w + k * 256 + lane * 4);
    bv[k] = *(const f32x4*)(b + k * 256 + lane * 4);
  }
  // the machine scheduler would otherwise interleave loads and adds in a rolling window of two or three loads in flight
  // (it minimises registers: 74 instead of ~200) -- the opposite of what a latency chain wants
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if constexpr (sizeof(XT) == 2) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[k][i] = (float)xv[k][i];
    } else {
      v[k] = xv[k];
    }
    if (!c) cv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if constexpr (NP > 0) {
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int k = 0; k < NV; ++k) v[k] += widen(p[j][k]);
  } else if constexpr (NP < 0) {
    constexpr int ZB = NV <= 4 ? 8 : 4;  // slabs per round trip (register budget: ZB * NV f32x4)
    for (int z0 = 0; z0 < nparts; z0 += ZB) {
      f32x4 q[ZB][NV];
#pragma unroll
      for (int j = 0; j < ZB; ++j)
#pragma unroll
        for (int k = 0; k < NV; ++k)
          q[j][k] = z0 + j < nparts ? widen(*(const PV*)(pr + (size_t)(z0 + j) * part_stride + k * 256))
                                    : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < ZB; ++j)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += q[j][k];
    }
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    v[k] += cv[k];
    if constexpr (sizeof(XT) == 2) {
      half4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = (f16)v[k][i];
        v[k][i] = (float)o[i];
      }
      *(half4*)(xr + k * 256 + lane * 4) = o;
    } else {
      *(f32x4*)(xr + k * 256 + lane * 4) = v[k];
    }
    s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  }
  const float rstd = ln_center<4>(v, s, 1.0f / D, eps, wave_sum);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    half4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (f16)(v[k][i] * rstd * wv[k][i] + bv[k][i]);
    if (h_tm)  // tile-major GEMM operand (common.hpp): the FFN inner projection's X
      *(half4*)(h + tm_offset(r, k * 256 + lane * 4, D)) = o;
    else
      *(half4*)(h + (size_t)r * D + k * 256 + lane * 4) = o;
  }
}

template <int NV, typename XT, typename PT>
static void launch_sum_ln_np(int blocks, hipStream_t stream, XT* x, const PT* parts, int nparts, size_t part_stride,
                             const float* c, int group, const float* w, const float* b, float eps, f16* h, int rows,
                             int h_tm, const void* pf, size_t pf_bytes) {
  // surplus workgroups for the weight prefetch: one per CU the row work leaves idle
  const int cus = num_cus();  // gemm.hip: per-device, atomically cached (decode chains call this from several host threads)
  // ... when the row work takes at most a quarter of the chip (<= 256 rows: the surplus then streams a 16.8 MB matrix in
  // one round trip; at 512 rows the prefetch cost more than it saved)
  const int extra = pf && pf_bytes && blocks * 4 <= cus ? cus - blocks : 0;
  const int main_blocks = blocks;
#define SMI_SL(NP)                                                                                                     \
  hipLaunchKernelGGL((sum_ln_kernel<NV, XT, NP, PT>), dim3(blocks + extra), dim3(256), 0, stream, x, parts, nparts,    \
                     part_stride, c, group, w, b, eps, h, rows, h_tm, pf, pf_bytes, main_blocks)
  switch (nparts) {
    case 0: SMI_SL(0); break;
    case 1: SMI_SL(1); break;
    case 2: SMI_SL(2); break;
    case 4: SMI_SL(4); break;
    case 8:
      if constexpr (NV <= 4) {
        SMI_SL(8);
        break;
      }
      [[fallthrough]];
    default: SMI_SL(-1); break;
  }
#undef SMI_SL
}

hipError_t launch_sum_layernorm(void* x, const void* parts, int nparts, size_t part_stride,
                                const float* c, int group, const float* w, const float* b, float eps,
                                f16* h, int rows, int d, hipStream_t stream, int h_tm, int x_f16, const void* pf,
                                size_t pf_bytes, int parts_f16) {
  const int blocks = (rows + 3) / 4;
  if (!parts) nparts = 0;
  const bool known = dispatch_nv(d, [&](auto nv) {
    dispatch_f16(x_f16, [&](auto xt) {
      dispatch_f16(parts_f16, [&](auto pt) {
        using XT = decltype(xt);
        using PT = decltype(pt);
        launch_sum_ln_np<decltype(nv)::value, XT, PT>(blocks, stream, (XT*)x, (const PT*)parts, nparts, part_stride, c, group,
                                                      w, b, eps, h, rows, h_tm, pf, pf_bytes);
      });
    });
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

// -------------------------------------------------- single-query (decode) attention
// One wave per (row, head).  kv: [pos][rows_pad][3d] (q|k|v), anc: [rows][anc_stride].
// Lane (pg = lane>>3, c = lane&7) owns the 8 head dims c*8..c*8+7 of the positions j0 + 8*it + pg:
// every load instruction fetches 8 whole 128-B K (or V) rows as 16 B per lane, a score is joined
// across the 8 lanes of its position by 3 xor-shuffles, the softmax statistics across the 8 position
// groups by 3 more, and the probabilities never leave the lanes that multiply them into V.
// NG = 8-position groups per chunk (chunk = 8 NG positions), chosen by the launcher: the first chunk is rarely full at
// decode time, and a compile-time chunk size keeps the loop body straight-line (run-time skipping of masked groups
// was slower than loading them, r02 experiment 20).
template <int NG>
__global__ __launch_bounds__(256) void dec_attention_kernel(const f16* __restrict__ kv,
                                                            const int32_t* __restrict__ anc,
                                                            int anc_stride, f16* __restrict__ ctx,
                                                            int rows, int rows_pad, int d, int heads,
                                                            int pos, float sl2e) {
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= rows * heads) return;
  const int r = wid / heads, h = wid % heads;
  const int lane = threadIdx.x & 63, pg = lane >> 3, c = lane & 7;
  const size_t ld = (size_t)3 * d;
  const size_t slab = (size_t)rows_pad * ld;
  const half8 qh = *(const half8*)(kv + (size_t)pos * slab + (size_t)r * ld + h * 64 + c * 8);
  float q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = (float)qh[e] * sl2e;

  const int32_t* ar = anc + (size_t)r * anc_stride;
  const f16* kbase = kv + d + h * 64 + c * 8;
  float m = -1e30f, l = 0.f;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  for (int j0 = 0; j0 <= pos; j0 += 8 * NG) {
    float s[NG];
    // masked positions (j > pos) load ONE shared cached line (position 0, slot 0) in straight-line code: skipping
    // them per 8-position group (uniform branches) measured 4.38 against 4.26 ms per step (r02 experiment 20)
    const f16* row[NG];
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      const int j = j0 + it * 8 + pg;
      const bool valid = j <= pos;
      const int src = valid ? (j == pos ? r : ar[j]) : 0;
      row[it] = kbase + (size_t)(valid ? j : 0) * slab + (size_t)src * ld;
    }
    // all 8 K rows and all 8 V rows (the V row follows its K row at +d) are requested before the
    // first score is formed: one memory round trip per 64 positions instead of two
    half8 kr[NG], vr[NG];
#pragma unroll
    for (int it = 0; it < NG; ++it) kr[it] = *(const half8*)row[it];
#pragma unroll
    for (int it = 0; it < NG; ++it) vr[it] = *(const half8*)(row[it] + d);
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      const bool valid = j0 + it * 8 + pg <= pos;
      const half8 kk = kr[it];
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += q[e] * (float)kk[e];
      acc = sum_over_8(acc);
      s[it] = valid ? acc : -INFINITY;
    }
    float mx = s[0];
#pragma unroll
    for (int it = 1; it < NG; ++it) mx = fmaxf(mx, s[it]);
    mx = max_over_groups_of_8(mx);
    const float m_new = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    float ps = 0.f;
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      s[it] = __builtin_amdgcn_exp2f(s[it] - m_new);  // 0 for masked positions
      ps += s[it];
    }
    ps = sum_over_groups_of_8(ps);
    l = l * alpha + ps;
    m = m_new;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] *= alpha;
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      const half8 vv = vr[it];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += s[it] * (float)vv[e];
    }
  }
  half8 out;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = sum_over_groups_of_8(o[e]);
    out[e] = (f16)(v / l);
  }
  if (pg == 0) *(half8*)(ctx + (size_t)r * d + h * 64 + c * 8) = out;
}

hipError_t launch_dec_attention(const f16* kv, const int32_t* anc, int anc_stride, f16* ctx, int rows,
                                int rows_pad, int d, int heads, int pos, hipStream_t stream) {
  const float sl2e = 0.125f * 1.4426950408889634f;
  const int waves = rows * heads;
  const dim3 grid((waves + 3) / 4);
#define SMI_DA_LAUNCH(NG)                                                                                          \
  hipLaunchKernelGGL(dec_attention_kernel<NG>, grid, dim3(256), 0, stream, kv, anc, anc_stride, ctx, rows, rows_pad, \
                     d, heads, pos, sl2e)
  // as few passes as 64-position chunks would need (each pass is a dependent memory round trip), and the smallest
  // chunk that covers positions 0..pos in that many passes
  const int passes = pos / 64 + 1;
  const int ng = (pos / 8 + 1 + passes - 1) / passes;
  switch (ng) {
    case 1: SMI_DA_LAUNCH(1); break;
    case 2: SMI_DA_LAUNCH(2); break;
    case 3: SMI_DA_LAUNCH(3); break;
    case 4: SMI_DA_LAUNCH(4); break;
    case 5: SMI_DA_LAUNCH(5); break;
    case 6: SMI_DA_LAUNCH(6); break;
    case 7: SMI_DA_LAUNCH(7); break;
    default: SMI_DA_LAUNCH(8); break;
  }
#undef SMI_DA_LAUNCH
  return hipGetLastError();
}

// candidate ordering shared by the selection and the beam step: value desc, token asc (topk_order.hpp: better, xs_key)
constexpr int VS_K2MAX = 16;

// Wave-wide arg-best reduction of the selection kernels on DPP row operations + v_permlane16/32_swap (VALU rate) instead of
// __shfl_xor (= ds_bpermute, an LDS round trip per step and word: vocab_select ran 20 rounds x 12 of them back to back,
// the beam step ~420 per sentence).  Step order as wave_max (common.hpp): xor 1, xor 2, half-row mirror, row mirror, then the
// two lane swaps, whose both results are folded (one is the lane's own value, the other its partner's).  A lane holds N
// 32-bit words; first(a, b) says that a precedes b.  Every lane ends with the same winner: the orders are total.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int N, typename First>
__device__ __forceinline__ void wave_first(unsigned (&w)[N], First first) {
  auto fold = [&](const unsigned(&a)[N], const unsigned(&b)[N]) {  // w = first(a, b) ? a : b
    const bool fa = first(a, b);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const unsigned x = a[i], y = b[i];  // (selected as values: `fa ? a[i] : b[i]` selects an address, and went to scratch)
      w[i] = fa ? x : y;
    }
  };
  auto dpp = [&](auto ctrl) {
    unsigned o[N];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = dpp_u<decltype(ctrl)::value>(w[i]);
    fold(o, w);
  };
  auto swap = [&](auto wide) {
    unsigned a[N], b[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const auto r = decltype(wide)::value ? __builtin_amdgcn_permlane32_swap(w[i], w[i], false, false)
                                           : __builtin_amdgcn_permlane16_swap(w[i], w[i], false, false);
      a[i] = r[0];
      b[i] = r[1];
    }
    fold(b, a);
  };
  dpp(std::integral_constant<int, 0xB1>{});
  dpp(std::integral_constant<int, 0x4E>{});
  dpp(std::integral_constant<int, 0x141>{});
  dpp(std::integral_constant<int, 0x140>{});
  swap(std::false_type{});
  swap(std::true_type{});
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
  auto u64 = [](const unsigned(&w)[2]) { return ((unsigned long long)w[1] << 32) | w[0]; };
  unsigned w[2] = {(unsigned)k, (unsigned)(k >> 32)};
  wave_first(w, [&](const unsigned(&a)[2], const unsigned(&b)[2]) { return u64(a) > u64(b); });
  return u64(w);
}
// best (score desc, row asc, token asc) continuation of the wave, in every lane
__device__ __forceinline__ void wave_best3(float& bv, int& br, int& bt) {
  unsigned w[3] = {__float_as_uint(bv), (unsigned)br, (unsigned)bt};
  wave_first(w, [](const unsigned(&a)[3], const unsigned(&b)[3]) {
    const float va = __uint_as_float(a[0]), vb = __uint_as_float(b[0]);
    return va > vb || (va == vb && ((int)a[1] < (int)b[1] || (a[1] == b[1] && (int)a[2] < (int)b[2])));
  });
  bv = __uint_as_float(w[0]);
  br = (int)w[1];
  bt = (int)w[2];
}

// ------------------------------------------------- vocabulary select (per row, tile statistics)
// The logits GEMM leaves, per row and 256-column tile, the tile maximum and sum exp(v - max)
// (GemmTileStats).  One workgroup per row then
//  1. folds the tile statistics into the row's softmax normaliser (pmax, psum), and
//  2. finds the top-k2 candidates WITHOUT reading the whole logits row: the k2 best tiles by maximum
//     (ties: lower tile first) among tiles >= 1 contain every candidate that can reach the top-k2 --
//     each of them holds an element >= the k2-th best tile maximum, and an element of a later tile
//     loses every value tie against them (lower token wins).  Tile 0 is always read too: it holds the
//     tokens the generation masks touch (PAD, UNK penalty, blocked EOS), so its raw maximum says
//     nothing.  Thread t owns column t of every selected tile; k2 rounds of a workgroup-wide arg-max
//     over sortable (value desc, token asc) keys (xs_key; 0 = no candidate) produce the exact ordered list.
// The pieces below are shared by vocab_select_kernel and vocab_select_banned_kernel.
constexpr int VSEL_SLOTS = VS_K2MAX + 1;
constexpr int VSEL_TPT = 8;  // tiles per thread: up to 2048 tiles = 524288 tokens

// logits of (row, token): fp32 row-major [rows][ldl], or -- f16_tm -- fp16 in the tile-major layout of common.hpp with K = ldl
// (what the logits GEMM of an fp16 model stores, round 4)
__device__ __forceinline__ float logit_at(const float* __restrict__ logits, int ldl, int f16_tm, int row, int tok) {
  return f16_tm ? (float)((const f16*)logits)[tm_offset(row, tok, ldl)] : logits[(size_t)row * ldl + tok];
}

// step 1 of the selection: the row's softmax normaliser (pmax, psum) from its tile statistics; m[] = the thread's tile maxima
__device__ __forceinline__ void vsel_normaliser(const float* __restrict__ tile_max, const float* __restrict__ tile_sum,
                                                int ntiles, int stat_rows, float* __restrict__ pmax,
                                                float* __restrict__ psum, float (&m)[VSEL_TPT], float* s_f) {
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* tm = tile_max + row;  // [tile][stat_rows]
  const float* ts = tile_sum + row;
  constexpr int TPT = VSEL_TPT;
  float sm[TPT];
  float lm = -INFINITY;
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int t = tid + 256 * j;
    m[j] = t < ntiles ? tm[(size_t)t * stat_rows] : -INFINITY;
    sm[j] = t < ntiles ? ts[(size_t)t * stat_rows] : 0.f;
    lm = fmaxf(lm, m[j]);
  }
  // ---- 1. softmax normaliser of the row
  lm = wave_max(lm);
  if (lane == 0) s_f[wv] = lm;
  __syncthreads();
  const float M = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < TPT; ++j)
    if (m[j] != -INFINITY) se += sm[j] * __expf(m[j] - M);
  se = wave_sum(se);
  __syncthreads();
  if (lane == 0) s_f[wv] = se;
  __syncthreads();
  if (tid == 0) {
    pmax[row] = M;
    psum[row] = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
  }
}

// Does a row of sentence s select at step_nr?  TABLE (per-sentence prompts, PromptTableDev): the row's block_eos follows its
// own sentence's mode there, and a row whose sentence is forced (prompt token, forced EOS, past its cap) leaves after its
// normaliser, as a k2 = 0 launch does for every row.  A free row's candidates are formed exactly as without the table.
// (The k2 = 0 test stays in the kernels: inside this helper it cost vocab_select_kernel<true> 6 SGPRs and a wait.)
template <bool TABLE>
__device__ __forceinline__ bool vsel_row_free(const PromptTableDev& table, int s, int step_nr, int& block_eos) {
  if constexpr (TABLE) {
    const PromptRowMode md = prompt_row_mode(table, s, step_nr);
    if (!md.free_step) return false;
    block_eos = md.block_eos;
  }
  return true;
}

// The selections are rounds of "workgroup-wide maximum of a sortable key, then retire the winner".  The kernels are VALU-bound
// (1280 rows x 4 waves on 1024 SIMDs: a round used to rebuild and compare the keys of all of a thread's slots, ~230 VALU
// instructions, 20 rounds), so every thread keeps its keys and its current best: a round is one wave reduction of the
// per-thread bests, one LDS exchange behind ONE barrier (the wave results alternate between the two halves of slot, by the
// running round count `rounds`), and only the winner's thread rescans its slots.
__device__ __forceinline__ unsigned long long vsel_wg_max(unsigned long long mine, unsigned long long (*slot)[4], int& rounds) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long w = wave_max_u64(mine);
  unsigned long long* s = slot[rounds & 1];
  if (lane == 0) s[wv] = w;
  __syncthreads();
  unsigned long long b = s[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) b = s[q] > b ? s[q] : b;
  ++rounds;
  return b;
}
// The round's winner b leaves the slots of the thread that held it.  Keys are unique (the tile or token index is part of
// them): exactly one thread.
template <int N>
__device__ __forceinline__ void vsel_retire(unsigned long long (&k)[N], unsigned long long& best, unsigned long long b) {
  if (b == 0ull || b != best) return;
  best = 0ull;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const unsigned long long kj = k[j] == b ? 0ull : k[j];
    k[j] = kj;
    best = kj > best ? kj : best;
  }
}
// The k2 best tiles >= 1 (value desc, tile asc) that `skip` does not exclude, to sel[1..]; sel[0] = tile 0, which is taken
// unconditionally.  Returns the number of entries of sel; last = the key of the last tile taken.  The rounds end early with
// fewer than k2 such tiles: the caller's barrier before it reads sel is also what lines the workgroup up again.
template <typename Skip>
__device__ __forceinline__ int vsel_best_tiles(const float (&m)[VSEL_TPT], int k2, int* sel, unsigned long long (*slot)[4],
                                               int& rounds, unsigned long long& last, Skip skip) {
  const int tid = threadIdx.x;
  unsigned long long tk[VSEL_TPT];
  unsigned long long tbest = 0ull;
#pragma unroll
  for (int j = 0; j < VSEL_TPT; ++j) {
    const int t = tid + 256 * j;
    tk[j] = (m[j] != -INFINITY && t != 0 && !skip(t)) ? xs_key(m[j], t) : 0ull;
    tbest = tk[j] > tbest ? tk[j] : tbest;
  }
  if (tid == 0) sel[0] = 0;
  int nsel = 1;
  for (int round = 0; round < k2; ++round) {
    const unsigned long long b = vsel_wg_max(tbest, slot, rounds);
    if (b == 0ull) break;
    if (tid == 0) sel[nsel] = xs_key_index(b);
    ++nsel;
    last = b;
    vsel_retire(tk, tbest, b);
  }
  return nsel;
}
// A column's key from its logit under the generation masks: 0 for a token that is no candidate.
struct VselColumns {
  const float* __restrict__ logits;
  int ldl, f16_tm, vocab;
  float inv_temp;
  int pad_idx, eos_idx, unk_idx;
  float unk_penalty;
  int block_eos;
  __device__ __forceinline__ unsigned long long key(int row, int tok) const {
    if (tok >= vocab || tok == pad_idx || (block_eos && tok == eos_idx)) return 0ull;
    float v = logit_at(logits, ldl, f16_tm, row, tok) * inv_temp;
    if (tok == unk_idx) v -= unk_penalty;
    return v != -INFINITY ? xs_key(v, tok) : 0ull;
  }
};
// entry o of the ordered list: the candidate of key b, or (-inf, 0x7fffffff) for none
__device__ __forceinline__ void vsel_write(unsigned long long b, float* __restrict__ pval, int* __restrict__ pidx, size_t o) {
  pval[o] = b != 0ull ? xs_key_value(b) : -INFINITY;
  pidx[o] = b != 0ull ? xs_key_index(b) : 0x7fffffff;
}

template <bool TABLE>
__global__ __launch_bounds__(256) void vocab_select_kernel(const float* __restrict__ logits, int ldl, int f16_tm, int vocab,
                                                           const float* __restrict__ tile_max,
                                                           const float* __restrict__ tile_sum, int ntiles,
                                                           int stat_rows, int k2, float inv_temp, int pad_idx, int eos_idx, int unk_idx,
                                                           float unk_penalty, int block_eos,
                                                           float* __restrict__ pmax, float* __restrict__ psum,
                                                           float* __restrict__ pval, int* __restrict__ pidx,
                                                           PromptTableDev table, int group, int step_nr) {
  __shared__ float s_f[4];
  __shared__ int s_sel[VSEL_SLOTS];
  __shared__ unsigned long long s_k2[2][4];
  const int row = blockIdx.x, tid = threadIdx.x;
  float m[VSEL_TPT];
  vsel_normaliser(tile_max, tile_sum, ntiles, stat_rows, pmax, psum, m, s_f);
  if (k2 == 0) return;
  if (!vsel_row_free<TABLE>(table, row / group, step_nr, block_eos)) return;
  // ---- 2a. the k2 best tiles among tiles >= 1, plus tile 0
  int rounds = 0;
  unsigned long long last = 0ull;
  const int nsel = vsel_best_tiles(m, k2, s_sel, s_k2, rounds, last, [](int) { return false; });
  __syncthreads();  // s_sel is complete; also what makes an early end of the tile rounds safe
  // ---- 2b. thread t owns column t of every selected tile
  const VselColumns cols{logits, ldl, f16_tm, vocab, inv_temp, pad_idx, eos_idx, unk_idx, unk_penalty, block_eos};
  unsigned long long ck[VSEL_SLOTS];
  unsigned long long cbest = 0ull;
#pragma unroll
  for (int j = 0; j < VSEL_SLOTS; ++j) {
    ck[j] = j < nsel ? cols.key(row, s_sel[j] * 256 + tid) : 0ull;
    cbest = ck[j] > cbest ? ck[j] : cbest;
  }
  // ---- 2c. ordered top-k2 by k2 workgroup-wide arg-max rounds
  for (int round = 0; round < k2; ++round) {
    const unsigned long long b = vsel_wg_max(cbest, s_k2, rounds);
    if (tid == 0) vsel_write(b, pval, pidx, (size_t)row * VS_K2MAX + round);
    vsel_retire(ck, cbest, b);
  }
}

// ------------------------------------------------- vocabulary select under step processors (bans)
// As vocab_select_kernel, with the ids the row's step processors ban (step_proc.hpp) removed from the candidates; pmax /
// psum stay those of the untouched row (a ban is -inf AFTER log_softmax).  A banned id is usually its tile's maximum, so
// the tile argument changes: a tile holding a banned id ("dirty") says nothing through its raw maximum.  The candidates are
//   tile 0, the k2 best CLEAN tiles >= 1 (value desc, tile asc), and every dirty tile >= 1 whose raw maximum is >= the
//   k2-th of those (every dirty tile when fewer than k2 clean tiles exist);
// each of the k2 clean tiles holds an unbanned element >= that maximum which wins every value tie against a later tile, and
// a dirty tile below it holds nothing that can reach the top-k2.  Their number is not bounded, so the tiles are read in
// groups of VSEL_SLOTS, each group merged with the running top-k2 (an LDS list, one more slot per thread) by k2 rounds of
// the workgroup-wide arg-max; banned columns are skipped through a per-group 256-bit mask per tile.
constexpr int VSB_MAX_BANS = kStepProcMaxLen + kStepProcMaxBanned;

template <bool TABLE>
__global__ __launch_bounds__(256) void vocab_select_banned_kernel(
    const float* __restrict__ logits, int ldl, int f16_tm, int vocab, const float* __restrict__ tile_max,
    const float* __restrict__ tile_sum, int ntiles, int stat_rows, int k2, float inv_temp, int pad_idx, int eos_idx,
    int unk_idx, float unk_penalty, int block_eos, const int32_t* __restrict__ hist, int hist_stride, int hist_len,
    StepProcDev proc, float* __restrict__ pmax, float* __restrict__ psum, float* __restrict__ pval, int* __restrict__ pidx,
    PromptTableDev table, int group, int step_nr) {
  __shared__ float s_f[4];
  __shared__ int32_t s_seq[kStepProcMaxLen];
  __shared__ int32_t s_ban[VSB_MAX_BANS];
  __shared__ uint32_t s_dirty[2048 / 32];
  __shared__ int s_tiles[2048];              // candidate tiles: [0] tile 0, [1, nsel) the clean ones, then the dirty ones
  __shared__ short s_slot[2048];             // tile -> slot in the current group, -1 elsewhere
  __shared__ uint32_t s_mask[VSEL_SLOTS][8]; // banned columns of the group's tiles
  __shared__ unsigned long long s_top[VS_K2MAX];
  __shared__ unsigned long long s_k2[2][4];
  __shared__ int s_nban, s_ndirty;
  const int row = blockIdx.x, tid = threadIdx.x;
  constexpr int TPT = VSEL_TPT;
  float m[TPT];
  vsel_normaliser(tile_max, tile_sum, ntiles, stat_rows, pmax, psum, m, s_f);
  if (k2 == 0) return;
  if (!vsel_row_free<TABLE>(table, row / group, step_nr, block_eos)) return;
  // ---- B0. the row's sequence into LDS, empty ban list / dirty bitmap / slot map
  const int32_t* h = hist + (size_t)row * hist_stride;
  for (int i = tid; i < hist_len; i += 256) s_seq[i] = h[i];
  if (tid < 2048 / 32) s_dirty[tid] = 0u;
  for (int t = tid; t < 2048; t += 256) s_slot[t] = -1;
  if (tid < VS_K2MAX) s_top[tid] = 0ull;
  if (tid == 0) {
    s_nban = 0;
    s_ndirty = 0;
  }
  __syncthreads();
  // ---- B1. banned ids and dirty tiles
  step_proc_bans(proc, s_seq, hist_len, tid, 256, [&](int tok) {
    if (tok < 0 || tok >= vocab) return;
    const int k = atomicAdd(&s_nban, 1);
    if (k < VSB_MAX_BANS) s_ban[k] = tok;
    atomicOr(&s_dirty[tok >> 13], 1u << ((tok >> 8) & 31));
  });
  __syncthreads();
  const int nban = min(s_nban, VSB_MAX_BANS);
  auto dirty = [&](int t) { return (s_dirty[t >> 5] >> (t & 31)) & 1u; };
  // ---- B2. the k2 best clean tiles >= 1, and the k2-th one's maximum
  int rounds = 0;
  unsigned long long last = 0ull;
  const int nsel = vsel_best_tiles(m, k2, s_tiles, s_k2, rounds, last, dirty);
  // ---- B3. the dirty tiles that can hold a candidate
  const bool all_dirty = nsel - 1 < k2;
  const float thr = all_dirty ? -INFINITY : xs_key_value(last);
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int t = tid + 256 * j;
    if (t != 0 && t < ntiles && m[j] != -INFINITY && dirty(t) && (all_dirty || m[j] >= thr))
      s_tiles[nsel + atomicAdd(&s_ndirty, 1)] = t;
  }
  __syncthreads();
  const int ncand = nsel + s_ndirty;
  // ---- B4. groups of VSEL_SLOTS tiles, each merged with the running top-k2
  const VselColumns cols{logits, ldl, f16_tm, vocab, inv_temp, pad_idx, eos_idx, unk_idx, unk_penalty, block_eos};
  for (int g0 = 0; g0 < ncand; g0 += VSEL_SLOTS) {
    const int gn = min(VSEL_SLOTS, ncand - g0);
    if (tid < VSEL_SLOTS * 8) s_mask[tid >> 3][tid & 7] = 0u;
    if (tid < gn) s_slot[s_tiles[g0 + tid]] = (short)tid;
    __syncthreads();
    for (int k = tid; k < nban; k += 256) {
      const int b = s_ban[k], sl = s_slot[b >> 8];
      if (sl >= 0) atomicOr(&s_mask[sl][(b & 255) >> 5], 1u << (b & 31));
    }
    __syncthreads();
    unsigned long long ck[VSEL_SLOTS + 1];
    unsigned long long cbest = 0ull;
#pragma unroll
    for (int j = 0; j < VSEL_SLOTS; ++j) {
      ck[j] = 0ull;
      if (j < gn && !((s_mask[j][tid >> 5] >> (tid & 31)) & 1u)) ck[j] = cols.key(row, s_tiles[g0 + j] * 256 + tid);
      cbest = ck[j] > cbest ? ck[j] : cbest;
    }
    ck[VSEL_SLOTS] = tid < k2 ? s_top[tid] : 0ull;  // the running list takes part as one more slot
    cbest = ck[VSEL_SLOTS] > cbest ? ck[VSEL_SLOTS] : cbest;
    __syncthreads();  // every s_top read before the rounds rewrite it
    for (int round = 0; round < k2; ++round) {
      const unsigned long long b = vsel_wg_max(cbest, s_k2, rounds);
      if (tid == 0) s_top[round] = b;
      vsel_retire(ck, cbest, b);
    }
    if (tid < gn) s_slot[s_tiles[g0 + tid]] = -1;
    __syncthreads();
  }
  // ---- B5. the ordered list
  if (tid < k2) vsel_write(s_top[tid], pval, pidx, (size_t)row * VS_K2MAX + tid);
}

hipError_t launch_vocab_select(const VocabSelectArgs& a, hipStream_t stream) {
  if (a.rows <= 0 || a.stat_rows < a.rows || a.ntiles <= 0 || a.ntiles > 2048 || a.k2 < 0 || a.k2 > VS_K2MAX ||
      (int64_t)a.ntiles * 256 < a.vocab)
    return hipErrorInvalidValue;
  const bool table = a.table.tok != nullptr;
  if (table && (!a.table.len || a.group < 1)) return hipErrorInvalidValue;
  // without a table the kernels read no table argument: they get the empty one
  const PromptTableDev tab = table ? a.table : PromptTableDev{};
  const int group = table ? a.group : 1, step_nr = table ? a.step_nr : 0;
  if (a.hist && a.proc.active()) {
    const StepProcDev& proc = a.proc;
    if (a.hist_len < 1 || a.hist_len > kStepProcMaxLen || a.hist_stride < a.hist_len || proc.num_banned < 0 ||
        proc.num_banned > kStepProcMaxBanned || (proc.num_banned > 0 && (!proc.tokens || !proc.offsets)))
      return hipErrorInvalidValue;
    hipLaunchKernelGGL(table ? vocab_select_banned_kernel<true> : vocab_select_banned_kernel<false>, dim3(a.rows), dim3(256), 0,
                       stream, a.logits, a.ldl, a.f16_tm, a.vocab, a.tile_max, a.tile_sum, a.ntiles, a.stat_rows, a.k2, a.inv_temp,
                       a.pad_idx, a.eos_idx, a.unk_idx, a.unk_penalty, a.block_eos, a.hist, a.hist_stride, a.hist_len, proc,
                       a.pmax, a.psum, a.pval, a.pidx, tab, group, step_nr);
  } else {
    hipLaunchKernelGGL(table ? vocab_select_kernel<true> : vocab_select_kernel<false>, dim3(a.rows), dim3(256), 0, stream,
                       a.logits, a.ldl, a.f16_tm, a.vocab, a.tile_max, a.tile_sum, a.ntiles, a.stat_rows, a.k2, a.inv_temp,
                       a.pad_idx, a.eos_idx, a.unk_idx, a.unk_penalty, a.block_eos, a.pmax, a.psum, a.pval, a.pidx, tab, group,
                       step_nr);
  }
  return hipGetLastError();
}

// ----------------------------------------------------------------- beam step (per sentence)
// One workgroup (256 threads) per sentence.  Takes the ordered top-k2 list and the normaliser vocab_select left for each
// live row, forms the 2*beam best (row, token) continuations and applies the fairseq2 EOS rules.
struct BeamState {
  int32_t* tok;        // [R] token fed at the current position
  float* cum;          // [R] cumulative log-prob
  int32_t* nactive;    // [n] live rows of the sentence (1 until the first expansion)
  int32_t* done;       // [n]
  int32_t* ndone;      // [1]
  int32_t* parent;     // [R] out: parent row (global slot) of the row's next state
  int32_t* new_tok;    // [R] out
  float* new_cum;      // [R] out
  const int32_t* hist; // [R][hist_stride] tokens of every position <= pos
  int32_t* fin_tok;    // [n][beam][hist_stride]
  int32_t* fin_len;    // [n][beam]
  float* fin_score;    // [n][beam]
  int32_t* fin_count;  // [n]
  float* margins;      // [n][2] smallest decision gap so far: {step candidates (log-prob), final ranking}
};

// TABLE (per-sentence prompts): prompt_len, forced_tok and max_len are those of the workgroup's own sentence.
template <bool TABLE>
__global__ __launch_bounds__(256) void beam_step_kernel(BeamState st, const float* __restrict__ logits,
                                                        int ldl, int f16_tm, const float* __restrict__ pmax,
                                                        const float* __restrict__ psum,
                                                        const float* __restrict__ pval,
                                                        const int* __restrict__ pidx,
                                                        int beam, int k2, int pos, int prompt_len,
                                                        int forced_tok, int max_len, float inv_temp,
                                                        float len_penalty, int normalize, int eos_idx,
                                                        int hist_stride, PromptTableDev table) {
  __shared__ float s_lse[8];
  __shared__ float c_val[8 * VS_K2MAX];
  __shared__ int c_tok[8 * VS_K2MAX];
  __shared__ int c_row[8 * VS_K2MAX];
  __shared__ int f_row[8];
  __shared__ float f_score[8];
  __shared__ int f_n, f_base;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int base = s * beam;
  const int step_nr = pos + 1;  // index of the token chosen now
  if constexpr (TABLE) {
    const PromptRowMode md = prompt_row_mode(table, s, step_nr);
    prompt_len = md.plen;
    forced_tok = md.forced_tok;
    max_len = md.max_len;
  }
  if (st.done[s]) {  // keep the rows inert
    if (tid < beam) {
      st.parent[base + tid] = base + tid;
      st.new_tok[base + tid] = st.tok[base + tid];
      st.new_cum[base + tid] = st.cum[base + tid];
    }
    return;
  }
  const int na = st.nactive[s];
  // (1) log-sum-exp of every live row: pmax + log(psum) of the ONE normaliser entry vocab_select leaves per row.  (The
  // chunk-partial merge this replaces gave the same bits for one entry: the wave maximum over one lane's pmax and 63
  // -inf is pmax, the lane's term is psum * __expf(pmax - pmax) = psum * 1, and the wave sum adds 63 zeros to it.)
  if (tid < na) s_lse[tid] = pmax[base + tid] + __logf(psum[base + tid]);
  __syncthreads();

  const bool forced_prompt = step_nr < prompt_len;
  const bool force_eos = !forced_prompt && step_nr == max_len - 1;
  if (forced_prompt || force_eos) {
    // candidate of every live row is one given token
    if (tid < na) {
      const int tk = forced_prompt ? forced_tok : eos_idx;
      const float lp = logit_at(logits, ldl, f16_tm, base + tid, tk) * inv_temp - s_lse[tid];
      c_val[tid] = st.cum[base + tid] + lp;
      c_tok[tid] = tk;
      c_row[tid] = base + tid;
    }
    __syncthreads();
    if (tid == 0) {
      if (forced_prompt) {
        for (int r = 0; r < beam; ++r) {
          const bool live = r < na;
          st.parent[base + r] = base + r;
          st.new_tok[base + r] = live ? c_tok[r] : st.tok[base + r];
          st.new_cum[base + r] = live ? c_val[r] : st.cum[base + r];
        }
        f_n = 0;
      } else {
        // sort the <= beam EOS candidates by score (desc, row asc) and finish them all
        int order[8];
        for (int r = 0; r < na; ++r) order[r] = r;
        for (int a = 1; a < na; ++a)
          for (int b = a; b > 0 && better(c_val[order[b]], order[b], c_val[order[b - 1]], order[b - 1]); --b) {
            const int t = order[b];
            order[b] = order[b - 1];
            order[b - 1] = t;
          }
        int cnt = st.fin_count[s];
        f_base = cnt;
        int nf = 0;
        for (int a = 0; a < na && cnt < beam; ++a) {
          f_row[nf] = c_row[order[a]];
          f_score[nf] = c_val[order[a]];
          ++nf;
          ++cnt;
        }
        f_n = nf;
        st.fin_count[s] = cnt;
        st.done[s] = 1;  // nothing can continue past the maximum length
        atomicAdd(st.ndone, 1);
        for (int r = 0; r < beam; ++r) {
          st.parent[base + r] = base + r;
          st.new_tok[base + r] = st.tok[base + r];
          st.new_cum[base + r] = st.cum[base + r];
        }
      }
    }
  } else {
    // (2) per live row: the selection's ordered top-k2 list as cumulative log-probs.  One wave per row.
    for (int r = wv; r < na; r += 4) {
      const size_t o = (size_t)(base + r) * VS_K2MAX;
      if (lane < k2) {
        const float v = pval[o + lane];
        c_val[r * VS_K2MAX + lane] = v == -INFINITY ? -INFINITY : st.cum[base + r] + v - s_lse[r];
        c_tok[r * VS_K2MAX + lane] = pidx[o + lane];
        c_row[r * VS_K2MAX + lane] = base + r;
      }
    }
    __syncthreads();
    // (3) wave 0: overall top-k2 over the na*k2 row candidates (score desc, row asc, token asc),
    //     two candidates per lane; then thread 0 applies the EOS rules on the sorted list.
    __shared__ float t_val[VS_K2MAX];
    __shared__ int t_tok[VS_K2MAX], t_row[VS_K2MAX];
    __shared__ int t_n;
    if (wv == 0) {
      float v2[2];
      int r2[2], k2t[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int e = u * 64 + lane;  // candidate id = row * VS_K2MAX + rank
        const bool ok = e < na * VS_K2MAX && (e % VS_K2MAX) < k2;
        v2[u] = ok ? c_val[e] : -INFINITY;
        r2[u] = ok ? c_row[e] : 0x7fffffff;
        k2t[u] = ok ? c_tok[e] : 0x7fffffff;
      }
      int nsel = 0;
      for (int sel = 0; sel < k2; ++sel) {
        // lane-local best of its two, then wave arg-best
        int u = (v2[1] > v2[0] || (v2[1] == v2[0] && (r2[1] < r2[0] || (r2[1] == r2[0] && k2t[1] < k2t[0])))) ? 1 : 0;
        float bv = v2[u];
        int br = r2[u], bt = k2t[u];
        wave_best3(bv, br, bt);
        if (bv == -INFINITY) break;
        if (lane == 0) {
          t_val[sel] = bv;
          t_tok[sel] = bt;
          t_row[sel] = br;
        }
        ++nsel;
#pragma unroll
        for (int w = 0; w < 2; ++w)
          if (r2[w] == br && k2t[w] == bt) v2[w] = -INFINITY;
      }
      if (lane == 0) t_n = nsel;
    }
    __syncthreads();
    if (tid == 0) {
      const int nsel = t_n;
      const float* tv = t_val;
      const int* tt = t_tok;
      const int* tr = t_row;
      int cnt = st.fin_count[s];
      f_base = cnt;
      int nf = 0;
      bool finished_all = false;
      for (int i = 0; i < nsel && i < beam; ++i) {
        if (tt[i] == eos_idx) {
          f_row[nf] = tr[i];
          f_score[nf] = tv[i];
          ++nf;
          if (++cnt == beam) {
            finished_all = true;
            break;
          }
        }
      }
      f_n = nf;
      st.fin_count[s] = cnt;
      if (st.margins) {
        // decision margin of this step: the smallest gap between neighbours of the sorted candidate
        // list up to (and including) the first candidate that is NOT consumed.  For beam 1 this is
        // the greedy top-1 / top-2 log-prob margin.  A parity test may excuse a token mismatch
        // only where this measured margin is below its stated epsilon.
        int last = nsel - 1;
        if (finished_all) {  // nothing after the hypothesis that completed the beam matters
          int c2 = f_base;
          for (int i = 0; i < nsel && i < beam; ++i)
            if (tt[i] == eos_idx && ++c2 == beam) {
              last = i;
              break;
            }
        } else {
          int taken = 0;
          for (int i = 0; i < nsel; ++i) {
            if (tt[i] == eos_idx) continue;
            if (++taken == beam) {
              last = i;
              break;
            }
          }
        }
        float g = st.margins[2 * s];
        for (int i = 0; i <= last && i + 1 < nsel; ++i) g = fminf(g, tv[i] - tv[i + 1]);
        st.margins[2 * s] = g;
      }
      if (finished_all) {
        st.done[s] = 1;
        atomicAdd(st.ndone, 1);
        for (int r = 0; r < beam; ++r) {
          st.parent[base + r] = base + r;
          st.new_tok[base + r] = st.tok[base + r];
          st.new_cum[base + r] = st.cum[base + r];
        }
      } else {
        int w = 0;
        for (int i = 0; i < nsel && w < beam; ++i) {
          if (tt[i] == eos_idx) continue;
          st.parent[base + w] = tr[i];
          st.new_tok[base + w] = tt[i];
          st.new_cum[base + w] = tv[i];
          ++w;
        }
        st.nactive[s] = w;
        for (; w < beam; ++w) {  // unreachable with vocab > 2*beam; keep the slot inert
          st.parent[base + w] = base + w;
          st.new_tok[base + w] = st.tok[base + w];
          st.new_cum[base + w] = -INFINITY;
        }
      }
    }
  }
  __syncthreads();
  // (4) copy out the hypotheses that finished at this step: generated tokens + EOS
  const int nf = f_n;
  for (int f = 0; f < nf; ++f) {
    const int slot = f_base + f;
    const int row = f_row[f];
    const int glen = step_nr - prompt_len;  // generated tokens before the EOS
    int32_t* dst = st.fin_tok + ((size_t)s * beam + slot) * hist_stride;
    const int32_t* src = st.hist + (size_t)row * hist_stride + prompt_len;
    for (int i = tid; i < glen; i += 256) dst[i] = src[i];
    if (tid == 0) {
      dst[glen] = eos_idx;
      st.fin_len[s * beam + slot] = glen + 1;
      const float seq_len = (float)(step_nr + 1);
      st.fin_score[s * beam + slot] = normalize ? f_score[f] / __powf(seq_len - 1.f, len_penalty) : f_score[f];
    }
  }
}

hipError_t launch_beam_step(const BeamStepArgs& a, hipStream_t stream) {
  BeamState st{a.tok, a.cum, a.nactive, a.done, a.ndone, a.parent, a.new_tok, a.new_cum,
               a.hist, a.fin_tok, a.fin_len, a.fin_score, a.fin_count, a.margins};
  hipLaunchKernelGGL(a.table.tok ? beam_step_kernel<true> : beam_step_kernel<false>, dim3(a.n), dim3(256), 0, stream, st,
                     a.logits, a.ldl, a.logits_f16_tm, a.pmax, a.psum, a.pval, a.pidx, a.beam, a.k2, a.pos, a.prompt_len,
                     a.forced_tok, a.max_len, a.inv_temp, a.len_penalty, a.normalize, a.eos_idx, a.hist_stride, a.table);
  return hipGetLastError();
}

// ------------------------------------------------------------------------ beam reorder
// new_anc[r][j] = anc[parent[r]][j] (j < pos), new_anc[r][pos] = parent[r];
// new_hist[r][j] = hist[parent[r]][j] (j <= pos), new_hist[r][pos+1] = new_tok[r];
// tok/cum take their new values.
__global__ __launch_bounds__(256) void beam_reorder_kernel(const int32_t* __restrict__ parent,
                                                           const int32_t* __restrict__ new_tok,
                                                           const float* __restrict__ new_cum,
                                                           const int32_t* __restrict__ anc,
                                                           int32_t* __restrict__ anc2,
                                                           const int32_t* __restrict__ hist,
                                                           int32_t* __restrict__ hist2,
                                                           int32_t* __restrict__ tok,
                                                           float* __restrict__ cum, int stride,
                                                           int pos) {
  const int r = blockIdx.x;
  const int p = parent[r];
  for (int j = threadIdx.x; j <= pos; j += 256) {
    anc2[(size_t)r * stride + j] = j == pos ? p : anc[(size_t)p * stride + j];
    hist2[(size_t)r * stride + j] = hist[(size_t)p * stride + j];
  }
  if (threadIdx.x == 0) {
    hist2[(size_t)r * stride + pos + 1] = new_tok[r];
    tok[r] = new_tok[r];
    cum[r] = new_cum[r];
  }
}

hipError_t launch_beam_reorder(const int32_t* parent, const int32_t* new_tok, const float* new_cum,
                               const int32_t* anc, int32_t* anc2, const int32_t* hist, int32_t* hist2,
                               int32_t* tok, float* cum, int rows, int stride, int pos,
                               hipStream_t stream) {
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(rows), dim3(256), 0, stream, parent, new_tok, new_cum,
                     anc, anc2, hist, hist2, tok, cum, stride, pos);
  return hipGetLastError();
}

// ------------------------------------------------------------------------- small helpers
__global__ void beam_init_kernel(int32_t* tok, float* cum, int32_t* nactive, int32_t* done,
                                 int32_t* ndone, int32_t* fin_count, int32_t* hist, int32_t* anc,
                                 float* margins, int rows, int n, int stride, int first_tok,
                                 const int32_t* __restrict__ first_toks, int first_stride, int beam) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) {
    if (first_toks) first_tok = first_toks[(size_t)(i / beam) * first_stride];
    tok[i] = first_tok;
    cum[i] = 0.f;
    hist[(size_t)i * stride] = first_tok;
    anc[(size_t)i * stride] = i;
  }
  if (i < n) {
    nactive[i] = 1;
    done[i] = 0;
    fin_count[i] = 0;
    if (margins) margins[2 * i] = margins[2 * i + 1] = INFINITY;
  }
  if (i == 0) *ndone = 0;
}

hipError_t launch_beam_init(int32_t* tok, float* cum, int32_t* nactive, int32_t* done, int32_t* ndone,
                            int32_t* fin_count, int32_t* hist, int32_t* anc, float* margins, int rows, int n,
                            int stride, int first_tok, hipStream_t stream, const int32_t* first_toks, int first_stride,
                            int beam) {
  const int total = rows > n ? rows : n;
  hipLaunchKernelGGL(beam_init_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, tok, cum, nactive,
                     done, ndone, fin_count, hist, anc, margins, rows, n, stride, first_tok, first_toks, first_stride,
                     beam < 1 ? 1 : beam);
  return hipGetLastError();
}

// finished hypotheses of each sentence sorted best first -> caller buffers
__global__ void beam_output_kernel(const int32_t* __restrict__ fin_tok, const int32_t* __restrict__ fin_len,
                                   const float* __restrict__ fin_score, const int32_t* __restrict__ fin_count,
                                   int beam, int stride, int out_stride, int32_t* __restrict__ out_tok,
                                   int32_t* __restrict__ out_len, float* __restrict__ out_score,
                                   float* __restrict__ margins) {
  __shared__ int order[8];
  const int s = blockIdx.x;
  const int cnt = fin_count[s];
  if (threadIdx.x == 0) {
    for (int i = 0; i < cnt; ++i) order[i] = i;
    for (int a = 1; a < cnt; ++a)  // stable insertion sort, score descending
      for (int b = a; b > 0 && fin_score[s * beam + order[b]] > fin_score[s * beam + order[b - 1]]; --b) {
        const int t = order[b];
        order[b] = order[b - 1];
        order[b - 1] = t;
      }
    // gap between the returned hypothesis and the runner-up (normalised-score units)
    if (margins && cnt >= 2) margins[2 * s + 1] = fin_score[s * beam + order[0]] - fin_score[s * beam + order[1]];
  }
  __syncthreads();
  for (int h = 0; h < beam; ++h) {
    int32_t* dst = out_tok + ((size_t)s * beam + h) * out_stride;
    if (h < cnt) {
      const int src = order[h];
      const int len = fin_len[s * beam + src];
      for (int i = threadIdx.x; i < out_stride; i += blockDim.x)
        dst[i] = i < len ? fin_tok[((size_t)s * beam + src) * stride + i] : -1;
      if (threadIdx.x == 0) {
        out_len[s * beam + h] = len;
        out_score[s * beam + h] = fin_score[s * beam + src];
      }
    } else {
      for (int i = threadIdx.x; i < out_stride; i += blockDim.x) dst[i] = -1;
      if (threadIdx.x == 0) {
        out_len[s * beam + h] = 0;
        out_score[s * beam + h] = -INFINITY;
      }
    }
  }
}

hipError_t launch_beam_output(const int32_t* fin_tok, const int32_t* fin_len, const float* fin_score,
                              const int32_t* fin_count, int n, int beam, int stride, int out_stride,
                              int32_t* out_tok, int32_t* out_len, float* out_score, float* margins,
                              hipStream_t stream) {
  hipLaunchKernelGGL(beam_output_kernel, dim3(n), dim3(128), 0, stream, fin_tok, fin_len, fin_score,
                     fin_count, beam, stride, out_stride, out_tok, out_len, out_score, margins);
  return hipGetLastError();
}

// tok[r] = (int32) src[r * src_stride + col]   (teacher forcing in smi_text_decoder_logits)
__global__ void gather_tokens_kernel(const int64_t* __restrict__ src, int src_stride, int col,
                                     int32_t* __restrict__ tok, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) tok[i] = (int32_t)src[(size_t)i * src_stride + col];
}

hipError_t launch_gather_tokens(const int64_t* src, int src_stride, int col, int32_t* tok, int rows,
                                hipStream_t stream) {
  hipLaunchKernelGGL(gather_tokens_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, src,
                     src_stride, col, tok, rows);
  return hipGetLastError();
}

}  // namespace smi
