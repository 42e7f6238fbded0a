// Multi-head self-attention over PACKED (pad-free) rows, head_dim = 64.
// Reference: StandardMultiheadAttention + SDPA with key-padding mask,
// wired at sonar/models/sonar_text/factory.py:130-141; scores * Dh^-0.5,
// softmax in fp32, P.V.  With packed rows the key-padding mask becomes the
// per-sentence key range [0, len).
//
// gfx950 mapping: one workgroup = 128 queries of one (sentence, head); each of
// the 4 waves owns 32 queries.  Scores are computed TRANSPOSED
// (S^T = K.Q^T on v_mfma_f32_32x32x16_f16), so a lane holds 16 scores of ONE
// query and P never moves between lanes or through LDS: the register -> key
// map, the lane-local online softmax with its lazy rescale, the V^T transpose
// reads and the PV step are attn_core.hpp, shared with relpos_attention.hip.
// K and V arrive by double-buffered global->LDS DMA.  S <= 514 in SONAR, so the
// kernel is HBM-bound (~64 flop/B); the score matrix never leaves registers.
#include <cstdlib>

#include "attn_core.hpp"
#include "common.hpp"
#include "kernels.hpp"

namespace smi {

constexpr int AT_QB = 128;  // queries per workgroup
constexpr int AT_KB = 64;   // keys per K/V tile

// TM: ctx is written in the tile-major GEMM operand layout (common.hpp) -- a wave then stores
// 2 KiB runs (32 rows x 64 B of one k-block) instead of 8-B pieces one row stride apart.
// QTM: qkv is READ tile-major ([T, 3d] as K = 3d blocks, the QKV GEMM's register-direct output):
// the 64-key x 64-B halves of a K or V tile are then contiguous 4 KiB runs.
//
// K and V tiles (64 keys x 128 B) go global -> LDS by DMA into two buffers: tile t+1 is in flight while
// tile t is consumed, one barrier per tile, no staging registers.  Both are row-major [key][128 B] with
// 16-B chunk c of key r at slot c ^ swz(r), the K and V swizzles of attn_core.hpp.
// NTL: the K / V tiles are loaded non-temporally (launcher: every sentence fits ONE 128-query block, so each qkv line
// is read by exactly one workgroup, once)
// CAUSAL (the decoder's teacher-forced scoring, launch_causal_attention): query i sees keys 0..i only.  The key loop of a
// 128-query block ends at min(len, q0 + 128) -- one bound for every wave, so the per-tile barrier stays uniform -- and
// the tiles that reach past q0 mask the keys after each lane's query.
template <bool TM, bool QTM, bool NTL = false, bool CAUSAL = false>
__global__ __launch_bounds__(256, 4) void attention_kernel(const f16* __restrict__ qkv,
                                                        const int32_t* __restrict__ cu,
                                                        f16* __restrict__ ctx, int d, float sl2e, int order) {
  constexpr int TILE = AT_KB * 128;  // 8 KiB
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE];  // [buffer][K | V]

  // order 0: sentence = blockIdx.x, head = blockIdx.y (dispatch order: all sentences of head 0, then head 1, ...).
  // order 1: the heads of a sentence are dispatched together, so the whole 6 KB qkv rows of a sentence are read at
  // about the same time (each head's piece is one 128-B line of the row) instead of in 16 passes over the matrix.
  int n = blockIdx.x, h = blockIdx.y;
  if (order) {
    const int lin = blockIdx.x + gridDim.x * blockIdx.y;
    h = lin % (int)gridDim.y;
    n = lin / (int)gridDim.y;
  }
  const int start = cu[n];
  const int len = cu[n + 1] - start;
  const int q0 = blockIdx.z * AT_QB;
  if (q0 >= len) return;
  const int kend = CAUSAL ? min(len, q0 + AT_QB) : len;  // keys this block reads

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const size_t ld = (size_t)3 * d;

  const int qi = q0 + wave * 32 + l31;
  const int K3 = 3 * d;
  // element (row r of this sentence, column c of the [q | k | v] row)
  auto at = [&](int r, int c) -> const f16* {
    if constexpr (QTM) return qkv + tm_offset(start + r, c, K3);
    return qkv + (size_t)(start + r) * ld + c;
  };
  half8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const half8*)at(min(qi, len - 1), h * 64 + (ks * 2 + hi) * 8);

  // DMA: instruction x of wave w fills LDS bytes [x*4096 + w*1024, +1024) of a tile: thread ->
  // (key = c>>3, slot = c&7), c = x*256 + tid, fetches the chunk that belongs in that slot
  auto stage = [&](int kv0, int buf) {
    char* kt = lds + buf * 2 * TILE;
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const int c = tid + 256 * x;
      const int key = c >> 3, slot = c & 7;
      const int row = min(kv0 + key, len - 1);
      if constexpr (NTL) {
        glds16_nt(at(row, d + h * 64 + (slot ^ ((key >> 1) & 7)) * 8), kt + x * 4096 + wave * 1024);
        glds16_nt(at(row, 2 * d + h * 64 + (slot ^ (((key >> 1) & 1) << 2)) * 8), kt + TILE + x * 4096 + wave * 1024);
      } else {
        glds16(at(row, d + h * 64 + (slot ^ ((key >> 1) & 7)) * 8), kt + x * 4096 + wave * 1024);
        glds16(at(row, 2 * d + h * 64 + (slot ^ (((key >> 1) & 1) << 2)) * 8), kt + TILE + x * 4096 + wave * 1024);
      }
    }
  };
  unsigned vaddr[2];  // V^T fragments of buffer 0, block 0
  attn_vt_addr(vaddr, lds + TILE, lane, 4 * hi);

  float m = -1e30f, lsum = 0.f;  // m: running reference of the SCALED scores (log2 domain)
  f32x16 o[2];
  attn_zero(o);

  stage(0, 0);
  for (int kv0 = 0, t = 0; kv0 < kend; kv0 += AT_KB, ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile t has landed for everyone; everyone is done with the other buffer
    if (kv0 + AT_KB < kend) stage(kv0 + AT_KB, (t + 1) & 1);
    const char* Ks = lds + (t & 1) * 2 * TILE;

    // The tile's two 32-key blocks are taken one after the other, each with its own online-softmax step: only
    // 16 scores, 8 P values and 16 V^T registers are live at a time (the 64-key version needed 131 VGPRs =
    // 3 workgroups per CU; the kernel is a short latency chain per workgroup, so resident workgroups are what pays).
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16 sc = attn_k_scores(Ks, kb * 32 + l31, hi, qf);  // S^T = K . Q^T, 32 keys
      // ---- online softmax (per query = per lane), then O^T += V^T . P^T: attn_core.hpp ----
      if (kv0 + AT_KB > len) sc = attn_mask_tail(sc, kv0 + kb * 32, 4 * hi, len);  // only a sentence's last tile has keys to mask
      if constexpr (CAUSAL) {
        if (kv0 + AT_KB > q0) {  // the tile reaches past the block's first query: keys after the lane's query are out
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kv0 + kb * 32 + attn_key(r) + 4 * hi > qi) sc[r] = -INFINITY;
        }
      }
      attn_lazy_rescale(attn_block_max(sc, sl2e), m, lsum, o);
      const AttnP p = attn_exp_p(sc, sl2e, m);
      lsum += p.sum;
      attn_pv(o, p.pf, vaddr, (t & 1) * 2 * TILE + kb * 4096);
    }
  }

  const float inv = attn_finish(lsum);
  if constexpr (TM) {
    // Tile-major context: a lane holds 8-B pieces of ONE row, so a direct store scatters 16-B pieces over 16 lines per
    // instruction.  The wave parks its 32 rows x 128 B in LDS (the K / V buffers, free after the barrier) and writes
    // them back as 16 rows x 64 B per instruction = one linear 1 KiB run of a tile-major block, 16 B per lane.
    __syncthreads();  // every wave is done with the K / V tiles
    char* st = lds + wave * 4096;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        half4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (f16)(o[db][q * 4 + e] * inv);
        *(half4*)(st + l31 * 128 + (((db * 4 + q) ^ (l31 & 7)) << 4) + hi * 8) = v;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-local hand-over: the readers below are lanes of this wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hb = i >> 1, row = (i & 1) * 16 + (lane >> 2), slot = lane & 3;
      const int qr = q0 + wave * 32 + row;
      const int rr = (start + qr) & 255;
      const int c4 = slot ^ tm_swz(rr);
      const f32x4 v = *(const f32x4*)(st + row * 128 + (((hb * 4 + c4) ^ (row & 7)) << 4));
      // whole 64-B row segments, read next by the attention-output GEMM on other XCDs: non-temporal (common.hpp)
      if (qr < len) store_nt((f32x4*)(ctx + tm_offset(start + qr, h * 64 + hb * 32 + c4 * 8, d)), v);
    }
  } else if (qi < len) {
    attn_store_row(o, inv, ctx, start + qi, h * 64, d, hi, 0);
  }
}

// Causal self-attention of the decoder's teacher-forced rows: cu = [0, seq, 2 seq, ...] (every sequence padded to seq
// rows, the padding last, so a valid query never sees a padded key); qkv row-major [rows][3d], ctx row-major [rows][d].
hipError_t launch_causal_attention(const f16* qkv, const int32_t* cu, f16* ctx, int nseq, int seq, int d, int heads,
                                   hipStream_t stream) {
  if (heads <= 0 || d != heads * 64 || nseq <= 0 || seq <= 0) return hipErrorInvalidValue;
  const float sl2e = 0.125f * 1.4426950408889634f;  // Dh^-0.5 * log2(e)
  hipLaunchKernelGGL((attention_kernel<false, false, false, true>), dim3(nseq, heads, (seq + AT_QB - 1) / AT_QB), dim3(256), 0,
                     stream, qkv, cu, ctx, d, sl2e, 1);
  return hipGetLastError();
}

hipError_t launch_attention(const f16* qkv, const int32_t* cu, f16* ctx, int N, int max_len, int d,
                            int heads, hipStream_t stream, int ctx_tm) {
  if (heads <= 0 || d != heads * 64 || N <= 0 || max_len <= 0) return hipErrorInvalidValue;
  const float sl2e = 0.125f * 1.4426950408889634f;  // Dh^-0.5 * log2(e)
  dim3 grid(N, heads, (max_len + AT_QB - 1) / AT_QB);
  const int order = tune(TUNE_ATT_ORDER, 1);  // ATT_ORDER=0: head-major dispatch (A/B measurements)
  // ctx_tm: bit 0 = ctx written tile-major, bit 1 = qkv read tile-major
  switch (ctx_tm & 3) {
    case 0: hipLaunchKernelGGL((attention_kernel<false, false>), grid, dim3(256), 0, stream, qkv, cu, ctx, d, sl2e, order); break;
    case 1: hipLaunchKernelGGL((attention_kernel<true, false>), grid, dim3(256), 0, stream, qkv, cu, ctx, d, sl2e, order); break;
    case 2: hipLaunchKernelGGL((attention_kernel<false, true>), grid, dim3(256), 0, stream, qkv, cu, ctx, d, sl2e, order); break;
    default:
      if (max_len <= AT_QB)
        hipLaunchKernelGGL((attention_kernel<true, true, true>), grid, dim3(256), 0, stream, qkv, cu, ctx, d, sl2e, order);
      else
        hipLaunchKernelGGL((attention_kernel<true, true, false>), grid, dim3(256), 0, stream, qkv, cu, ctx, d, sl2e, order);
      break;
  }
  return hipGetLastError();
}

}  // namespace smi
