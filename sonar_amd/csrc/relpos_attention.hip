// Relative-position self-attention of the conformer block, head_dim = 64 (RelativePositionSDPA of fairseq2 ~=0.4):
// scores[i][j] = ((q_i + u) . k_j + (q_i + v) . rp[i - j]) / 8, softmax over the clip's frames.
// Same transposed-score / lane-local-softmax structure as attention.hip: the register -> key map, the online softmax, the
// V^T transpose reads and the PV step are those of attn_core.hpp.  The position term of a 32-key block needs rp rows for the
// 63 relative offsets the (32 queries x 32 keys) block spans: G[rho][i] = rp[rel_lo + rho] . (q_i + v) comes out of 8 more
// MFMAs, goes through a per-wave LDS pad and is read back at row (ii - jj + 31), column ii -- bank = ii, conflict-free both
// ways.  Two kernels: relpos_attention_kernel (position rows from global memory per wave, fp32 pad) and
// relpos_attention_lds_kernel (position rows through an LDS ring, fp16 pad; the default).
#include <type_traits>

#include "attn_core.hpp"
#include "common.hpp"
#include "kernels.hpp"

namespace smi {

constexpr int RA_QB = 128, RA_KB = 32;

// K and V blocks (32 keys x 128 B each) go global -> LDS by DMA, double-buffered: the block of the next
// iteration is in flight while this one is consumed, one barrier per block, no staging registers; both in the row-major
// swizzled layouts of attn_core.hpp.  A DMA instruction writes wave-base + lane*16: thread -> (key = tid>>3, slot = tid&7)
// fetches the chunk that belongs in that slot.

// DMA sources of a thread: row tid>>3 of a 32-row block, the chunk that lands in slot tid&7 under the K and the V swizzle
struct RpDma {
  int key, kchunk, vchunk;
};
__device__ __forceinline__ RpDma rp_dma(int tid) {
  const int skey = tid >> 3, sslot = tid & 7;
  return {skey, sslot ^ ((skey >> 1) & 7), sslot ^ (((skey >> 1) & 1) << 2)};
}

// B fragments of the lane's query with the two biases added: q_chunk(c0) is the address of columns c0 .. c0 + 7 of its head
template <typename Src>
__device__ __forceinline__ void rp_query_frags(half8 (&qu)[4], half8 (&qv)[4], Src q_chunk, const float* __restrict__ u_bias,
                                               const float* __restrict__ v_bias, int h, int hi) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int c0 = (ks * 2 + hi) * 8;
    const half8 q = *(const half8*)q_chunk(c0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      qu[ks][e] = (f16)((float)q[e] + u_bias[h * 64 + c0 + e]);
      qv[ks][e] = (f16)((float)q[e] + v_bias[h * 64 + c0 + e]);
    }
  }
}

// One half of a wave's pad, G[32 rho][32 queries] (float or f16) = (32 position rows, A fragments rf) . (q + v)^T
template <typename T>
__device__ __forceinline__ void rp_pad_half(T* G, const half8 (&rf)[4], const half8 (&qv)[4], int l31, int hi) {
  f32x16 g;
#pragma unroll
  for (int r = 0; r < 16; ++r) g[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) g = __builtin_amdgcn_mfma_f32_32x32x16_f16(rf[ks], qv[ks], g, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) G[(attn_key(r) + 4 * hi) * 32 + l31] = (T)g[r];
}

// 3 waves per SIMD (<= 168 registers; 3 workgroups x 48 KiB of LDS per CU): the kernel is a chain of LDS round trips, DMA
// waits and one barrier per 32-key block, so a third resident workgroup is what hides them (round 4; it took 204 registers =
// 2 waves before the pad addresses and the first block's second pad half stopped occupying 31 registers across the loop).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void relpos_attention_kernel(const f16* __restrict__ qkv,
                                                               const int32_t* __restrict__ cu,
                                                               const f16* __restrict__ rp, int rp_zero,
                                                               int rp_rows,
                                                               const float* __restrict__ u_bias,
                                                               const float* __restrict__ v_bias,
                                                               f16* __restrict__ ctx, int d, float sl2e,
                                                               int ctx_tm) {
  constexpr int BLK = RA_KB * 128;  // 4 KiB
  __shared__ __attribute__((aligned(16))) char lds[4 * BLK + 4 * 64 * 32 * 4];
  const int n = blockIdx.x, h = blockIdx.y;
  const int start = cu[n], len = cu[n + 1] - start;
  const int q0 = blockIdx.z * RA_QB;
  if (q0 >= len) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  float* Gs = (float*)(lds + 4 * BLK) + wave * 64 * 32;  // [64 rho][32 queries]
  char* const kvb = lds;
  const size_t ld = (size_t)3 * d;
  const f16* qbase = qkv + (size_t)start * ld + h * 64;
  const f16* kbase = qbase + d;
  const f16* vbase = qbase + 2 * d;
  const f16* rph = rp + h * 64;

  const int i0 = q0 + wave * 32;
  const int qi = i0 + l31;
  const f16* qptr = qbase + (size_t)min(qi, len - 1) * ld;
  half8 qu[4], qv[4];
  rp_query_frags(qu, qv, [&](int c0) { return qptr + c0; }, u_bias, v_bias, h, hi);

  const RpDma dma = rp_dma(tid);
  auto stage = [&](int j0, int buf) {
    const int row = min(j0 + dma.key, len - 1);
    glds16(kbase + (size_t)row * ld + dma.kchunk * 8, kvb + buf * 2 * BLK + wave * 1024);
    glds16(vbase + (size_t)row * ld + dma.vchunk * 8, kvb + buf * 2 * BLK + BLK + wave * 1024);
  };
  // position rows of a key block: rp[rel_lo + 32 gb + l31], rel_lo = i0 - j0 - 31
  auto rp_row = [&](int j0, int gb) {
    const int row = min(max(i0 - j0 - 31 + gb * 32 + l31 + rp_zero, 0), rp_rows - 1);
    return rph + (size_t)row * d;
  };

  float m = -1e30f, lsum = 0.f;
  f32x16 o[2];
  attn_zero(o);
  unsigned vaddr[2];
  attn_vt_addr(vaddr, kvb + BLK, lane, 4 * hi);
  // pad read addresses: query l31 needs G[rho][l31] for rho = l31 - jj + 31, jj = the key of accumulator register r.  Row rho
  // of an EVEN key block sits at rho * 128 B (rows 0..31 = this block's half, 32..63 = the previous block's); an odd block
  // swaps the halves, i.e. adds 4 KiB modulo 8 KiB.  With jj(r) = c_r + 4 hi, c_r = attn_key(r), every read is
  // (gbase + parity * 4096 - c_r * 128) mod 8192: ONE base register and compile-time offsets (round 4: the 16 per-register
  // offsets of round 1-3 cost 15 VGPRs of a kernel that sits one register class above 3 waves per SIMD).
  const int gbase = (l31 + 31 - 4 * hi) * 128 + l31 * 4;
  stage(0, 0);
  half8 rf[4];  // the position rows of the NEXT block travel through the softmax / PV half of this one
  {
    // The first key block needs BOTH pad halves (rho 32..63 have no previous block to come from): that half is computed
    // here, in a prologue, so that its four position-row registers are not live inside the loop (they were: `if (kb == 0)`
    // in the loop body kept 16 more VGPRs alive across every iteration's peak).  All eight 16-B loads are issued
    // together, ahead of the K / V wait.
    half8 rf_hi[4];
    const f16* rrow = rp_row(0, 0);
    const f16* rrow1 = rp_row(0, 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rf[ks] = *(const half8*)(rrow + (ks * 2 + hi) * 8);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rf_hi[ks] = *(const half8*)(rrow1 + (ks * 2 + hi) * 8);
    rp_pad_half(Gs + 32 * 32, rf_hi, qv, l31, hi);  // block 0 reads rho 32..63 from half 1
  }

  for (int j0 = 0, kb = 0; j0 < len; j0 += RA_KB, ++kb) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // block kb has landed for everyone; everyone is done with the other buffer

    // ---- content term: S^T = K . (Q+u)^T ----
    f32x16 s = attn_k_scores(kvb + (kb & 1) * 2 * BLK, l31, hi, qu);
    // ---- position term: G[rho][i] = rp[rel_lo + rho] . (q_i + v), rho = 0..63 ----
    // rel_lo drops by 32 per key block, so rows 32..63 of this block are rows 0..31 of the previous
    // one: the pad is two 32-row halves used alternately, and only the first key block computes both.
    rp_pad_half(Gs + (kb & 1) * 32 * 32, rf, qv, l31, hi);  // rho 0..31 of this block
    // next block: K / V by DMA into the other buffer, its position rows into rf
    if (j0 + RA_KB < len) {
      stage(j0 + RA_KB, (kb + 1) & 1);
      const f16* rrow = rp_row(j0 + RA_KB, 0);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) rf[ks] = *(const half8*)(rrow + (ks * 2 + hi) * 8);
    }
    // (each wave reads back only what it wrote: no workgroup barrier needed, only LDS ordering)
    // the 16 pad reads are issued back to back and waited for once (left to itself hipcc sinks each
    // read into the branch of its `< len` mask: 16 exec-masked blocks, each with its own LDS wait)
    float bd[16];
    int gb = gbase + ((kb & 1) << 12);
    asm volatile("" : "+v"(gb));  // one live base: keep hipcc from materialising the 16 (or 32) addresses in registers
#pragma unroll
    for (int r = 0; r < 16; ++r) bd[r] = *(const float*)((const char*)Gs + ((gb - attn_key(r) * 128) & 8191));
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(bd[r]));
    // x = content + position (unscaled); only the last key block of a clip has keys to mask
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] += bd[r];
    if (j0 + RA_KB > len) s = attn_mask_tail(s, j0, 4 * hi, len);
    attn_lazy_rescale(attn_block_max(s, sl2e), m, lsum, o);  // (the 32 output accumulators live in AGPRs)
    const AttnP p = attn_exp_p(s, sl2e, m);
    lsum += p.sum;
    attn_pv(o, p.pf, vaddr, (kb & 1) * 2 * BLK);
  }
  const float inv = attn_finish(lsum);
  if (qi < len) attn_store_row(o, inv, ctx, start + qi, h * 64, d, hi, ctx_tm);
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 6: the same kernel with the position rows staged ONCE per workgroup through LDS and the score pad in fp16.
// What bounded the kernel above (profiles/r06_experiments.txt, experiment 14): not its ~250 VALU instructions per key block and
// not exposed latency, but the throughput of its global loads -- every wave fetched its own 32 position rows per block as four
// global_load_dwordx4 that each touch 32 different 128-B lines (the MFMA A-operand layout wants lane = row): 128 line requests
// for 4 KiB, and every row is fetched by all four waves of the workgroup one block apart (a quarter of the kernel's time).
//  * The rows a workgroup needs at key block kb are the aligned 32-row blocks b = w - kb of rp[A + 32 b + (0..31)], A = q0 - 31 +
//    rp_zero, for its waves w = 0..3 (plus b = w + 1 for the first block's second pad half): from one key block to the next ONE
//    new block enters.  A ring of five 4 KiB slots (slot = b mod 5) holds them; the new block arrives by one coalesced LDS-DMA
//    instruction per thread (rows clamped to the table as before), in the K layout (row-major, 16-B chunk c of row r at c ^
//    ((r >> 1) & 7)), and every wave reads its A fragments with four conflict-free ds_read_b128: a quarter of the L2 -> CU bytes,
//    a sixteenth of the line requests.
//  * LDS: 16 KiB K / V + 20 KiB ring leave 16 KiB of the 52 KiB that let three workgroups share a CU, so the pad holds the
//    position scores in fp16 ([64 rho][32 queries] x 2 B per wave).  The reference's fp16 model rounds the position scores (and
//    the content scores) to fp16 before adding them (fairseq2 RelativePositionSDPA: two fp16 matmuls); here only the position
//    term takes that rounding, the sum and the softmax stay fp32.
// SMI_SPEECH_RP_LDS=0: the kernel above (A/B runs).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void relpos_attention_lds_kernel(
    const f16* __restrict__ qkv, const int32_t* __restrict__ cu, const f16* __restrict__ rp, int rp_zero, int rp_rows,
    const float* __restrict__ u_bias, const float* __restrict__ v_bias, f16* __restrict__ ctx, int d, float sl2e, int ctx_tm,
    int qkv_tm) {
  constexpr int BLK = RA_KB * 128;  // 4 KiB
  __shared__ __attribute__((aligned(16))) char lds[4 * BLK + 4 * BLK + 5 * BLK];  // K / V x 2 | fp16 pads | position-row ring
  const int n = blockIdx.x, h = blockIdx.y;
  const int start = cu[n], len = cu[n + 1] - start;
  const int q0 = blockIdx.z * RA_QB;
  if (q0 >= len) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  char* const kvb = lds;
  f16* Gs = (f16*)(lds + 4 * BLK) + wave * 64 * 32;  // [64 rho][32 queries]
  char* ring = lds + 4 * BLK + 4 * BLK;
  const size_t ld = (size_t)3 * d;
  // qkv_tm: the fused QKV projection leaves q | k | v in the tile-major layout (common.hpp; K = 3 d), which lets that GEMM run on the
  // 4-wave engine: a 16-B chunk of a row is a 16-B chunk there too, the chunks of 8 consecutive rows of a 32-column block are 512
  // contiguous bytes, so the per-thread DMA sources below only change their address arithmetic
  auto src = [&](int row, int col) -> const f16* {  // 16-B chunk (start + row, col .. col + 7) of qkv
    return qkv_tm ? qkv + tm_offset(start + row, col, 3 * d) : qkv + (size_t)(start + row) * ld + col;
  };
  const f16* rph = rp + h * 64;

  const int i0 = q0 + wave * 32;
  const int qi = i0 + l31;
  half8 qu[4], qv[4];
  rp_query_frags(qu, qv, [&](int c0) { return src(min(qi, len - 1), h * 64 + c0); }, u_bias, v_bias, h, hi);

  const RpDma dma = rp_dma(tid);
  auto stage = [&](int j0, int buf) {
    const int row = min(j0 + dma.key, len - 1);
    glds16(src(row, d + h * 64 + dma.kchunk * 8), kvb + buf * 2 * BLK + wave * 1024);
    glds16(src(row, 2 * d + h * 64 + dma.vchunk * 8), kvb + buf * 2 * BLK + BLK + wave * 1024);
  };
  // position rows: aligned block b = rows A + 32 b + (0..31), clamped to the table, into ring slot `slot` (K layout)
  const int rowA = q0 - 31 + rp_zero + dma.key;
  auto stage_rp = [&](int b, int slot) {
    const int row = min(max(rowA + 32 * b, 0), rp_rows - 1);
    glds16(rph + (size_t)row * d + dma.kchunk * 8, ring + slot * BLK + wave * 1024);
  };
  // A fragments of the 32-row block (K layout) at LDS address `blk`: row l31, chunks (2 ks + hi).  asm: a C++ LDS load behind an
  // LDS-DMA issue gets `s_waitcnt vmcnt(0)` from hipcc while the next block's transfers are in flight
  auto frags = [&](unsigned blk, half8 (&f)[4]) {
    const unsigned a = blk + l31 * 128;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      asm volatile("ds_read_b128 %0, %1" : "=v"(f[ks]) : "v"(a + (((ks * 2 + hi) ^ ((l31 >> 1) & 7)) << 4)) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) : : "memory");
  };
  auto rp_frags = [&](int slot, half8 (&rf)[4]) { frags((unsigned)(size_t)ring + slot * BLK, rf); };

  float m = -1e30f, lsum = 0.f;
  f32x16 o[2];
  attn_zero(o);
  unsigned vaddr[2];
  attn_vt_addr(vaddr, kvb + BLK, lane, 4 * hi);
  // pad reads: byte ((l31 + 31 - 4 hi) * 64 + l31 * 2 + parity * 2048 - c_r * 64) mod 4096 of the wave's pad (rows of 32 fp16),
  // c_r = attn_key(r).  Of an even block: rd_base + (27 - c_r) * 64, no wrap; of an odd block: the same xor 2048
  const unsigned rd_base = (unsigned)(size_t)Gs + (l31 + 31 - 4 * hi - 27) * 64 + l31 * 2;
  stage(0, 0);
#pragma unroll
  for (int b = 0; b < 5; ++b) stage_rp(b, b);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  {
    // the first key block needs BOTH pad halves: rho 32..63 = block wave + 1
    half8 rf_hi[4];
    rp_frags(wave + 1, rf_hi);
    rp_pad_half(Gs + 32 * 32, rf_hi, qv, l31, hi);  // block 0 reads rho 32..63 from half 1
  }

  int rslot = wave;  // ring slot of block (wave - kb)
  int dslot = 4;     // ring slot of block -(kb + 1), the one that arrives during key block kb
  // one 32-key block; P = parity of the block index (which K / V buffer, which pad half is the new one): the loop is unrolled by
  // two so that the pad addresses of an even block are one base + compile-time offsets and those of an odd block one xor away
  // (+2 KiB modulo the 4 KiB pad), the exponent arguments come from v_pk_fma_f32 and the row sum from a tree of packed adds
  // (experiment 14: 16 adds + 16 ands + 16 adds per block for the wrapped reads, 16 + 16 scalar VALU operations for the rest)
  auto block = [&](auto ptag, int j0) {
    constexpr int kb = decltype(ptag)::value;  // only its parity is used below
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // block kb (K, V, its position rows) has landed for everyone; everyone is done with the other buffers

    // ---- content term: S^T = K . (Q+u)^T ----
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    {
      half8 kf[4];
      frags((unsigned)(size_t)kvb + (kb & 1) * 2 * BLK, kf);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qu[ks], s, 0, 0, 0);
    }
    // ---- position term: G[rho][i] = rp[rel_lo + rho] . (q_i + v), rho = 0..31 new, 32..63 = the previous block's ----
    {
      half8 rf[4];
      rp_frags(rslot, rf);
      rp_pad_half(Gs + (kb & 1) * 32 * 32, rf, qv, l31, hi);
    }
    // next block: K / V into the other buffer, the one new block of position rows into the slot that just fell out of use
    if (j0 + RA_KB < len) {
      stage(j0 + RA_KB, (kb + 1) & 1);
      stage_rp(-(j0 / RA_KB + 1), dslot);
    }
    rslot = rslot ? rslot - 1 : 4;
    dslot = dslot ? dslot - 1 : 4;
    float bd[16];
    {
      // 32-bit destinations: ds_read_u16 zero-extends itself.  With 16-bit asm outputs hipcc masks every result with 0xffff right
      // behind its load -- in front of the wait below, i.e. on a register the data has not reached yet (stale values whenever a
      // second workgroup on the CU delays the LDS: the run-to-run differences this kernel had at first).
      unsigned raw[16];
      unsigned rb = rd_base;
      asm volatile("" : "+v"(rb));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr ((kb & 1) == 0) {
          asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(raw[r]) : "v"(rb), "n"((27 - attn_key(r)) * 64) : "memory");
        } else {
          const unsigned a = (rb + (27 - attn_key(r)) * 64) ^ 2048u;
          asm volatile("ds_read_u16 %0, %1" : "=v"(raw[r]) : "v"(a) : "memory");
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(raw[0]), "+v"(raw[1]), "+v"(raw[2]), "+v"(raw[3]), "+v"(raw[4]), "+v"(raw[5]), "+v"(raw[6]), "+v"(raw[7]),
                     "+v"(raw[8]), "+v"(raw[9]), "+v"(raw[10]), "+v"(raw[11]), "+v"(raw[12]), "+v"(raw[13]), "+v"(raw[14]),
                     "+v"(raw[15])
                   :
                   : "memory");
#pragma unroll
      for (int r = 0; r < 16; ++r) bd[r] = (float)__builtin_bit_cast(f16, (unsigned short)raw[r]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] += bd[r];
    if (j0 + RA_KB > len) s = attn_mask_tail(s, j0, 4 * hi, len);
    attn_lazy_rescale(attn_block_max(s, sl2e), m, lsum, o);
    const AttnP p = attn_exp_p_packed(s, sl2e, m);
    lsum += p.sum;
    attn_pv(o, p.pf, vaddr, (kb & 1) * 2 * BLK);
  };
  for (int j0 = 0;;) {
    block(std::integral_constant<int, 0>{}, j0);
    j0 += RA_KB;
    if (j0 >= len) break;
    block(std::integral_constant<int, 1>{}, j0);
    j0 += RA_KB;
    if (j0 >= len) break;
  }
  const float inv = attn_finish(lsum);
  if (qi < len) attn_store_row(o, inv, ctx, start + qi, h * 64, d, hi, ctx_tm);
}

bool relpos_attention_reads_tile_major() { return tune(TUNE_SPEECH_RP_LDS, 1) != 0; }

hipError_t launch_relpos_attention(const f16* qkv, const int32_t* cu, const f16* rp, int rp_zero, int rp_rows,
                                   const float* u_bias, const float* v_bias, f16* ctx, int n, int max_len, int d,
                                   int heads, hipStream_t stream, int ctx_tm, int qkv_tm) {
  if (heads <= 0 || d != heads * 64 || n <= 0 || max_len <= 0) return hipErrorInvalidValue;
  if (qkv_tm && tune(TUNE_SPEECH_RP_LDS, 1) == 0) return hipErrorInvalidValue;  // only the LDS-ring kernel reads tile-major q | k | v
  const float sl2e = 0.125f * 1.4426950408889634f;
  dim3 grid(n, heads, (max_len + RA_QB - 1) / RA_QB);
  if (tune(TUNE_SPEECH_RP_LDS, 1) != 0)
    hipLaunchKernelGGL(relpos_attention_lds_kernel, grid, dim3(256), 0, stream, qkv, cu, rp, rp_zero, rp_rows, u_bias, v_bias,
                       ctx, d, sl2e, ctx_tm, qkv_tm);
  else
    hipLaunchKernelGGL(relpos_attention_kernel, grid, dim3(256), 0, stream, qkv, cu, rp, rp_zero, rp_rows, u_bias,
                       v_bias, ctx, d, sl2e, ctx_tm);
  return hipGetLastError();
}

}  // namespace smi
