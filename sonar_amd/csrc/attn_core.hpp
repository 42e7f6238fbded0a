// The online-softmax core of the MFMA attention kernels for head_dim 64 (attention.hip: attention_kernel;
// relpos_attention.hip: relpos_attention_kernel, relpos_attention_lds_kernel), once.  One wave owns 32 queries and takes the
// keys in blocks of 32.  Scores are computed TRANSPOSED, S^T = K . Q^T on v_mfma_f32_32x32x16_f16, so lane (l31, hi) holds 16
// scores of ONE query, l31: the softmax is lane-local but for one exchange with the lane 32 away, and the fp32 scores convert
// in-register into the B operand of O^T += V^T . P^T (the 16-wide MFMA k-slot order is a free permutation as long as V^T is
// fetched in the same order).  K and V blocks are row-major [key][128 B] in LDS, 16-B chunk c of key r at slot c ^ swz(r):
// K swz = (r >> 1) & 7 (conflict-free ds_read_b128), V swz = ((r >> 1) & 1) << 2 (ds_read_b64_tr_b16 over all 64 banks).
// Per lane: m, the running reference of the SCALED scores (log2 domain, starts at -1e30f), lsum, the sum of its p, and o[2],
// the 32 dims x (its query) of the output for its 8 rows of each 32-dim block db.
#pragma once
#include "common.hpp"

namespace smi {

// The S^T register -> key map: accumulator register r of a lane in half hi holds the score of key attn_key(r) + 4 hi of the
// 32-key block (and k slot e of PV MFMA u is key 16 u + 4 hi + 8 (e >> 2) + (e & 3): the same map over r = 8 u + e).
// attn_key(r) never has bit 2 set, so `attn_key(r) | hi4` is the same key.  Helpers that need 4 hi take it as hi4, multiplied
// by the kernel: there it is one value shared with the kernel's own uses, and that is what keeps attention_kernel's
// registers where they were (profiles/isa_identity_attn_core.txt).
constexpr int attn_key(int r) { return (r & 3) + 8 * (r >> 2); }

__device__ __forceinline__ void attn_zero(f32x16 (&o)[2]) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
}

// joins the two halves' sums of a query; returns 1 / (the softmax denominator).  (By reference: by value the loop's
// accumulator phis come out in another order and attention_kernel takes 4 more VGPRs.)
__device__ __forceinline__ float attn_finish(const float& lsum) {
  const float ltot = lsum + __shfl_xor(lsum, 32, 64);
  return 1.0f / ltot;
}

// V^T fragment addresses of block 0 of the V tile at LDS address v_tile: lane p of a 16-lane group feeds row (p >> 2) of its
// [4 keys][16 dims] block and gets the 4 keys of dim p.  MFMA (db, u), half `part`: keys 16 u + 4 hi + 8 part + (0..3), dims
// 32 db + 16 (l31 >> 4) + (0..15); 16 u + 8 part (and 32 per further block) never changes the swizzle bit, so attn_pv adds it
// as an immediate offset.
__device__ __forceinline__ void attn_vt_addr(unsigned (&vaddr)[2], const char* v_tile, int lane, int hi4) {
  const int p16 = lane & 15, g16 = (lane >> 4) & 1;
  const int key = hi4 + (p16 >> 2);
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    const int chunk = db * 4 + g16 * 2 + ((p16 & 3) >> 1);
    vaddr[db] = (unsigned)(size_t)(v_tile + key * 128 + ((chunk ^ (((key >> 1) & 1) << 2)) << 4) + (p16 & 1) * 8);
  }
}

// S^T = K . Q^T of the 32-key block whose row krow (the lane's key: l31, + 32 per block of the tile) sits in k_tile
__device__ __forceinline__ f32x16 attn_k_scores(const char* k_tile, int krow, int hi, const half8 (&qf)[4]) {
  f32x16 s;
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const half8 kf = *(const half8*)(k_tile + krow * 128 + (((ks * 2 + hi) ^ ((krow >> 1) & 7)) << 4));
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s, 0, 0, 0);
  }
  return s;
}

// keys at or past len are out (key0 = the block's first key); the caller tests first whether the block has any
__device__ __forceinline__ f32x16 attn_mask_tail(f32x16 s, int key0, int hi4, int len) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (key0 + (attn_key(r) | hi4) >= len) s[r] = -INFINITY;
  return s;
}

// The scaled maximum of a query's 32 scores (sl2e > 0).  The other half of the keys sits 32 lanes away: v_permlane32_swap
// (VALU) instead of __shfl_xor (an LDS round trip in the middle of the softmax chain, once per key block).
__device__ __forceinline__ float attn_block_max(f32x16 s, float sl2e) {
  float mx = s[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
  return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * sl2e;
}

// Lazy rescale: the reference m only moves when some query's block maximum mx exceeds it by more than 2^8; until then
// p = exp2(x - m) <= 256 (fine in fp32 and in range for the fp16 P operand) and the 32 output accumulators are left alone.
__device__ __forceinline__ void attn_lazy_rescale(float mx, float& m, float& lsum, f32x16 (&o)[2]) {
  if (__any(mx > m + 8.0f)) {
    const float m_new = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    lsum *= alpha;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
  }
}

// p = exp2(s * sl2e - m) of a block: the B operands pf[u] (keys 16 u ..) of the PV step and the lane's sum of p
struct AttnP {
  half8 pf[2];
  float sum;
};
__device__ __forceinline__ AttnP attn_exp_p(f32x16 s, float sl2e, float m) {
  AttnP p;
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], sl2e, -m));
    psum += e;
    p.pf[r >> 3][r & 7] = (f16)e;
  }
  p.sum = psum;
  return p;
}

// The same with the exponent arguments from v_pk_fma_f32 and the sum as a tree of packed adds: 16 + 16 scalar VALU operations
// fewer per block, another summation order (relpos_attention_lds_kernel, which is bound by its VALU work per key block).
__device__ __forceinline__ AttnP attn_exp_p_packed(f32x16 s, float sl2e, float m) {
  AttnP p;
  f32x2 ps2[8];
  const f32x2 sc2 = {sl2e, sl2e}, nm2 = {-m, -m};
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const f32x2 a = __builtin_elementwise_fma(f32x2{s[r], s[r + 1]}, sc2, nm2);
    const f32x2 pp = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
    ps2[r >> 1] = pp;
    p.pf[r >> 3][r & 7] = (f16)pp[0];
    p.pf[r >> 3][(r & 7) + 1] = (f16)pp[1];
  }
  const f32x2 t0 = (ps2[0] + ps2[1]) + (ps2[2] + ps2[3]), t1 = (ps2[4] + ps2[5]) + (ps2[6] + ps2[7]);
  const f32x2 t = t0 + t1;
  p.sum = t[0] + t[1];
  return p;
}

// O^T += V^T . P^T of the 32-key block that starts `off` bytes behind block 0 of attn_vt_addr (buffer and block offset).
__device__ __forceinline__ void attn_pv(f32x16 (&o)[2], const half8 (&pf)[2], const unsigned (&vaddr)[2], unsigned off) {
  half4 va[2][2][2];  // [db][u][part]
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    const unsigned a = vaddr[db] + off;
    va[db][0][0] = lds_tr_read_b64<0>(a);
    va[db][0][1] = lds_tr_read_b64<1024>(a);
    va[db][1][0] = lds_tr_read_b64<2048>(a);
    va[db][1][1] = lds_tr_read_b64<3072>(a);
  }
  // the wait carries the 8 results as operands: the MFMAs below depend on IT, not just on the reads
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(va[0][0][0]), "+v"(va[0][0][1]), "+v"(va[0][1][0]), "+v"(va[0][1][1]), "+v"(va[1][0][0]),
                 "+v"(va[1][0][1]), "+v"(va[1][1][0]), "+v"(va[1][1][1])
               :
               : "memory");
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      half8 vf;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vf[e] = va[db][u][0][e];
        vf[4 + e] = va[db][u][1][e];
      }
      o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[u], o[db], 0, 0, 0);
    }
}

// Read-out of a lane's query: o * inv as fp16 to columns col0 + 32 db + 8 q + 4 hi + (0..3) of row `row` of ctx [rows][d],
// row-major, or (ctx_tm) in the tile-major GEMM operand layout (common.hpp: any packed row addresses its own 64-B slice of a
// 16 KiB block, no alignment of the sentence or clip needed).
__device__ __forceinline__ void attn_store_row(const f32x16 (&o)[2], float inv, f16* ctx, int row, int col0, int d, int hi,
                                               int ctx_tm) {
  f16* op = ctx + (size_t)row * d + col0;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      half4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (f16)(o[db][q * 4 + e] * inv);
      const int col = db * 32 + 8 * q + 4 * hi;
      if (ctx_tm) *(half4*)(ctx + tm_offset(row, col0 + col, d)) = v;
      else *(half4*)(op + col) = v;
    }
}

}  // namespace smi
