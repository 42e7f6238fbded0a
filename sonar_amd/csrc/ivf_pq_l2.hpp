// L2 search over the product-quantised lists, plain and residual (restated in tests/ivf_pq_l2_ref.py).
// The stored row is what the codes decode to, y^ (plain) or c + r^ (residual: c the fp16 centroid of the slot's list, r^ the
// decoded fp16 residual), and the Euclidean nearest row is the one with the largest q.y^ - 1/2 ||y^||^2.  The query's part is
// the sum the PQ scan already forms; the rest hangs on the slot alone and is ONE fp32 per slot, the bias:
//   plain     bias = -fl32(1/2 ||y^||^2)                          score = fl32(acc + bias)
//   residual  bias = -fl32(S1 + S2), S1 = sum c r^, S2 = 1/2 sum r^ r^      score = fl32(fl32(acc + bias) + coarse)
// with coarse = q.c - 1/2 ||c||^2, the biased score the L2 probe returns beside the list number:
//   q.y^ - 1/2 ||y^||^2 = (q.c - 1/2 ||c||^2) + q.r^ - (c.r^ + 1/2 ||r^||^2).
// Every sum of a bias is an fp64 sum in l2_half_norm's order (l2_rows.hpp, called); S1 and S2 are joined by one fp64 add and
// rounded to fp32 once.  The plain bias has the bits smi_l2_prepare gives the decoded row, negated.
// Two kernels: the bias of a set of items (one wave each, no n x d temporary) and the PQ scan with the flat L2 scan's change.
// This header is included once, inside ivf.hip's unnamed namespace, behind every kernel the parent commit had.

// The bias of one item, in every lane of its wave: code = its M code bytes, crow = the centroid row of its list (RES; null:
// none, the residual is the row itself).  Chunk c of the decoded row is 16 bytes of one codeword (dsub >= 8).
template <bool RES>
__device__ __forceinline__ float pq_l2_item_bias(const uint8_t* __restrict__ code, int d, int dshift, const f16* __restrict__ cb,
                                                 const f16* __restrict__ crow, int lane) {
  const int dmask = (1 << dshift) - 1;
  auto codeword = [&](int c) {
    const int k0 = c * 8, m = k0 >> dshift;
    return *(const half8*)(cb + (((size_t)m * PQ_CW + code[m]) << dshift) + (k0 & dmask));
  };
  if constexpr (!RES) {
    return -l2_half_norm(d, lane, codeword);
  } else {
    const double s2 = 0.5 * l2_ordered_sum(d, lane, [&](int c, double& s) {
      const half8 r = codeword(c);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += (double)r[e] * (double)r[e];
    });
    const double s1 = !crow ? 0.0 : l2_ordered_sum(d, lane, [&](int c, double& s) {
      const half8 r = codeword(c), cv = *(const half8*)(crow + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += (double)cv[e] * (double)r[e];
    });
    return -(float)(s1 + s2);
  }
}

// One wave per item i < n of codes uint8 [n, M].  ids (nullable): the items are slots, and one whose id is below 0 (a pad, an
// unused slot: its codes may be unwritten) gets 0 without its codes being read.  RES: the item's list is labels[i] (labels
// given) or the list slot i lies in by off (int32 [K + 1], bisection); outside [0, K): no centroid.
template <bool RES>
__global__ __launch_bounds__(IVF_TB) void pq_l2_bias_kernel(const uint8_t* __restrict__ codes, int64_t n, int d, int dshift,
                                                            const f16* __restrict__ cb, const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ off, const int32_t* __restrict__ labels,
                                                            const f16* __restrict__ cent, int K, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (i >= n) return;  // wave-uniform
  float b = 0.f;
  if (!ids || ids[i] >= 0) {
    const f16* crow = nullptr;
    if constexpr (RES) crow = pq_centroid_row(cent, K, d, labels ? labels[i] : i < off[K] ? ivf_unit_list(off, K, (int)i) : -1);
    b = pq_l2_item_bias<RES>(codes + (size_t)i * (d >> dshift), d, dshift, cb, crow, lane);
  }
  if (lane == 0) out[i] = b;
}

// ivf_pq_scan_lists_kernel with the change ivf_l2_scan_lists_kernel made to the flat scan: the fold loads the four slot
// biases with one 16-byte load beside the four ids.  Score = a + b4[r], and with RES (a + b4[r]) + c, the pair's coarse term
// waiting in LDS behind the pair numbers as in the cosine kernel.  The sum starts from +0 and is never -0, so a zero score is
// +0.  A pad slot stays out by id >= 0, whatever its bias.  Its own kernel, outside the twice-included ivf_list_kernels.hpp:
// there is no keyed twin.
template <int KT, int B, bool RES>
__global__ __launch_bounds__(IVF_TB) void ivf_pq_l2_scan_lists_kernel(const f16* __restrict__ qn, int d, int nq, int nprobe,
                                                                      const uint8_t* __restrict__ codes, int dshift,
                                                                      const f16* __restrict__ cb, const int32_t* __restrict__ ids,
                                                                      const float* __restrict__ bias,
                                                                      const int32_t* __restrict__ off, int K,
                                                                      const int32_t* __restrict__ poff,
                                                                      const int32_t* __restrict__ ubase,
                                                                      const int32_t* __restrict__ pairs, int k_out,
                                                                      float* __restrict__ ps, int32_t* __restrict__ pi,
                                                                      const float* __restrict__ coarse) {
  constexpr int NR = B / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lists = (unsigned long long*)(smem + 4 * B * IVF_SLICE);
  int* spair = (int*)(lists + B * KT);
  [[maybe_unused]] float* scoarse = (float*)(spair + B);  // RES only
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= ubase[K]) return;
  const int l = ivf_unit_list(ubase, K, b);
  const int p0 = poff[l] + (b - ubase[l]) * B;
  const int npair = min(B, poff[l + 1] - p0);
  const int s_begin = off[l], s_end = off[l + 1];
  if constexpr (RES) {
    ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [&](int pr) { scoarse[tid] = pr >= 0 ? coarse[pr] : 0.f; });
  } else {
    ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [](int) {});
  }

  const int nk = d / IVF_BK, cc = tid & 7;
  const int T = (s_end - s_begin + B - 1) / B * nk;  // the slices of the walk
  const int M = d >> dshift, dsub = 1 << dshift;
  const f16* qsrc[NR];  // this thread's query rows of a slice
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int pr = spair[(tid >> 3) + 32 * j];
    qsrc[j] = pr >= 0 ? qn + (size_t)(pr / nprobe) * d + cc * 8 : nullptr;
  }
  unsigned cd[NR];  // the code bytes of this thread's chunk of the slice the next `fetch` gathers
  auto fetch_codes = [&](int it) {  // ivf_pq_scan_lists_kernel's, as `fetch` below
    const int tile = it / nk, ks = it - tile * nk;
    const int m = (ks * IVF_BK + cc * 8) >> dshift;  // < M
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int slot = s_begin + tile * B + (tid >> 3) + 32 * j;
      cd[j] = slot < s_end ? codes[(size_t)slot * M + m] : 0u;
    }
  };
  auto fetch = [&](int it, u32x4(&qv)[NR], u32x4(&lv)[NR]) {
    if (it == 0) fetch_codes(0);
    const int tile = it / nk, ks = it - tile * nk;
    const int k0 = ks * IVF_BK + cc * 8;
    const f16* cw = cb + ((size_t)(k0 >> dshift) * PQ_CW << dshift) + (k0 & (dsub - 1));  // codeword 0 of the sub-quantiser
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int slot = s_begin + tile * B + (tid >> 3) + 32 * j;
      qv[j] = qsrc[j] ? *(const u32x4*)(qsrc[j] + ks * IVF_BK) : u32x4{0u, 0u, 0u, 0u};
      lv[j] = slot < s_end ? *(const u32x4*)(cw + ((size_t)cd[j] << dshift)) : u32x4{0u, 0u, 0u, 0u};
    }
    if (it + 1 < T) fetch_codes(it + 1);
  };
  auto fold = [&](int slot0, const f32x4(&acc)[NR]) {
    const f32x4 b4 = *(const f32x4*)(bias + slot0);
    const IvfKeyTest<B, IvfNoKeys> pass(IvfNoKeys{}, nullptr);
    if constexpr (RES) {
      ivf_topk_fold<KT, B>(
          lists, npair, *(const int4*)(ids + slot0), acc,
          [b4, scoarse](int pr) {
            const float c = scoarse[pr];
            return [b4, c](float a, int r) { return (a + b4[r]) + c; };
          },
          pass);
    } else {
      ivf_topk_fold<KT, B>(
          lists, npair, *(const int4*)(ids + slot0), acc, [b4](int) { return [b4](float a, int r) { return a + b4[r]; }; }, pass);
    }
  };
  ivf_slice_walk<B, IvfF16>(smem, s_begin, s_end, nk, ivf_live_blocks<B>(npair), fetch, fold);
  ivf_lists_readout<KT>(lists, spair, npair, nprobe, nq, k_out, ps, pi);
}

// smi_l2_pq_bias: the refusals, then one wave per item
int pq_l2_bias_entry(const void* codes, int64_t n, int32_t d, int32_t dsub, const void* codebooks, const int32_t* slot_ids,
                     const int32_t* list_offsets, const int32_t* labels, const void* centroids, int64_t K, float* out,
                     void* stream) {
  return rows_entry(
      !codes || !out, nullptr, "", n, d,
      [&] {
        if (const int rc = pq_check_codebooks(d, dsub, codebooks)) return rc;
        if (!centroids) {
          if (labels || list_offsets)
            return fail(SMI_ERR_INVALID_ARG, "labels and list_offsets name the lists of centroids: give centroids, or neither");
          return (int)SMI_OK;
        }
        if (const int rc = pq_check_centroids(centroids, K)) return rc;
        if (!labels == !list_offsets)
          return fail(SMI_ERR_INVALID_ARG, "with centroids, give labels or list_offsets: one of the two");
        if (list_offsets && !slot_ids) return fail(SMI_ERR_INVALID_ARG, "list_offsets describe slots: give slot_ids with them");
        return (int)SMI_OK;
      },
      [&] {
        const auto grid = grid_for(n, IVF_TB / 64);
        if (centroids)
          hipLaunchKernelGGL(pq_l2_bias_kernel<true>, grid, dim3(IVF_TB), 0, (hipStream_t)stream, (const uint8_t*)codes, n, d,
                             pq_shift(dsub), (const f16*)codebooks, slot_ids, list_offsets, labels, (const f16*)centroids, (int)K, out);
        else
          hipLaunchKernelGGL(pq_l2_bias_kernel<false>, grid, dim3(IVF_TB), 0, (hipStream_t)stream, (const uint8_t*)codes, n, d,
                             pq_shift(dsub), (const f16*)codebooks, slot_ids, (const int32_t*)nullptr, (const int32_t*)nullptr,
                             (const f16*)nullptr, 0, out);
      });
}

// smi_l2_pq_search / smi_l2_pq_search_residual: smi_l2_flat_search's refusals and the PQ entries' own, over the kernel above
template <bool RES>
int pq_l2_search_entry(const void* qn, int64_t nq, int32_t d, const int32_t* probes, const float* coarse, int32_t nprobe,
                       const void* list_codes, int32_t dsub, const void* codebooks, const float* list_bias, const int32_t* list_ids,
                       const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* ws, int64_t ws_bytes,
                       void* stream) {
  return search_entry(
      !qn || !list_codes || !list_bias || (RES && !coarse), no_refusals, nq, d, probes, nprobe, list_ids, list_offsets, K, k, idx,
      score, ws, ws_bytes, stream, "smi_l2_pq_search_ws_bytes(nq, K, nprobe, k, d, dsub)", 0, 0,
      [&] {
        if (const int rc = pq_check_codebooks(d, dsub, codebooks)) return rc;
        if ((uintptr_t)list_bias % 16) return fail(SMI_ERR_INVALID_ARG, "list_bias must be 16-byte aligned");
        if (RES && (uintptr_t)coarse % 4) return fail(SMI_ERR_INVALID_ARG, "coarse must be 4-byte aligned");
        return (int)SMI_OK;
      },
      no_prepare, [&](auto kt, int unit, int64_t units, const SearchWs& w, hipStream_t st) {
        constexpr int KT = decltype(kt)::value;
        constexpr int lds_small = RES ? ivf_pq_residual_scan_lds<IVF_BM>(KT) : ivf_scan_lds<IVF_BM>(KT);
        constexpr int lds_big = RES ? ivf_pq_residual_scan_lds<IVF_BIG>(KT) : ivf_scan_lds<IVF_BIG>(KT);
        return launch_units<ivf_pq_l2_scan_lists_kernel<KT, IVF_BM, RES>, ivf_pq_l2_scan_lists_kernel<KT, IVF_BIG, RES>>(
            unit, units, lds_small, lds_big, st, (const f16*)qn, d, (int)nq, nprobe, (const uint8_t*)list_codes, pq_shift(dsub),
            (const f16*)codebooks, list_ids, list_bias, list_offsets, (int)K, (const int32_t*)w.poff, (const int32_t*)w.ubase,
            (const int32_t*)w.pairs, k, w.ps, w.pi, coarse);
      });
}
