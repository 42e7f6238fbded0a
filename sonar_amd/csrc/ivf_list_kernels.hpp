// The list-walking kernels of ivf.hip that answer a search -- ivf_scan_lists_kernel, ivf_range_lists_kernel,
// ivf_i8_scan_lists_kernel, ivf_pq_scan_lists_kernel -- stated once and INCLUDED TWICE by ivf.hip (no include guard; read the
// comment at the inclusion): once as the kernels themselves and once as their keyed twins <name>_keyed of the filtered search
// (DESIGN.md 3.24).  The includer defines
//   IVF_TWIN(name)     name, or name##_keyed
//   IVF_TWIN_PARAM     nothing, or `, IvfKeys keyargs`: the twin's last argument
//   IVF_TWIN_KEYS      IvfNoKeys, or IvfKeys: what IvfKeyTest (ivf_scan.hpp) is instantiated on
//   IVF_TWIN_KEYARGS   IvfNoKeys{}, or keyargs
// What each kernel does, and why, is said where ivf.hip introduces it; what the keys add is the same four lines in each: the
// IvfKeyTest `keys` over B ints of LDS behind everything else, keys.pair() in the prologue's hook, keys.rows() behind its
// barrier, keys.slots() beside the load of the ids and keys(bi, r) in the test of a candidate, behind id >= 0.

// ---------------------------------------------------------------- fp16 rows (comment: ivf.hip, "search")
template <int KT, int B>
__global__ __launch_bounds__(IVF_TB) void IVF_TWIN(ivf_scan_lists_kernel)(const f16* __restrict__ qn, int d, int nq, int nprobe,
                                                                const f16* __restrict__ rows, const int32_t* __restrict__ ids,
                                                                const int32_t* __restrict__ off, int K,
                                                                const int32_t* __restrict__ poff,
                                                                const int32_t* __restrict__ ubase,
                                                                const int32_t* __restrict__ pairs, int k_out,
                                                                float* __restrict__ ps, int32_t* __restrict__ pi IVF_TWIN_PARAM) {
  constexpr int NR = B / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lists = (unsigned long long*)(smem + 4 * B * IVF_SLICE);
  int* spair = (int*)(lists + B * KT);
  IvfKeyTest<B, IVF_TWIN_KEYS> keys(IVF_TWIN_KEYARGS, spair + B);
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= ubase[K]) return;
  const int l = ivf_unit_list(ubase, K, b);
  const int p0 = poff[l] + (b - ubase[l]) * B;
  const int npair = min(B, poff[l + 1] - p0);
  const int s_begin = off[l], s_end = off[l + 1];
  ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [&](int pr) { keys.pair(pr, nprobe); });
  keys.rows();

  const int nk = d / IVF_BK, cc = tid & 7;
  const f16* qsrc[NR];  // this thread's query rows of a slice
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int pr = spair[(tid >> 3) + 32 * j];
    qsrc[j] = pr >= 0 ? qn + (size_t)(pr / nprobe) * d + cc * 8 : nullptr;
  }
  auto fetch = [&](int it, u32x4(&qv)[NR], u32x4(&lv)[NR]) {
    const int tile = it / nk, ks = it - tile * nk;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int slot = s_begin + tile * B + (tid >> 3) + 32 * j;
      qv[j] = qsrc[j] ? *(const u32x4*)(qsrc[j] + ks * IVF_BK) : u32x4{0u, 0u, 0u, 0u};
      lv[j] = slot < s_end ? *(const u32x4*)(rows + (size_t)slot * d + ks * IVF_BK + cc * 8) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto fold = [&](int slot0, const f32x4(&acc)[NR]) {
    keys.slots(slot0);
    ivf_topk_fold<KT, B>(lists, npair, *(const int4*)(ids + slot0), acc, IvfSumIsScore{}, keys);
  };
  ivf_slice_walk<B, IvfF16>(smem, s_begin, s_end, nk, ivf_live_blocks<B>(npair), fetch, fold);
  ivf_lists_readout<KT>(lists, spair, npair, nprobe, nq, k_out, ps, pi);
}

// ---------------------------------------------------------------- range search (comment: ivf.hip)
// The query keys [B] go behind the counters.
template <int B, bool EMIT>
__global__ __launch_bounds__(IVF_TB) void IVF_TWIN(ivf_range_lists_kernel)(const f16* __restrict__ qn, int d, int nprobe,
                                                                 const float* __restrict__ threshold,
                                                                 const f16* __restrict__ rows, const int32_t* __restrict__ ids,
                                                                 const int32_t* __restrict__ off, int K,
                                                                 const int32_t* __restrict__ poff,
                                                                 const int32_t* __restrict__ ubase,
                                                                 const int32_t* __restrict__ pairs,
                                                                 int32_t* __restrict__ pair_counts,
                                                                 const int64_t* __restrict__ base, int64_t total,
                                                                 float* __restrict__ score, int32_t* __restrict__ idx IVF_TWIN_PARAM) {
  constexpr int NR = B / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* spair = (int*)(smem + 4 * B * IVF_SLICE);
  float* sthr = (float*)(spair + B);
  unsigned* scnt = (unsigned*)(sthr + B);
  IvfKeyTest<B, IVF_TWIN_KEYS> keys(IVF_TWIN_KEYARGS, scnt + B);
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= ubase[K]) return;
  const int l = ivf_unit_list(ubase, K, b);
  const int p0 = poff[l] + (b - ubase[l]) * B;
  const int npair = min(B, poff[l + 1] - p0);
  const int s_begin = off[l], s_end = off[l + 1];
  ivf_range_init<B>(spair, sthr, scnt, pairs, p0, npair, nprobe, threshold, [&](int pr) { keys.pair(pr, nprobe); });
  keys.rows();

  const int nk = d / IVF_BK, cc = tid & 7;
  const f16* qsrc[NR];  // this thread's query rows of a slice
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int pr = spair[(tid >> 3) + 32 * j];
    qsrc[j] = pr >= 0 ? qn + (size_t)(pr / nprobe) * d + cc * 8 : nullptr;
  }
  auto fetch = [&](int it, u32x4(&qv)[NR], u32x4(&lv)[NR]) {  // ivf_scan_lists_kernel's, which keeps its own text
    const int tile = it / nk, ks = it - tile * nk;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int slot = s_begin + tile * B + (tid >> 3) + 32 * j;
      qv[j] = qsrc[j] ? *(const u32x4*)(qsrc[j] + ks * IVF_BK) : u32x4{0u, 0u, 0u, 0u};
      lv[j] = slot < s_end ? *(const u32x4*)(rows + (size_t)slot * d + ks * IVF_BK + cc * 8) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  // what this lane keeps of its unit rows wc * B / 2 + bi * 16 + l15: the threshold, and the hits counted so far or the
  // pair's segment [lo, hi) of the output
  const int row0 = (tid >> 6 & 1) * (B / 2) + (tid & 15);
  float thr[NR];
  int hits[NR];
  int64_t lo[NR], hi[NR];
#pragma unroll
  for (int bi = 0; bi < NR; ++bi) {
    const int pr = spair[row0 + bi * 16];
    thr[bi] = sthr[row0 + bi * 16];
    hits[bi] = 0;
    lo[bi] = EMIT && pr >= 0 ? base[pr] : 0;
    hi[bi] = EMIT && pr >= 0 ? min(base[pr + 1], total) : 0;
  }
  auto fold = [&](int slot0, const f32x4(&acc)[NR]) {
    ivf_range_fold<B>(ids, slot0, thr, acc, keys, [&](int bi, unsigned mask, const int(&idr)[4]) {
      if constexpr (EMIT) {
        int64_t pos = lo[bi] + atomicAdd(&scnt[row0 + bi * 16], (unsigned)__popc(mask));
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (mask >> r & 1u) {
            if (pos < hi[bi]) {
              score[pos] = acc[bi][r];
              idx[pos] = idr[r];
            }
            ++pos;
          }
      } else {
        hits[bi] += __popc(mask);
      }
    });
  };
  ivf_slice_walk<B, IvfF16>(smem, s_begin, s_end, nk, ivf_live_blocks<B>(npair), fetch, fold);
  if constexpr (!EMIT) {
#pragma unroll
    for (int bi = 0; bi < NR; ++bi)
      if (hits[bi]) atomicAdd(&scnt[row0 + bi * 16], (unsigned)hits[bi]);
    __syncthreads();
    if (tid < npair) pair_counts[spair[tid]] = (int32_t)scnt[tid];
  }
}

// ---------------------------------------------------------------- int8 lists (comment: ivf.hip)
// The query keys [B] go behind the query scales.
template <int KT, int B>
__global__ __launch_bounds__(IVF_TB) void IVF_TWIN(ivf_i8_scan_lists_kernel)(const int8_t* __restrict__ qc, const float* __restrict__ qscale,
                                                                   int d, int nq, int nprobe, const int8_t* __restrict__ rows,
                                                                   const float* __restrict__ scales,
                                                                   const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ off, int K,
                                                                   const int32_t* __restrict__ poff,
                                                                   const int32_t* __restrict__ ubase,
                                                                   const int32_t* __restrict__ pairs, int k_out,
                                                                   float* __restrict__ ps, int32_t* __restrict__ pi IVF_TWIN_PARAM) {
  constexpr int OPB = B * IVF_I8_BK;  // bytes of one operand's K slice
  constexpr int NR = B / 32;          // 16-row blocks of a wave per operand
  constexpr int NL = B / IVF_I8_RP;   // rows of an operand slice a thread loads
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lists = (unsigned long long*)(smem + 4 * OPB);
  int* spair = (int*)(smem + 4 * OPB + B * KT * 8);
  float* sqs = (float*)(spair + B);  // the pairs' query scales
  IvfKeyTest<B, IVF_TWIN_KEYS> keys(IVF_TWIN_KEYARGS, sqs + B);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, kg = lane >> 4, wr = wave >> 1, wc = wave & 1;
  const int b = blockIdx.x;
  if (b >= ubase[K]) return;
  int lo = 0, hi = K;  // the last l in [0, K) with ubase[l] <= b; ubase[l + 1] > b follows from b < ubase[K]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ubase[mid] <= b) lo = mid;
    else hi = mid;
  }
  const int l = lo;
  const int p0 = poff[l] + (b - ubase[l]) * B;
  const int npair = min(B, poff[l + 1] - p0);
  const int s_begin = off[l], s_end = off[l + 1];
  ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [&](int pr) {
    sqs[tid] = pr >= 0 ? qscale[pr / nprobe] : 0.f;
    keys.pair(pr, nprobe);
  });
  keys.rows();

  const int nk = (d + IVF_I8_BK - 1) / IVF_I8_BK;
  const int ntiles = (s_end - s_begin + B - 1) / B;
  const int T = ntiles * nk;

  // this thread's rows of a slice, and where its chunk lands in LDS
  const int cc = tid % IVF_I8_CH;
  const int8_t* qsrc[NL];
  int lds_off[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int r = tid / IVF_I8_CH + IVF_I8_RP * j;
    const int pr = spair[r];
    qsrc[j] = pr >= 0 ? qc + (size_t)(pr / nprobe) * d + cc * 16 : nullptr;
    lds_off[j] = r * IVF_I8_BK + ((cc ^ (r & (IVF_I8_CH - 1))) << 4);
  }
  u32x4 qv[NL], lv[NL];
  auto load = [&](int it) {
    const int tile = it / nk, ks = it - tile * nk;
    const bool in_row = ks * IVF_I8_BK + cc * 16 < d;  // false for chunks 4 .. 7 of the last slice when d % 128 == 64
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int slot = s_begin + tile * B + tid / IVF_I8_CH + IVF_I8_RP * j;
      qv[j] = qsrc[j] && in_row ? *(const u32x4*)(qsrc[j] + ks * IVF_I8_BK) : u32x4{0u, 0u, 0u, 0u};
      lv[j] = slot < s_end && in_row ? *(const u32x4*)(rows + (size_t)slot * d + ks * IVF_I8_BK + cc * 16)
                                     : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      *(u32x4*)(smem + buf * 2 * OPB + lds_off[j]) = qv[j];
      *(u32x4*)(smem + buf * 2 * OPB + OPB + lds_off[j]) = lv[j];
    }
  };

  i32x4 acc[NR][NR];  // [slot block ai][pair block bi]
#pragma unroll
  for (int ai = 0; ai < NR; ++ai)
#pragma unroll
    for (int bi = 0; bi < NR; ++bi) acc[ai][bi] = i32x4{0, 0, 0, 0};
  // 16-pair blocks of this wave that hold a pair at all (wave-uniform)
  const int nb_live = min(NR, max(0, (npair - wc * (B / 2) + 15) / 16));

  if (T > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  int ks = 0, tile = 0;
  for (int it = 0; it < T; ++it) {
    const int buf = it & 1;
    if (it + 1 < T) load(it + 1);
    // 16-slot blocks of this wave below the end of the list (the lists are padded to 16 slots): wave-uniform
    const int slot_w = s_begin + tile * B + wr * (B / 2);
    const int na_live = min(NR, max(0, (s_end - slot_w) / 16));
    if (na_live > 0 && nb_live > 0) {
      const char* qs = smem + buf * 2 * OPB;
      const char* ls = qs + OPB;
#pragma unroll
      for (int kk = 0; kk < IVF_I8_BK / 64; ++kk) {
        const int ch = kk * 4 + kg;
        i32x4 fa[NR], fb[NR];
#pragma unroll
        for (int ai = 0; ai < NR; ++ai) {
          const int ra = wr * (B / 2) + ai * 16 + l15;
          fa[ai] = *(const i32x4*)(ls + ra * IVF_I8_BK + ((ch ^ (ra & (IVF_I8_CH - 1))) << 4));
        }
#pragma unroll
        for (int bi = 0; bi < NR; ++bi) {
          const int rb = wc * (B / 2) + bi * 16 + l15;
          fb[bi] = *(const i32x4*)(qs + rb * IVF_I8_BK + ((ch ^ (rb & (IVF_I8_CH - 1))) << 4));
        }
#pragma unroll
        for (int ai = 0; ai < NR; ++ai)
          if (ai < na_live) {
#pragma unroll
            for (int bi = 0; bi < NR; ++bi)
              if (bi < nb_live) acc[ai][bi] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[ai], fb[bi], acc[ai][bi], 0, 0, 0);
          }
      }
    }
    if (it + 1 < T) store(buf ^ 1);
    if (++ks == nk) {
      // the tile is finished: fold this wave's scores into the pairs' lists, as ivf_scan_lists_kernel does
#pragma unroll
      for (int ai = 0; ai < NR; ++ai) {
        if (ai < na_live) {
          const int slot0 = slot_w + ai * 16 + 4 * kg;  // < s_end, 16-byte aligned: off % 16 == 0
          const int4 id4 = *(const int4*)(ids + slot0);
          const float4 sc4 = *(const float4*)(scales + slot0);
          const int idr[4] = {id4.x, id4.y, id4.z, id4.w};
          const float scr[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
          keys.slots(slot0);
#pragma unroll
          for (int bi = 0; bi < NR; ++bi) {
            const int pr = wc * (B / 2) + bi * 16 + l15;
            if (pr < npair) {
              unsigned long long* lst = lists + pr * KT;
              const float sq = sqs[pr];
              const float thr = xs_unord(
                  (uint32_t)(__hip_atomic_load(lst + KT - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> 32));
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float v = __fmul_rn(__fmul_rn((float)acc[ai][bi][r], scr[r]), sq);
                if (idr[r] >= 0 && keys(bi, r) && v >= thr) xs_insert<KT>(lst, v, idr[r]);
              }
            }
          }
        }
#pragma unroll
        for (int bi = 0; bi < NR; ++bi) acc[ai][bi] = i32x4{0, 0, 0, 0};
      }
      ks = 0;
      ++tile;
    }
    __syncthreads();
  }

  // (the last barrier of the loop, or the one before it when the list is empty, made the lists final)
  if (tid < npair) {
    const int pr = spair[tid];
    const int q = pr / nprobe, p = pr - q * nprobe;
    const size_t o = ((size_t)p * nq + q) * k_out;
    for (int j = 0; j < k_out; ++j) {
      const unsigned long long key = lists[tid * KT + j];
      const bool have = key != XS_EMPTY;
      ps[o + j] = have ? xs_key_value(key) : -INFINITY;
      pi[o + j] = have ? xs_key_index(key) : -1;
    }
  }
}

// ---------------------------------------------------------------- product-quantised lists (comment: ivf.hip)
// The query keys [B] go behind the pair numbers, or behind the coarse terms where RES keeps them.
template <int KT, int B, bool RES>
__global__ __launch_bounds__(IVF_TB) void IVF_TWIN(ivf_pq_scan_lists_kernel)(const f16* __restrict__ qn, int d, int nq, int nprobe,
                                                                   const uint8_t* __restrict__ codes, int dshift,
                                                                   const f16* __restrict__ cb, const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ off, int K,
                                                                   const int32_t* __restrict__ poff,
                                                                   const int32_t* __restrict__ ubase,
                                                                   const int32_t* __restrict__ pairs, int k_out,
                                                                   float* __restrict__ ps, int32_t* __restrict__ pi,
                                                                   const float* __restrict__ coarse IVF_TWIN_PARAM) {
  constexpr int NR = B / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* lists = (unsigned long long*)(smem + 4 * B * IVF_SLICE);
  int* spair = (int*)(lists + B * KT);
  [[maybe_unused]] float* scoarse = (float*)(spair + B);  // RES only
  IvfKeyTest<B, IVF_TWIN_KEYS> keys(IVF_TWIN_KEYARGS, spair + (RES ? 2 * B : B));
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b >= ubase[K]) return;
  const int l = ivf_unit_list(ubase, K, b);
  const int p0 = poff[l] + (b - ubase[l]) * B;
  const int npair = min(B, poff[l + 1] - p0);
  const int s_begin = off[l], s_end = off[l + 1];
  if constexpr (RES) {
    ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [&](int pr) {
      scoarse[tid] = pr >= 0 ? coarse[pr] : 0.f;
      keys.pair(pr, nprobe);
    });
  } else {
    ivf_pairs_init<KT, B>(lists, spair, pairs, p0, npair, [&](int pr) { keys.pair(pr, nprobe); });
  }
  keys.rows();

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
  auto fetch_codes = [&](int it) {
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
    keys.slots(slot0);
    if constexpr (RES) {
      ivf_topk_fold<KT, B>(
          lists, npair, *(const int4*)(ids + slot0), acc,
          [scoarse](int pr) {
            const float c = scoarse[pr];
            return [c](float a, int) { return a + c; };
          },
          keys);
    } else {
      ivf_topk_fold<KT, B>(lists, npair, *(const int4*)(ids + slot0), acc, IvfSumIsScore{}, keys);
    }
  };
  ivf_slice_walk<B, IvfF16>(smem, s_begin, s_end, nk, ivf_live_blocks<B>(npair), fetch, fold);
  ivf_lists_readout<KT>(lists, spair, npair, nprobe, nq, k_out, ps, pi);
}
