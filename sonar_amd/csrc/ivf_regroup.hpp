// Regrouping of list-contiguous IVF storage (restated in tests/ivf_regroup_ref.py): the surviving slots of a
// filled index together with a set of new, already-encoded rows, into fresh storage of smi_ivf_build's layout.  One device
// operation behind `extend` (new rows), `remove` (survivors alone, on the effective ids of a row mask) and `merge_from` (the
// other index's slots as the new rows) of all five index classes: they share this storage -- payload rows of row_bytes
// bytes, one int32 id and at most one 32-bit aux value (scale, bias) per slot.
//
// The ITEMS of a call are the old slots 0 .. old_slots, then the new rows: item j < old_slots is old slot j, item
// old_slots + i is new row i.  An init kernel (list_sizes = 0, list_ids = -1), then four passes, the first three the build's
// bucketing (bucket.hpp) over the items' list numbers:
//   keys      the list of every item, -1 where it is left out: an old slot without a row (id < 0: a pad, an unused slot, a row
//             masked out) or from old_offsets[K] on; a new row whose label is outside [0, K) or whose given id is below 0.  The
//             list of an old slot is found in old_offsets by bisection (ivf_unit_list);
//   histogram + scan   list_sizes, list_offsets (aligned to IVF_ALIGN) and the cursor: bucket_hist_kernel, ivf_scan_kernel;
//   scatter   the SOURCE MAP, one item number per destination slot, -1 for a pad.  It is written into list_ids, which the
//             move then overwrites slot by slot with the ids themselves: no map in the workspace.  The build's scatter with
//             one more test: a position at or beyond `bound` is not written;
//   move      ivf_gather_kernel's shape, one wave per destination slot below min(list_offsets[K], bound): the payload (16
//             bytes per lane per access where row_bytes and the three bases allow it, else byte by byte), the aux value and
//             the id in the same pass; zeros, aux 0 and id -1 for a pad slot.
// `bound` = smi_ivf_slots_bound(old_rows_bound + n_new, K) <= capacity_slots is known to the host, so no store leaves the
// caller's buffers whatever the device data say: were there more survivors than old_rows_bound promises, the rows beyond
// the bound are dropped (list_offsets and list_sizes then still count them: the caller broke the contract).
// This header is included once, inside ivf.hip's unnamed namespace, behind every kernel the parent commit had.

// sizes[0 .. K) = 0 and ids[0 .. capacity) = -1: what the build does with two memsets.  A kernel here, because the entry
// is meant to be captured: with two hipMemsetAsync calls in their place (20 bytes of list_sizes at K = 5, then list_ids) a
// graph replay left garbage in list_sizes on this runtime, where the same call outside a graph was right
// (tests/test_gpu_ivf_regroup.py, test_regroup_is_capturable); with kernel nodes only, the replay is the direct call's result.
__global__ __launch_bounds__(IVF_TB) void ivf_regroup_init_kernel(int32_t* __restrict__ sizes, int K, int32_t* __restrict__ ids,
                                                                  int capacity) {
  const int64_t i = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  if (i < K) sizes[i] = 0;
  if (i < capacity) ids[i] = -1;
}

// keys[j] = the list of item j, or -1
__global__ __launch_bounds__(IVF_TB) void ivf_regroup_keys_kernel(const int32_t* __restrict__ old_ids,
                                                                  const int32_t* __restrict__ old_off, int old_slots,
                                                                  const int32_t* __restrict__ new_labels,
                                                                  const int32_t* __restrict__ new_ids, int n_new, int K,
                                                                  int32_t* __restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  if (j >= (int64_t)old_slots + n_new) return;
  int c = -1;
  if (j < old_slots) {
    if (j < old_off[K] && old_ids[j] >= 0) c = ivf_unit_list(old_off, K, (int)j);
  } else {
    const int64_t i = j - old_slots;
    c = new_labels[i];
    if (new_ids && new_ids[i] < 0) c = -1;
  }
  keys[j] = c;
}

// bucket_scatter_kernel with the positions bounded: out[pos] = j only for pos in [0, bound)
__global__ __launch_bounds__(IVF_TB) void ivf_regroup_scatter_kernel(const int32_t* __restrict__ keys, int n, int K,
                                                                     int32_t* __restrict__ cursor, int32_t* __restrict__ out,
                                                                     int bound) {
  const int64_t j = (int64_t)blockIdx.x * IVF_TB + threadIdx.x;
  const int c = j < n ? keys[j] : -1;
  const bool ok = key_ok(c, K);
  const int pos = wave_claim(cursor, c, ok, threadIdx.x & 63);
  if (ok && (unsigned)pos < (unsigned)bound) out[pos] = (int32_t)j;
}

// One wave per destination slot below min(off[K], bound).  ids[slot] holds the slot's item number (the source map) on entry
// and its id on exit: every lane reads it in one instruction before lane 0 writes it.  An item number outside the items (the
// scatter writes none) reads nothing and gives a pad.  The aux values move as 32-bit words: their bits are kept.
template <bool V16>
__global__ __launch_bounds__(IVF_TB) void ivf_regroup_move_kernel(
    const uint8_t* __restrict__ old_rows, const uint32_t* __restrict__ old_aux, const int32_t* __restrict__ old_ids, int old_slots,
    const uint8_t* __restrict__ new_rows, const uint32_t* __restrict__ new_aux, const int32_t* __restrict__ new_ids,
    int new_id_base, int n_new, int row_bytes, const int32_t* __restrict__ off, int K, int bound, uint8_t* __restrict__ rows,
    uint32_t* __restrict__ aux, int32_t* ids) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * (IVF_TB / 64) + (threadIdx.x >> 6);
  if (slot >= off[K] || slot >= bound) return;  // wave-uniform
  const int src = ids[slot];
  const uint8_t* s = nullptr;
  uint32_t a = 0u;
  int id = -1;
  if (src >= 0 && src < old_slots) {
    s = old_rows + (size_t)src * row_bytes;
    a = old_aux ? old_aux[src] : 0u;
    id = old_ids[src];
  } else if (src >= old_slots && src - old_slots < n_new) {
    const int i = src - old_slots;
    s = new_rows + (size_t)i * row_bytes;
    a = new_aux ? new_aux[i] : 0u;
    id = new_ids ? new_ids[i] : new_id_base + i;
  }
  uint8_t* o = rows + (size_t)slot * row_bytes;
  if constexpr (V16) {
    u32x4* o16 = (u32x4*)o;
    const u32x4* s16 = (const u32x4*)s;
    if (s) {
      for (int c = lane; c < row_bytes / 16; c += 64) o16[c] = s16[c];
    } else {
      for (int c = lane; c < row_bytes / 16; c += 64) o16[c] = u32x4{0u, 0u, 0u, 0u};
    }
  } else {
    for (int c = lane; c < row_bytes; c += 64) o[c] = s ? s[c] : (uint8_t)0;
  }
  if (lane == 0) {
    if (aux) aux[slot] = a;
    ids[slot] = id;
  }
}

// regroup: cursor int32 [K] | keys int32 [old_slots + n_new]
struct RegroupWs : WsLayout {
  int32_t *cursor, *keys;
  RegroupWs(void* ws, int64_t items, int64_t K) : WsLayout(ws) {
    cursor = take<int32_t>(K, 16);
    keys = take<int32_t>(items, 16);
  }
};

// the refusals on the shapes the sizing function sees
int check_regroup_shape(int64_t old_slots, int64_t n_new, int64_t K) {
  if (K < 1) return fail(SMI_ERR_INVALID_ARG, "K=%lld: at least one list", (long long)K);
  if (old_slots < 0 || n_new < 0)
    return fail(SMI_ERR_INVALID_ARG, "old_slots=%lld, n_new=%lld: negative", (long long)old_slots, (long long)n_new);
  if (old_slots + n_new < 1) return fail(SMI_ERR_INVALID_ARG, "old_slots=0 and n_new=0: empty input on both sides");
  if (old_slots > IVF_MAX || n_new > IVF_MAX || K > IVF_MAX || old_slots + n_new > IVF_MAX)
    return fail(SMI_ERR_UNSUPPORTED, "old_slots=%lld, n_new=%lld, K=%lld: slot, row and list numbers must fit int32",
                (long long)old_slots, (long long)n_new, (long long)K);
  return SMI_OK;
}

int regroup_entry(const void* old_rows, const float* old_aux, const int32_t* old_ids, const int32_t* old_offsets, int64_t old_slots,
                  int64_t old_rows_bound, const void* new_rows, const float* new_aux, const int32_t* new_labels,
                  const int32_t* new_ids, int32_t new_id_base, int64_t n_new, int32_t row_bytes, int64_t K, void* list_rows,
                  float* list_aux, int32_t* list_ids, int64_t capacity_slots, int32_t* list_offsets, int32_t* list_sizes, void* ws,
                  int64_t ws_bytes, void* stream) {
  if (!list_rows || !list_ids || !list_offsets || !list_sizes) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (const int rc = check_regroup_shape(old_slots, n_new, K)) return rc;
  if (row_bytes < 1) return fail(SMI_ERR_INVALID_ARG, "row_bytes=%d: at least one byte per row", row_bytes);
  if (old_slots > 0 && (!old_rows || !old_ids || !old_offsets))
    return fail(SMI_ERR_INVALID_ARG, "null old_rows, old_ids or old_offsets with old_slots=%lld", (long long)old_slots);
  if (n_new > 0 && (!new_rows || !new_labels))
    return fail(SMI_ERR_INVALID_ARG, "null new_rows or new_labels with n_new=%lld", (long long)n_new);
  if (old_rows_bound < 0 || old_rows_bound > old_slots)
    return fail(SMI_ERR_INVALID_ARG, "old_rows_bound=%lld must be in [0, old_slots=%lld]", (long long)old_rows_bound,
                (long long)old_slots);
  if ((old_slots > 0 && !old_aux != !list_aux) || (n_new > 0 && !new_aux != !list_aux))
    return fail(SMI_ERR_INVALID_ARG, "old_aux, new_aux and list_aux go together: all of the sides that have rows, or none");
  if (new_id_base < 0 || new_id_base + n_new > IVF_MAX)
    return fail(SMI_ERR_UNSUPPORTED, "new_id_base=%d + n_new=%lld: row ids must fit int32", new_id_base, (long long)n_new);
  if (list_rows == old_rows || list_rows == new_rows || list_ids == old_ids || list_ids == new_ids ||
      list_offsets == old_offsets || (list_aux && (list_aux == old_aux || list_aux == new_aux)))
    return fail(SMI_ERR_INVALID_ARG, "the output storage must not be an input: the regroup is not in place");
  const int64_t rows_bound = old_rows_bound + n_new;
  const int64_t bound = slots_bound(rows_bound, K);
  if (bound > IVF_MAX)
    return fail(SMI_ERR_UNSUPPORTED, "%lld rows over K=%lld lists can need %lld slots: slot numbers must fit int32",
                (long long)rows_bound, (long long)K, (long long)bound);
  if (capacity_slots < bound || capacity_slots < 1 || capacity_slots > IVF_MAX)
    return fail(SMI_ERR_INVALID_ARG, "capacity of %lld slots, smi_ivf_slots_bound(old_rows_bound + n_new, K) = %lld",
                (long long)capacity_slots, (long long)bound);
  const int64_t items = old_slots + n_new;
  const RegroupWs w(ws, items, K);
  if (const int rc = check_ws(ws, ws_bytes, w.bytes(), "smi_lists_regroup_ws_bytes(old_slots, n_new, K)")) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(IVF_TB), items_grid = grid_for(items, IVF_TB);
  hipLaunchKernelGGL(ivf_regroup_init_kernel, grid_for(std::max(K, capacity_slots), IVF_TB), block, 0, st, list_sizes, (int)K,
                     list_ids, (int)capacity_slots);
  hipLaunchKernelGGL(ivf_regroup_keys_kernel, items_grid, block, 0, st, old_ids, old_offsets, (int)old_slots, new_labels, new_ids,
                     (int)n_new, (int)K, w.keys);
  hipLaunchKernelGGL(bucket_hist_kernel<IVF_TB>, items_grid, block, 0, st, (const int32_t*)w.keys, (int)items, (int)K, list_sizes);
  hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), block, 0, st, (const int32_t*)list_sizes, (int)K, IVF_ALIGN, 1, list_offsets,
                     w.cursor, (int32_t*)nullptr);
  if (bound > 0) {
    hipLaunchKernelGGL(ivf_regroup_scatter_kernel, items_grid, block, 0, st, (const int32_t*)w.keys, (int)items, (int)K, w.cursor,
                       list_ids, (int)bound);
    const bool v16 = row_bytes % 16 == 0 && (uintptr_t)old_rows % 16 == 0 && (uintptr_t)new_rows % 16 == 0 &&
                     (uintptr_t)list_rows % 16 == 0;
    const auto move = v16 ? ivf_regroup_move_kernel<true> : ivf_regroup_move_kernel<false>;
    hipLaunchKernelGGL(move, grid_for(bound, IVF_TB / 64), block, 0, st, (const uint8_t*)old_rows, (const uint32_t*)old_aux, old_ids,
                       (int)old_slots, (const uint8_t*)new_rows, (const uint32_t*)new_aux, new_ids, new_id_base, (int)n_new,
                       row_bytes, (const int32_t*)list_offsets, (int)K, (int)bound, (uint8_t*)list_rows, (uint32_t*)list_aux,
                       list_ids);
  }
  HIP_TRY(hipGetLastError());
  return SMI_OK;
}
