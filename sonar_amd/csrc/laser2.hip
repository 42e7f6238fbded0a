// LASER2 BiLSTM sentence encoder (sonar/nn/laser_lstm_encoder.py, arch `laser2` of models/laser2_text/config.py).
//
// Layout: the batch is sorted by length, descending (PackedSequence order), and every activation is TIME-MAJOR PACKED:
// step t holds active(t) = #{len > t} rows, a prefix of the sorted batch, at packed rows off(t) .. off(t) + active(t).
// Padded positions cost neither projection nor recurrence work.
//
//   laser2_embed_kernel    packed x0 [T][Ep] fp16 <- embedding rows (ids outside [0, vocab) raise *bad, never read)
//   (GEMM engines)         pre [T][G] fp32 = x . W_ih^T + (b_ih + b_hh), both directions in one product (G = ndir * 4Hp)
//   lstm_step_kernel       one launch per (layer, step) covers both directions: gates = pre + h_prev . W_hh^T (fp16 MFMA,
//                          fp32 accumulation), cell update in the read-out (fp32 c), h -> next layer's packed input and the
//                          h_prev double buffer, or (last layer) a running fp32 max with -inf where the token is pad_idx
//   laser2_finalize_kernel padding_value for rows with non-pad tokens at or beyond their length, un-sort to [n, units]
//
// Packed gate-column order (W_ih rows, bias, `pre` columns, W_hh rows): for direction d, unit tile j (16 hidden units),
// gate q (i, f, g, o), unit u of the tile: column d*4Hp + j*64 + q*16 + u.  One output tile of the recurrent product thus
// holds i, f, g, o of the same 16 hidden units, and each lane owns the same (row, unit) in all four gate accumulators.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "api_common.hpp"

namespace smi {

namespace {

constexpr int kUnits = 16;     // hidden units per output tile (x 4 gates = 64 columns)
constexpr int kWaveRows = 32;  // sorted-batch rows per wave (two 16-row MFMA blocks)
constexpr int kBlockRows = 4 * kWaveRows;

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// x0[off[t] + b][:] = table[ids[order[b] * s + t]][:] for b < active(t); pad[off[t] + b] = (id == pad_idx)
// meta = order[n] | sorted lengths[n] | off[s + 1]
__global__ __launch_bounds__(256) void laser2_embed_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ meta,
                                                           int n, int s, const f16* __restrict__ table, int64_t vocab, int ep,
                                                           int pad_idx, f16* __restrict__ x, uint8_t* __restrict__ pad,
                                                           int32_t* bad) {
  const int32_t* order = meta;
  const int32_t* off = meta + 2 * n;
  const int t = blockIdx.x;
  const int active = off[t + 1] - off[t];
  const int vecs = ep / 8;
  for (int b = blockIdx.y * 4 + (threadIdx.x >> 6); b < active; b += gridDim.y * 4) {
    const int64_t id = ids[(int64_t)order[b] * s + t];
    const int64_t p = off[t] + b;
    const bool ok = id >= 0 && id < vocab;
    if ((threadIdx.x & 63) == 0) {
      pad[p] = id == pad_idx;
      if (!ok) *bad = 1;
    }
    for (int v = threadIdx.x & 63; v < vecs; v += 64) {
      half8 val = {};
      if (ok) val = *(const half8*)(table + id * ep + v * 8);
      *(half8*)(x + p * ep + v * 8) = val;
    }
  }
}

struct StepArgs {
  const float* pre;     // [T][G] fp32 preactivations (bias folded in)
  int G;                // ndir * 4 * hp
  const f16* whh;       // [ndir][4hp][hp] packed
  const f16* h_prev;    // [ndir][bcap][hp] (not read at step 0)
  f16* h_next;          // [ndir][bcap][hp]
  float* c;             // [ndir][bcap][hp]
  f16* xout;            // next layer's packed input [T][ldx], or null (last layer)
  int ldx;
  float* runmax;        // [ndir][bcap][hp] (last layer) or null
  const uint8_t* pad;   // [T] token == pad_idx, per packed row
  const int32_t* lens;  // [n] sorted lengths
  const int32_t* off;   // [s + 1]
  int hp, bcap, step, active;
};

// One (layer, step): grid (hp / 16, ceil(active / 128), ndir); 4 waves of 32 sorted rows each, all on the same 16 units.
__global__ __launch_bounds__(256) void lstm_step_kernel(StepArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x, d = blockIdx.z;
  const int b0 = blockIdx.y * kBlockRows + wave * kWaveRows;
  if (b0 >= a.active) return;
  const int hp = a.hp;
  // the step's preactivations do not depend on the recurrence: issue their loads before the K loop
  const int u = j * kUnits + (lane & 15);
  const int col = d * 4 * hp + j * 64 + (lane & 15);
  float pre[2][4][4];
  int64_t prow[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = b0 + m * 16 + (lane >> 4) * 4 + e;
      prow[m][e] = -1;
      if (b < a.active) {
        // forward: time = step; reverse: each row starts at its own last valid token
        const int t = d == 0 ? a.step : a.lens[b] - 1 - a.step;
        prow[m][e] = a.off[t] + b;
        const float* pr = a.pre + prow[m][e] * a.G + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[m][e][q] = pr[q * 16];
      }
    }
  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[m][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.step > 0) {
    // A = h_prev rows (row l & 15 of each 16-row block), B = W_hh^T columns (unit l & 15 of each gate); k = 8 (l >> 4) + e
    const int kq = (lane >> 4) * 8;
    const f16* hb = a.h_prev + ((size_t)d * a.bcap + b0 + (lane & 15)) * hp + kq;
    const bool r0 = b0 + (lane & 15) < a.active, r1 = b0 + 16 + (lane & 15) < a.active;
    const f16* wb = a.whh + ((size_t)d * 4 * hp + (size_t)j * 64 + (lane & 15)) * hp + kq;
    for (int k0 = 0; k0 < hp; k0 += 32) {
      half8 x0 = {}, x1 = {};
      if (r0) x0 = *(const half8*)(hb + k0);
      if (r1) x1 = *(const half8*)(hb + (size_t)16 * hp + k0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const half8 w = *(const half8*)(wb + (size_t)q * 16 * hp + k0);
        acc[0][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x0, w, acc[0][q], 0, 0, 0);
        acc[1][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, w, acc[1][q], 0, 0, 0);
      }
    }
  }
  // read-out: the lane owns unit u = 16 j + (l & 15) and sorted rows b0 + 16 m + 4 (l >> 4) + e
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = b0 + m * 16 + (lane >> 4) * 4 + e;
      const int64_t p = prow[m][e];
      if (p < 0) continue;
      const float gi = sigmoidf_(acc[m][0][e] + pre[m][e][0]);
      const float gf = sigmoidf_(acc[m][1][e] + pre[m][e][1]);
      const float gg = tanhf(acc[m][2][e] + pre[m][e][2]);
      const float go = sigmoidf_(acc[m][3][e] + pre[m][e][3]);
      const size_t si = ((size_t)d * a.bcap + b) * hp + u;
      const float cp = a.step > 0 ? a.c[si] : 0.f;
      const float cn = gf * cp + gi * gg;
      const float hn = go * tanhf(cn);
      a.c[si] = cn;
      a.h_next[si] = (f16)hn;
      if (a.xout) a.xout[p * a.ldx + d * hp + u] = (f16)hn;
      if (a.runmax) {  // max over time; a pad_idx token contributes -inf (laser_lstm_encoder.py:105-114)
        const float mp = a.step > 0 ? a.runmax[si] : -INFINITY;
        a.runmax[si] = a.pad[p] ? mp : fmaxf(mp, hn);
      }
    }
  }
}

// out[order[b]][d*H + u] = max(runmax[d][b][u], padding_value if row b has a non-pad token at or beyond its length)
__global__ __launch_bounds__(256) void laser2_finalize_kernel(const float* __restrict__ runmax, const int64_t* __restrict__ ids,
                                                              const int32_t* __restrict__ meta, int n, int s, int pad_idx,
                                                              float padding_value, int hidden, int hp, int ndir, int bcap,
                                                              float* __restrict__ out) {
  const int b = blockIdx.x;
  const int orig = meta[b], len = meta[n + b];
  int tail = 0;
  for (int t = len + threadIdx.x; t < s; t += blockDim.x) tail |= ids[(int64_t)orig * s + t] != pad_idx;
  tail = __syncthreads_or(tail);
  const int units = ndir * hidden;
  for (int i = threadIdx.x; i < units; i += blockDim.x) {
    const int d = i / hidden, u = i - d * hidden;
    float v = runmax[((size_t)d * bcap + b) * hp + u];
    if (tail) v = fmaxf(v, padding_value);
    out[(size_t)orig * units + i] = v;
  }
}

}  // namespace
}  // namespace smi

using namespace smi;
using smi_host::DevBuf;
using smi_host::fail;
using smi_host::round_up;

struct smi_laser2 {
  smi_laser2_config cfg{};
  int ndir = 1, hp = 0, ep = 0, kl = 0, G = 0;
  DevBuf embed;                        // [vocab][ep] fp16
  std::vector<DevBuf> wih, bias, whh;  // per layer: [G][k_in] fp16, [G] fp32, [ndir][4hp][hp] fp16
  // workspace (grow-only)
  int64_t cap_tokens = 0;
  int cap_rows = 0;
  size_t cap_meta = 0;
  DevBuf x0, seq[2], pre, padm, hbuf, cbuf, runmax, meta;
  int32_t* meta_h = nullptr;  // pinned staging words of `meta`
  hipEvent_t meta_ev = nullptr;
  int32_t* bad = nullptr;      // pinned host word: sticky out-of-vocabulary flag (cleared by smi_laser2_status)
  int32_t* bad_dev = nullptr;  // its device address
  ~smi_laser2() {
    if (meta_h) (void)hipHostFree(meta_h);
    if (meta_ev) (void)hipEventDestroy(meta_ev);
    if (bad) (void)hipHostFree(bad);
  }
  int64_t bytes() const {
    int64_t t = embed.bytes + x0.bytes + seq[0].bytes + seq[1].bytes + pre.bytes + padm.bytes + hbuf.bytes + cbuf.bytes +
                runmax.bytes + meta.bytes;
    for (auto* v : {&wih, &bias, &whh})
      for (auto& b : *v) t += b.bytes;
    return t;
  }
};

namespace {

// A caller tensor (host or device, fp32 or fp16) -> host fp32
int fetch(const smi_tensor& t, int64_t expect, std::vector<float>& dst, const char* name, int layer) {
  if (!t.data) return fail(SMI_ERR_INVALID_ARG, "layer %d: weight %s: null data", layer, name);
  if (t.numel != expect)
    return fail(SMI_ERR_INVALID_ARG, "layer %d: weight %s: numel %lld, expected %lld", layer, name, (long long)t.numel,
                (long long)expect);
  if (t.dtype != SMI_F32 && t.dtype != SMI_F16) return fail(SMI_ERR_INVALID_ARG, "weight %s: bad dtype %d", name, t.dtype);
  const size_t es = t.dtype == SMI_F32 ? 4 : 2;
  std::vector<char> raw((size_t)expect * es);
  if (t.on_device)
    HIP_TRY(hipMemcpy(raw.data(), t.data, raw.size(), hipMemcpyDeviceToHost));
  else
    std::memcpy(raw.data(), t.data, raw.size());
  dst.resize(expect);
  for (int64_t i = 0; i < expect; ++i)
    dst[i] = t.dtype == SMI_F32 ? ((const float*)raw.data())[i] : (float)((const _Float16*)raw.data())[i];
  return SMI_OK;
}

template <typename T>
int put(DevBuf& dst, const std::vector<T>& v) {
  HIP_TRY(dst.alloc(v.size() * sizeof(T)));
  HIP_TRY(hipMemcpy(dst.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return SMI_OK;
}

// packed gate column of (direction d, gate q, hidden unit u) -- see the file comment
inline int gate_col(int d, int q, int u, int hp) { return d * 4 * hp + (u / kUnits) * 64 + q * kUnits + u % kUnits; }

int ensure_workspace(smi_laser2* L, int64_t tokens, int rows, int s) {
  const int64_t tpad = (tokens + 255) / 256 * 256;
  if (tpad > L->cap_tokens) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(L->x0.alloc((size_t)tpad * L->ep * 2));
    HIP_TRY(hipMemset(L->x0.p, 0, L->x0.bytes));
    for (auto& b : L->seq) {
      HIP_TRY(b.alloc((size_t)tpad * L->kl * 2));
      HIP_TRY(hipMemset(b.p, 0, b.bytes));  // the pad columns [ndir*hp, kl) stay zero
    }
    HIP_TRY(L->pre.alloc((size_t)tpad * L->G * 4));
    HIP_TRY(L->padm.alloc((size_t)tpad));
    L->cap_tokens = tpad;
  }
  if (rows > L->cap_rows) {
    HIP_TRY(hipDeviceSynchronize());
    const int r = round_up(rows, kBlockRows);
    HIP_TRY(L->hbuf.alloc((size_t)2 * L->ndir * r * L->hp * 2));
    HIP_TRY(hipMemset(L->hbuf.p, 0, L->hbuf.bytes));
    HIP_TRY(L->cbuf.alloc((size_t)L->ndir * r * L->hp * 4));
    HIP_TRY(L->runmax.alloc((size_t)L->ndir * r * L->hp * 4));
    L->cap_rows = r;
  }
  const size_t words = (size_t)2 * rows + s + 1;
  if (words > L->cap_meta) {
    HIP_TRY(hipDeviceSynchronize());
    if (L->meta_h) (void)hipHostFree(L->meta_h);
    L->meta_h = nullptr;
    L->cap_meta = 0;
    const size_t w = std::max<size_t>(words, 4096);
    HIP_TRY(hipHostMalloc((void**)&L->meta_h, w * 4, hipHostMallocDefault));
    HIP_TRY(L->meta.alloc(w * 4));
    L->cap_meta = w;
  }
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_laser2_create(const smi_laser2_config* cfg, const smi_tensor* embed, const smi_laser2_layer* layers,
                      int64_t max_tokens_hint, smi_laser2** out) {
  if (!cfg || !embed || !layers || !out) return fail(SMI_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const smi_laser2_config& c = *cfg;
  if (c.vocab_size <= 0 || c.embed_dim <= 0 || c.hidden_size <= 0 || c.num_layers <= 0 || c.num_layers > 64 ||
      (c.bidirectional != 0 && c.bidirectional != 1) || c.hidden_size > 8192 || c.embed_dim > 8192 || c.pad_idx < 0 ||
      c.pad_idx >= c.vocab_size)
    return fail(SMI_ERR_INVALID_ARG, "bad laser2 config (vocab %lld, pad %d, embed %d, hidden %d, layers %d, bidirectional %d)",
                (long long)c.vocab_size, c.pad_idx, c.embed_dim, c.hidden_size, c.num_layers, c.bidirectional);
  if (!smi_host::have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  auto* L = new smi_laser2();
  L->cfg = c;
  L->ndir = c.bidirectional ? 2 : 1;
  const int H = c.hidden_size, E = c.embed_dim, nd = L->ndir;
  // zero padding to the kernels' granularity is exact: a padded unit has zero weights and bias, so i = f = o = 1/2 and
  // g = 0, c = h = 0 throughout, and its zero columns add nothing to the next layer
  L->hp = round_up(H, 32);
  L->ep = round_up(E, 64);
  L->kl = round_up(nd * L->hp, 64);
  L->G = nd * 4 * L->hp;
  const int hp = L->hp, G = L->G;
  int rc = SMI_OK;
  {
    std::vector<float> e;
    rc = fetch(*embed, c.vocab_size * E, e, "embed_tokens", -1);
    if (rc == SMI_OK) {
      std::vector<f16> p((size_t)c.vocab_size * L->ep, (f16)0.f);
      for (int64_t v = 0; v < c.vocab_size; ++v)
        for (int k = 0; k < E; ++k) p[v * L->ep + k] = (f16)e[v * E + k];
      rc = put(L->embed, p);
    }
  }
  for (int l = 0; l < c.num_layers && rc == SMI_OK; ++l) {
    const int in = l == 0 ? E : nd * H;
    const int kin = l == 0 ? L->ep : L->kl;
    std::vector<f16> wih((size_t)G * kin, (f16)0.f), whh((size_t)G * hp, (f16)0.f);
    std::vector<float> bias(G, 0.f);
    for (int d = 0; d < nd && rc == SMI_OK; ++d) {
      const smi_laser2_layer& w = layers[(size_t)l * nd + d];
      std::vector<float> wi, wh, bi, bh;
      if ((rc = fetch(w.weight_ih, (int64_t)4 * H * in, wi, "weight_ih", l)) != SMI_OK) break;
      if ((rc = fetch(w.weight_hh, (int64_t)4 * H * H, wh, "weight_hh", l)) != SMI_OK) break;
      if ((rc = fetch(w.bias_ih, 4 * H, bi, "bias_ih", l)) != SMI_OK) break;
      if ((rc = fetch(w.bias_hh, 4 * H, bh, "bias_hh", l)) != SMI_OK) break;
      for (int q = 0; q < 4; ++q)
        for (int u = 0; u < H; ++u) {
          const int r = q * H + u, gc = gate_col(d, q, u, hp);
          bias[gc] = bi[r] + bh[r];
          for (int k = 0; k < in; ++k) {
            // input column k of a layer >= 1 is unit k % H of direction k / H: packed at (k / H) * hp + k % H
            const int kc = l == 0 ? k : (k / H) * hp + k % H;
            wih[(size_t)gc * kin + kc] = (f16)wi[(size_t)r * in + k];
          }
          for (int k = 0; k < H; ++k) whh[(size_t)gc * hp + k] = (f16)wh[(size_t)r * H + k];
        }
    }
    if (rc != SMI_OK) break;
    L->wih.emplace_back();
    L->bias.emplace_back();
    L->whh.emplace_back();
    if ((rc = put(L->wih.back(), wih)) != SMI_OK) break;
    if ((rc = put(L->bias.back(), bias)) != SMI_OK) break;
    rc = put(L->whh.back(), whh);
  }
  if (rc == SMI_OK) {
    hipError_t e = hipHostMalloc((void**)&L->bad, sizeof(int32_t), hipHostMallocMapped);
    if (e == hipSuccess) {
      *L->bad = 0;
      e = hipHostGetDevicePointer((void**)&L->bad_dev, L->bad, 0);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L->meta_ev, hipEventDisableTiming);
    if (e != hipSuccess) rc = fail(SMI_ERR_HIP, "laser2 create: %s", hipGetErrorString(e));
  }
  if (rc == SMI_OK) rc = ensure_workspace(L, std::max<int64_t>(max_tokens_hint, 1), 1, 1);
  if (rc != SMI_OK) {
    delete L;
    return rc;
  }
  *out = L;
  return SMI_OK;
}

void smi_laser2_destroy(smi_laser2* h) {
  if (!h) return;
  (void)hipDeviceSynchronize();
  delete h;
}

int64_t smi_laser2_device_bytes(const smi_laser2* h) { return h ? h->bytes() : 0; }

int smi_laser2_forward(smi_laser2* L, const int64_t* ids, const int32_t* seq_lens, int32_t n, int32_t s, float* out,
                       void* stream_v) {
  if (!L || !ids || !seq_lens || !out) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (n <= 0 || s <= 0) return fail(SMI_ERR_INVALID_ARG, "batch %d x %d", n, s);
  int max_len = 0;
  int64_t tokens = 0;
  for (int i = 0; i < n; ++i) {
    if (seq_lens[i] <= 0 || seq_lens[i] > s)
      return fail(SMI_ERR_INVALID_ARG, "seq_lens[%d]=%d outside [1,%d]", i, seq_lens[i], s);
    max_len = std::max(max_len, seq_lens[i]);
    tokens += seq_lens[i];
  }
  // pad_packed_sequence pads to max(seq_lens); the reference asserts that equals seqs.size(1) (laser_lstm_encoder.py:86)
  if (max_len != s) return fail(SMI_ERR_INVALID_ARG, "max(seq_lens)=%d differs from the batch width %d", max_len, s);
  if (!smi_host::have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  hipStream_t stream = (hipStream_t)stream_v;
  if (int rc = ensure_workspace(L, tokens, n, s)) return rc;
  const int nd = L->ndir, hp = L->hp, G = L->G, H = L->cfg.hidden_size;

  // sort by length, descending (stable: ties keep their input order), and the packed step offsets
  HIP_TRY(hipEventSynchronize(L->meta_ev));  // the previous forward's copy of the staging words has been made
  int32_t* order = L->meta_h;
  int32_t* slen = order + n;
  int32_t* off = slen + n;
  std::vector<int32_t> idx(n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return seq_lens[a] > seq_lens[b]; });
  for (int i = 0; i < n; ++i) {
    order[i] = idx[i];
    slen[i] = seq_lens[idx[i]];
  }
  std::vector<int> active(s);
  off[0] = 0;
  for (int t = 0, b = n; t < s; ++t) {
    while (b > 0 && slen[b - 1] <= t) --b;
    active[t] = b;
    off[t + 1] = off[t] + b;
  }
  HIP_TRY(hipMemcpyAsync(L->meta.p, L->meta_h, ((size_t)2 * n + s + 1) * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(L->meta_ev, stream));
  const int32_t* meta_d = L->meta.as<int32_t>();

  hipLaunchKernelGGL(laser2_embed_kernel, dim3(s, std::min(64, (n + 3) / 4)), dim3(256), 0, stream, ids, meta_d, n, s,
                     L->embed.as<f16>(), (int64_t)L->cfg.vocab_size, L->ep, L->cfg.pad_idx, L->x0.as<f16>(),
                     L->padm.as<uint8_t>(), L->bad_dev);
  HIP_TRY(hipGetLastError());
  const int M = (int)((tokens + 255) / 256 * 256);
  const f16* xin = L->x0.as<f16>();
  int kin = L->ep;
  for (int l = 0; l < L->cfg.num_layers; ++l) {
    const bool last = l + 1 == L->cfg.num_layers;
    HIP_TRY(launch_gemm_tn(EPI_STORE_F32, xin, L->wih[l].as<f16>(), L->bias[l].as<float>(), L->pre.p, M, G, kin, G, stream));
    f16* xout = last ? nullptr : L->seq[l & 1].as<f16>();
    StepArgs a;
    a.pre = L->pre.as<float>();
    a.G = G;
    a.whh = L->whh[l].as<f16>();
    a.c = L->cbuf.as<float>();
    a.xout = xout;
    a.ldx = L->kl;
    a.runmax = last ? L->runmax.as<float>() : nullptr;
    a.pad = L->padm.as<uint8_t>();
    a.lens = meta_d + n;
    a.off = meta_d + 2 * n;
    a.hp = hp;
    a.bcap = L->cap_rows;
    for (int st = 0; st < s; ++st) {
      a.h_prev = L->hbuf.as<f16>() + (size_t)((st + 1) & 1) * nd * L->cap_rows * hp;
      a.h_next = L->hbuf.as<f16>() + (size_t)(st & 1) * nd * L->cap_rows * hp;
      a.step = st;
      a.active = active[st];
      hipLaunchKernelGGL(lstm_step_kernel, dim3(hp / kUnits, (active[st] + kBlockRows - 1) / kBlockRows, nd), dim3(256), 0,
                         stream, a);
      HIP_TRY(hipGetLastError());
    }
    xin = xout;
    kin = L->kl;
  }
  hipLaunchKernelGGL(laser2_finalize_kernel, dim3(n), dim3(256), 0, stream, L->runmax.as<float>(), ids, meta_d, n, s,
                     L->cfg.pad_idx, L->cfg.padding_value, H, hp, nd, L->cap_rows, out);
  HIP_TRY(hipGetLastError());
  return SMI_OK;
}

int smi_laser2_status(smi_laser2* L, void* stream) {
  if (!L) return fail(SMI_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (L->bad && *(volatile int32_t*)L->bad) {
    *L->bad = 0;
    return fail(SMI_ERR_INVALID_ARG, "token ids outside [0, %lld) reached the LASER2 encoder (vocabulary / tokenizer mismatch)",
                (long long)L->cfg.vocab_size);
  }
  return SMI_OK;
}

}  // extern "C"
