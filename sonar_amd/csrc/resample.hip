// Sample-rate conversion of a ragged batch of clips in one launch (include/sonar_mi355.h, smi_resample_*).
//
// The filter is the windowed-sinc polyphase resampler torchaudio's functional.resample applies by default
// (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).  With o = orig / gcd, n = new / gcd:
//   base = min(o, n) * 0.99, width = ceil(6 o / base), taps = 2 width + o
//   k[p][i] = sinc(t) * cos(pi t / 12)^2 * base / o,  t = ((i - width) / o - p / n) * base clamped to [-6, 6]
//   y[m n + p] = sum_i k[p][i] * x[m o + i - width]   (x zero outside the clip)
// Per phase only S = floor(12 o / base) + 1 consecutive taps are non-zero in fp32 (outside them the window is cos(pi/2)^2);
// the host builds that compact [n][S] table and the first tap index of every phase in double precision, once per (o, n).
//
// Kernel: a workgroup owns a tile of consecutive outputs of ONE clip.  It stages the table (rows padded to an odd stride)
// and the tile's input span (zero-filled outside the clip) in LDS.  A thread then owns up to 8 outputs of ONE phase (they
// lie a multiple of n apart), so a tap is read once for all of them and 8 independent accumulators hide the LDS latency.
// Every output is accumulated over its taps in ascending order with one fmaf each -- so a value depends on its clip, the
// two rates and its index alone, never on the tile, the batch or where the operands were read from (a table or span too
// large for LDS is read through L2 instead, by the same arithmetic).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <tuple>
#include <vector>

#include "api_common.hpp"

using namespace smi_host;

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_GROUP = 8;           // outputs of one phase per thread
constexpr int RS_TILE = RS_THREADS * RS_GROUP;  // outputs per workgroup: the 21 KB table of 44.1 -> 16 kHz is staged once per 8 KB of output
constexpr int RS_STAGE = 8;           // 16-byte loads a thread keeps in flight while it stages a tile
constexpr int RS_LDS_WORDS = 15872;   // at most 62 KiB of the 160 KiB per CU; a launch asks for what its clips need
constexpr int RS_TAB_WORDS = 9216;    // the table goes to LDS up to 36 KiB (11.025 -> 16 kHz: 35 KiB); the rest is the span
constexpr int RS_MAX_RATE = 1 << 20;
constexpr int64_t RS_MAX_TABLE_BYTES = 16ll << 20;

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum : int32_t { RS_COPY = 1, RS_TAB_LDS = 2, RS_SPAN_LDS = 4 };

struct RsClip {
  int64_t in_begin, in_end;    // the clip's samples in `waves`
  int64_t out_begin, out_len;  // its outputs in `out`
  int64_t tile0;               // first workgroup of the clip
  const float* taps;           // device [n][S | 1]: the rows padded to an odd stride (LDS banks), then
  const int32_t* first;        // device [n], behind the taps in the same allocation
  int32_t o, n, S, width, tile, flags;
};

struct Filter {
  int o = 0, n = 0, width = 0, S = 0;
  std::vector<float> taps;     // [n][S]
  std::vector<int32_t> first;  // [n]
};

struct DevFilter {
  DevBuf buf;  // [n][S | 1] taps, [n] first tap indices, zeros up to a multiple of 16 bytes: the image of the LDS copy
};

std::mutex g_rs_mu;
std::map<std::pair<int, int>, Filter>& filters() {
  static std::map<std::pair<int, int>, Filter> m;
  return m;
}
std::map<std::tuple<int, int, int>, DevFilter>& dev_filters() {
  static std::map<std::tuple<int, int, int>, DevFilter> m;
  return m;
}

struct Shape {
  int o, n, width, S;
  double base;
};

Shape filter_shape(int orig, int nw) {
  const int g = std::gcd(orig, nw);
  Shape s;
  s.o = orig / g;
  s.n = nw / g;
  s.base = std::min(s.o, s.n) * 0.99;
  s.width = (int)std::ceil(6.0 * s.o / s.base);
  s.S = (int)std::floor(12.0 * s.o / s.base) + 1;
  return s;
}

int check_rates(int orig, int nw) {
  if (orig <= 0 || nw <= 0)
    return fail(SMI_ERR_UNSUPPORTED, "resampling %d Hz -> %d Hz: sample rates must be positive", orig, nw);
  if (orig > RS_MAX_RATE || nw > RS_MAX_RATE)
    return fail(SMI_ERR_UNSUPPORTED, "resampling %d Hz -> %d Hz: sample rates above %d Hz are not supported", orig, nw,
                RS_MAX_RATE);
  return SMI_OK;
}

int check_table(int orig, int nw) {
  const Shape s = filter_shape(orig, nw);
  const double bytes = 4.0 * s.n * (std::floor(12.0 * s.o / s.base) + 1);
  if (bytes > (double)RS_MAX_TABLE_BYTES)
    return fail(SMI_ERR_UNSUPPORTED, "resampling %d Hz -> %d Hz: the filter table of %.0f bytes exceeds %lld bytes", orig, nw,
                bytes, (long long)RS_MAX_TABLE_BYTES);
  return SMI_OK;
}

// the cached filter of a validated rate pair (g_rs_mu held)
const Filter& filter_locked(int orig, int nw) {
  const Shape sh = filter_shape(orig, nw);
  Filter& f = filters()[{sh.o, sh.n}];
  if (f.n) return f;
  const int o = sh.o, n = sh.n, width = sh.width, S = sh.S, total = 2 * width + o;
  const double base = sh.base, scale = base / o;
  auto tval = [&](int p, int i) {  // the operation order of the tests' restatement: (-p / n + (i - width) / o) * base
    const double a = (double)(-p) / (double)n;
    const double b = (double)(i - width) / (double)o;
    const double t = a + b;
    return t * base;
  };
  f.taps.assign((size_t)n * S, 0.f);
  f.first.resize(n);
  for (int p = 0; p < n; ++p) {
    // first tap whose window is not the clamped cos(pi/2)^2
    int i = (int)std::floor(width + (double)o * p / n - 6.0 * o / base);
    i = std::max(0, std::min(i, total - 1));
    while (i > 0 && tval(p, i - 1) > -6.0) --i;
    while (i < total - 1 && !(tval(p, i) > -6.0)) ++i;
    i = std::max(0, std::min(i, total - S));
    f.first[p] = i;
    for (int s = 0; s < S; ++s) {
      double t = tval(p, i + s);
      t = std::min(6.0, std::max(-6.0, t));
      const double c = std::cos(t * M_PI / 12.0);
      const double window = c * c;
      const double tp = t * M_PI;
      const double sinc = tp == 0.0 ? 1.0 : std::sin(tp) / tp;
      f.taps[(size_t)p * S + s] = (float)(sinc * (window * scale));
    }
  }
  f.o = o;
  f.width = width;
  f.S = S;
  f.n = n;
  return f;
}

int dev_filter_locked(const Filter& f, const DevFilter** out) {
  DevFilter& d = dev_filters()[{DeviceOnce::dev(), f.o, f.n}];
  if (!d.buf.p) {
    const size_t sp = f.S | 1, words = ((size_t)f.n * (sp + 1) + 3) / 4 * 4;
    std::vector<float> img(words, 0.f);
    for (int p = 0; p < f.n; ++p) std::memcpy(img.data() + p * sp, f.taps.data() + (size_t)p * f.S, (size_t)f.S * 4);
    std::memcpy(img.data() + (size_t)f.n * sp, f.first.data(), (size_t)f.n * 4);
    DevBuf buf;
    HIP_TRY(buf.alloc(words * 4));
    HIP_TRY(hipMemcpy(buf.p, img.data(), words * 4, hipMemcpyHostToDevice));
    d.buf = std::move(buf);
  }
  *out = &d;
  return SMI_OK;
}

int64_t num_samples(int64_t nsamples, int orig, int nw) {
  const int g = std::gcd(orig, nw);
  const int64_t o = orig / g, n = nw / g;
  return (int64_t)(((__int128)nsamples * n + o - 1) / o);
}

// LDS plan of one rate pair: whether the table / the input span of a tile are staged, the tile, and the words it takes
void plan(const Filter& f, int32_t* tile, int32_t* flags, int64_t* lds_words) {
  const int64_t tab_words = (int64_t)f.n * ((f.S | 1) + 1);
  const bool tab_lds = tab_words <= RS_TAB_WORDS;
  const int64_t avail = RS_LDS_WORDS - (tab_lds ? (tab_words + 3) / 4 * 4 : 0);
  // rows m0 .. m0 + (tile + n - 2) / n of taps, plus the slack of the 16-byte alignment at both ends
  auto span = [&](int64_t t) { return (t + f.n - 2) / f.n * f.o + 2 * f.width + f.o + 8; };
  int t = RS_TILE;
  while (t > RS_THREADS && span(t) > avail) t >>= 1;
  const bool span_lds = span(t) <= avail;
  *tile = span_lds ? t : RS_TILE;
  *flags = (tab_lds ? RS_TAB_LDS : 0) | (span_lds ? RS_SPAN_LDS : 0);
  *lds_words = RS_LDS_WORDS - avail + (span_lds ? span(t) : 0);
}

template <bool TAB_LDS, bool SPAN_LDS>
__device__ __forceinline__ void resample_tile(const RsClip& c, const float* __restrict__ waves, float* __restrict__ dst,
                                              float* lds, int64_t j0, int cnt) {
  const int tid = threadIdx.x, n = c.n, o = c.o, S = c.S, SP = S | 1;
  const int tab_words = (n * (SP + 1) + 3) / 4 * 4;
  const float* tab = TAB_LDS ? lds : c.taps;
  const int32_t* fst = TAB_LDS ? (const int32_t*)(lds + n * SP) : c.first;
  float* xs = lds + (TAB_LDS ? tab_words : 0);
  const int64_t m0 = j0 / n;
  const int p0 = (int)(j0 - m0 * n);
  const int64_t g0 = c.in_begin + m0 * o - c.width;  // sample under tap 0 of output row m0 (may lie in front of the clip)
  int shift = 0;
  if (TAB_LDS) {  // the device image is the LDS image
    const f32x4* src = (const f32x4*)c.taps;
    const int nvec = tab_words / 4;
    for (int e0 = tid; e0 < nvec; e0 += RS_STAGE * RS_THREADS) {  // RS_STAGE unconditional loads in flight per thread
      f32x4 v[RS_STAGE];
#pragma unroll
      for (int i = 0; i < RS_STAGE; ++i) v[i] = src[min(e0 + i * RS_THREADS, nvec - 1)];
#pragma unroll
      for (int i = 0; i < RS_STAGE; ++i)
        if (e0 + i * RS_THREADS < nvec) ((f32x4*)lds)[e0 + i * RS_THREADS] = v[i];
    }
  }
  if (SPAN_LDS) {
    const int rows = (p0 + cnt - 1) / n;
    const int len = rows * o + 2 * c.width + o;
    const int64_t al = g0 & ~(int64_t)3;  // the span in 16-byte chunks of `waves`
    shift = (int)(g0 - al);
    const int nchunk = (shift + len + 3) >> 2;
    // chunks [lo, hi) lie wholly inside the clip: one 16-byte load each, RS_STAGE of them in flight per thread
    const bool vec = ((uintptr_t)waves & 15) == 0;
    const int64_t lo64 = (c.in_begin - al + 3) >> 2, hi64 = (c.in_end - al) >> 2;
    const int lo = vec ? (int)(lo64 < 0 ? 0 : lo64 > nchunk ? nchunk : lo64) : 0;
    const int hi = vec ? (int)(hi64 < lo ? lo : hi64 > nchunk ? nchunk : hi64) : 0;
    const int nin = hi - lo;
    const f32x4* src = (const f32x4*)(waves + al) + lo;
    for (int i0 = tid; i0 < nin; i0 += RS_STAGE * RS_THREADS) {
      f32x4 v[RS_STAGE];
#pragma unroll
      for (int i = 0; i < RS_STAGE; ++i) v[i] = src[min(i0 + i * RS_THREADS, nin - 1)];
#pragma unroll
      for (int i = 0; i < RS_STAGE; ++i)
        if (i0 + i * RS_THREADS < nin) ((f32x4*)xs)[lo + i0 + i * RS_THREADS] = v[i];
    }
    // the chunks at the clip's ends and outside it: sample by sample, zero outside the clip
    for (int e = tid; e < nchunk - nin; e += RS_THREADS) {
      const int ch = e < lo ? e : e + nin;
      const int64_t a = al + 4 * (int64_t)ch;
      float4 v;
      v.x = (a >= c.in_begin && a < c.in_end) ? waves[a] : 0.f;
      v.y = (a + 1 >= c.in_begin && a + 1 < c.in_end) ? waves[a + 1] : 0.f;
      v.z = (a + 2 >= c.in_begin && a + 2 < c.in_end) ? waves[a + 2] : 0.f;
      v.w = (a + 3 >= c.in_begin && a + 3 < c.in_end) ? waves[a + 3] : 0.f;
      ((float4*)xs)[ch] = v;
    }
  }
  if (TAB_LDS || SPAN_LDS) __syncthreads();
  if (SPAN_LDS) {
    // outputs u, u + stride, ... of the tile share their phase (stride is a multiple of n): one tap read serves them all
    const int stride = n >= RS_THREADS ? n : n * ((RS_THREADS + n - 1) / n);
    const int xstep = stride / n * o;
    for (int u = tid; u < stride && u < cnt; u += RS_THREADS) {
      const int r = p0 + u, dm = r / n, p = r - dm * n;
      const float* k = tab + (int64_t)p * SP;
      const float* x = xs + shift + dm * o + fst[p];
      const int live = (cnt - u + stride - 1) / stride;  // <= RS_GROUP: stride >= RS_THREADS, cnt <= RS_TILE
      int xo[RS_GROUP];
      float acc[RS_GROUP];
#pragma unroll
      for (int g = 0; g < RS_GROUP; ++g) {
        xo[g] = g < live ? g * xstep : 0;  // an output past the tile re-reads the first one's samples and is not stored
        acc[g] = 0.f;
      }
      for (int s = 0; s < S; ++s) {
        const float kv = k[s];
#pragma unroll
        for (int g = 0; g < RS_GROUP; ++g) acc[g] = fmaf(kv, x[xo[g] + s], acc[g]);
      }
#pragma unroll
      for (int g = 0; g < RS_GROUP; ++g)
        if (g < live) dst[u + g * stride] = acc[g];
    }
  } else {
    for (int q = tid; q < cnt; q += RS_THREADS) {
      const int r = p0 + q, dm = r / n, p = r - dm * n;
      const float* k = tab + (int64_t)p * SP;
      const int64_t gi = g0 + (int64_t)dm * o + fst[p];
      float acc = 0.f;
      for (int s = 0; s < S; ++s) {
        const int64_t idx = gi + s;
        const float xv = (idx >= c.in_begin && idx < c.in_end) ? waves[idx] : 0.f;
        acc = fmaf(k[s], xv, acc);
      }
      dst[q] = acc;
    }
  }
}

__global__ __launch_bounds__(RS_THREADS) void resample_batch_kernel(const float* __restrict__ waves,
                                                                    const RsClip* __restrict__ clips, int nclips,
                                                                    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int64_t b = blockIdx.x;
  int lo = 0, hi = nclips;  // the last clip with tile0 <= b: clips without outputs share the tile0 of the clip behind them
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (clips[mid].tile0 <= b) lo = mid; else hi = mid;
  }
  const RsClip c = clips[lo];
  const int64_t j0 = (b - c.tile0) * c.tile;
  if (j0 >= c.out_len) return;
  const int cnt = (int)(c.out_len - j0 < c.tile ? c.out_len - j0 : c.tile);
  float* dst = out + c.out_begin + j0;
  if (c.flags & RS_COPY) {  // a clip already at the target rate
    const float* src = waves + c.in_begin + j0;
    for (int q = threadIdx.x; q < cnt; q += RS_THREADS) dst[q] = src[q];
    return;
  }
  const bool tl = c.flags & RS_TAB_LDS, sl = c.flags & RS_SPAN_LDS;
  if (tl && sl) resample_tile<true, true>(c, waves, dst, lds, j0, cnt);
  else if (tl) resample_tile<true, false>(c, waves, dst, lds, j0, cnt);
  else if (sl) resample_tile<false, true>(c, waves, dst, lds, j0, cnt);
  else resample_tile<false, false>(c, waves, dst, lds, j0, cnt);
}

}  // namespace

extern "C" {

int64_t smi_resample_num_samples(int64_t nsamples, int32_t orig_rate, int32_t new_rate) {
  if (check_rates(orig_rate, new_rate)) return -1;
  if (nsamples < 0) {
    fail(SMI_ERR_INVALID_ARG, "negative sample count");
    return -1;
  }
  return num_samples(nsamples, orig_rate, new_rate);
}

int smi_resample_filter(int32_t orig_rate, int32_t new_rate, int32_t* phases, int32_t* support, int32_t* width, float* taps,
                        int32_t* first) {
  if (int rc = check_rates(orig_rate, new_rate)) return rc;
  if (int rc = check_table(orig_rate, new_rate)) return rc;
  std::lock_guard<std::mutex> lock(g_rs_mu);
  const Filter& f = filter_locked(orig_rate, new_rate);
  if (phases) *phases = f.n;
  if (support) *support = f.S;
  if (width) *width = f.width;
  if (taps) std::copy(f.taps.begin(), f.taps.end(), taps);
  if (first) std::copy(f.first.begin(), f.first.end(), first);
  return SMI_OK;
}

int smi_resample_batch(const float* waves, const int64_t* in_offsets, const int32_t* rates, int32_t n, int32_t new_rate,
                       float* out, const int64_t* out_offsets, void* stream_v) {
  if (!waves || !in_offsets || !rates || !out || !out_offsets) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (n <= 0) return fail(SMI_ERR_INVALID_ARG, "bad n");
  if (in_offsets[0] < 0 || out_offsets[0] < 0) return fail(SMI_ERR_INVALID_ARG, "offsets must not be negative");
  for (int i = 0; i < n; ++i) {
    if (int rc = check_rates(rates[i], new_rate)) return rc;
    if (rates[i] != new_rate)
      if (int rc = check_table(rates[i], new_rate)) return rc;
    if (in_offsets[i + 1] < in_offsets[i] || out_offsets[i + 1] < out_offsets[i])
      return fail(SMI_ERR_INVALID_ARG, "offsets must be non-decreasing");
    const int64_t want = num_samples(in_offsets[i + 1] - in_offsets[i], rates[i], new_rate);
    if (out_offsets[i + 1] - out_offsets[i] != want)
      return fail(SMI_ERR_INVALID_ARG, "clip %d: out_offsets give %lld samples, %lld samples at %d Hz make %lld at %d Hz", i,
                  (long long)(out_offsets[i + 1] - out_offsets[i]), (long long)(in_offsets[i + 1] - in_offsets[i]), rates[i],
                  (long long)want, new_rate);
  }
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  std::vector<RsClip> clips(n);
  int64_t tiles = 0, lds_words = 0;
  {
    std::lock_guard<std::mutex> lock(g_rs_mu);
    for (int i = 0; i < n; ++i) {
      RsClip& c = clips[i];
      c = RsClip{in_offsets[i], in_offsets[i + 1], out_offsets[i], out_offsets[i + 1] - out_offsets[i], tiles, nullptr, nullptr,
                 1, 1, 0, 0, RS_TILE, RS_COPY};
      if (rates[i] != new_rate) {
        const Filter& f = filter_locked(rates[i], new_rate);
        const DevFilter* d = nullptr;
        if (int rc = dev_filter_locked(f, &d)) return rc;
        c.taps = d->buf.as<float>();
        c.first = d->buf.as<int32_t>() + (size_t)f.n * (f.S | 1);
        c.o = f.o;
        c.n = f.n;
        c.S = f.S;
        c.width = f.width;
        int64_t words = 0;
        plan(f, &c.tile, &c.flags, &words);
        lds_words = std::max(lds_words, words);
      }
      tiles += (c.out_len + c.tile - 1) / c.tile;
    }
  }
  if (tiles == 0) return SMI_OK;
  if (tiles > 0x7fffffffll) return fail(SMI_ERR_UNSUPPORTED, "batch of %lld output tiles exceeds one launch", (long long)tiles);
  hipStream_t stream = (hipStream_t)stream_v;
  RsClip* clips_dev = nullptr;
  HIP_TRY(hipMallocAsync((void**)&clips_dev, (size_t)n * sizeof(RsClip), stream));
  HIP_TRY(hipMemcpyAsync(clips_dev, clips.data(), (size_t)n * sizeof(RsClip), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(resample_batch_kernel, dim3((unsigned)tiles), dim3(RS_THREADS), (size_t)lds_words * 4, stream, waves, clips_dev, n,
                     out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipFreeAsync(clips_dev, stream));
  return SMI_OK;
}

}  // extern "C"
