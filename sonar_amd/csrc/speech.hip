// Device kernels of the SpeechToEmbedding hot path: Kaldi-style log-mel filterbank,
// frame stacking + LayerNorm, the conformer block's depthwise convolution (its
// relative-position attention: relpos_attention.hip), LayerNorm variants, and the attention
// pooler's single-query cross-attention.  GEMMs (FFNs, projections, pointwise convolutions) run on the shared
// MFMA tile engines in gemm.hip.
//
// Reference: sonar/inference_pipelines/speech.py:283-308,431-474 (fbank options, frame
// padding to a multiple of 2), sonar/models/sonar_speech/{factory.py:53-152, model.py:59-77},
// sonar/nn/encoder_pooler.py:70-89; conformer / Wav2Vec2Frontend / RelativePositionSDPA
// semantics of fairseq2 ~=0.4 as listed in SURVEY a26-a29.
#include "common.hpp"
#include "kernels.hpp"
#include "ln_core.hpp"

namespace smi {

// ================================================================== filterbank
// One workgroup per frame: 400 samples -> remove DC -> pre-emphasis 0.97 -> povey window ->
// zero-pad to 512 -> radix-2 FFT in LDS -> power -> 80 triangular mel bins -> log.
constexpr int FB_WIN = 400, FB_SHIFT = 160, FB_NFFT = 512, FB_BINS = 80;

__global__ __launch_bounds__(256) void fbank_kernel(const float* __restrict__ wave, float scale,
                                                    const float* __restrict__ window,
                                                    const float* __restrict__ mel_w,  // [80][256]
                                                    const int* __restrict__ mel_range,  // [80][2]
                                                    float* __restrict__ out) {
  __shared__ float re[FB_NFFT], im[FB_NFFT];
  __shared__ float red[4];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* src = wave + (size_t)f * FB_SHIFT;
  // load (two samples per thread, 400 valid)
  float a0 = tid < FB_WIN ? src[tid] * scale : 0.f;
  float a1 = tid + 256 < FB_WIN ? src[tid + 256] * scale : 0.f;
  float s = wave_sum(a0 + a1);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / FB_WIN;
  if (tid < FB_WIN) re[tid] = a0 - mean;
  if (tid + 256 < FB_WIN) re[tid + 256] = a1 - mean;
  __syncthreads();
  // pre-emphasis + window, bit-reversed scatter for the in-place DIT FFT
  float y0 = 0.f, y1 = 0.f;
  if (tid < FB_WIN) y0 = (re[tid] - 0.97f * re[tid == 0 ? 0 : tid - 1]) * window[tid];
  if (tid + 256 < FB_WIN) y1 = (re[tid + 256] - 0.97f * re[tid + 255]) * window[tid + 256];
  __syncthreads();
  {
    const int r0 = __brev((unsigned)tid) >> 23, r1 = __brev((unsigned)(tid + 256)) >> 23;
    re[r0] = y0;
    im[r0] = 0.f;
    re[r1] = y1;
    im[r1] = 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int st = 1; st <= 9; ++st) {
    const int half = 1 << (st - 1);
    const int grp = tid >> (st - 1), pos = tid & (half - 1);
    const int i0 = grp * (half << 1) + pos, i1 = i0 + half;
    float sn, cs;
    sincospif(-(float)pos / (float)half, &sn, &cs);
    const float xr = re[i1], xi = im[i1];
    const float tr = xr * cs - xi * sn, ti = xr * sn + xi * cs;
    const float ur = re[i0], ui = im[i0];
    re[i0] = ur + tr;
    im[i0] = ui + ti;
    re[i1] = ur - tr;
    im[i1] = ui - ti;
    __syncthreads();
  }
  // power spectrum of bins 0..255 (Kaldi's mel banks do not use the Nyquist bin)
  const float pw = re[tid] * re[tid] + im[tid] * im[tid];
  __syncthreads();
  re[tid] = pw;
  __syncthreads();
  if (tid < FB_BINS) {
    const int k0 = mel_range[tid * 2], k1 = mel_range[tid * 2 + 1];
    float e = 0.f;
    for (int k = k0; k < k1; ++k) e += mel_w[tid * 256 + k] * re[k];
    out[(size_t)f * FB_BINS + tid] = __logf(fmaxf(e, 1.1920929e-07f));
  }
}

// per-utterance standardisation over time (two-pass mean / unbiased std, as the reference's
// converter does).  Three short launches over `nblk` workgroups of 12 x 80 threads (thread (g, b)
// owns frames g, g+12, ... of its workgroup's frame range for mel bin b, loads independent so they
// overlap); column partials go through a stream-ordered scratch [2][nblk][80] (+ [80]: frame 0) and every workgroup
// folds the partials it needs itself (nblk <= 256).
//   pass 0: part0[blk][b] = sum_f (x - x[0])   pass 1: part1[blk][b] = sum_f (x - mean)^2
//   pass 2: x = (x - mean) / std
__global__ __launch_bounds__(960) void fbank_standardize_kernel(float* __restrict__ fb, int frames, int per_blk,
                                                                float* __restrict__ part, int nblk, int pass) {
  __shared__ float red[12][FB_BINS];
  __shared__ float stat[2][FB_BINS];
  const int b = threadIdx.x % FB_BINS, g = threadIdx.x / FB_BINS;
  float* part0 = part;
  float* part1 = part + (size_t)nblk * FB_BINS;
  float* x0_saved = part + (size_t)2 * nblk * FB_BINS;  // frame 0 as pass 0 saw it (pass 2 rewrites the frames in place)
  // fold the partials of the earlier passes
  for (int q = 0; q < pass; ++q) {
    const float* src = q == 0 ? part0 : part1;
    float t = 0.f;
    for (int i = g; i < nblk; i += 12) t += src[(size_t)i * FB_BINS + b];
    red[g][b] = t;
    __syncthreads();
    if (g == 0) {
      float v = 0.f;
      for (int i = 0; i < 12; ++i) v += red[i][b];
      stat[q][b] = q == 0 ? x0_saved[b] + v / frames : 1.0f / sqrtf(v / (frames - 1));
    }
    __syncthreads();
  }
  const int f0 = blockIdx.x * per_blk, f1 = min(frames, f0 + per_blk);
  // pass 0 sums around the column's first value (frame 0): exact mean for a constant column (see the batch kernel)
  const float mean = pass > 0 ? stat[0][b] : fb[b];
  if (pass == 0 && blockIdx.x == 0 && g == 0) x0_saved[b] = fb[b];
  if (pass == 2) {
    const float inv = stat[1][b];
    for (int f = f0 + g; f < f1; f += 12) {
      float* p = fb + (size_t)f * FB_BINS + b;
      *p = (*p - mean) * inv;
    }
    return;
  }
  float acc = 0.f;
  for (int f = f0 + g; f < f1; f += 12) {
    const float d = fb[(size_t)f * FB_BINS + b] - mean;
    acc += pass == 0 ? d : d * d;
  }
  red[g][b] = acc;
  __syncthreads();
  if (g == 0) {
    float v = 0.f;
    for (int i = 0; i < 12; ++i) v += red[i][b];
    (pass == 0 ? part0 : part1)[(size_t)blockIdx.x * FB_BINS + b] = v;
  }
}

// ---- batched filterbank: every clip of a batch in one launch, output zero-padded [n][tpad][80] ----
// grid (tpad, n): workgroup (f, c) computes frame f of clip c (samples off[c] + 160 f ..), or writes the
// zero padding the encoder's collation expects (speech.py:444, pad value 0) when f >= frames(c).
__global__ __launch_bounds__(256) void fbank_batch_kernel(const float* __restrict__ waves,
                                                          const int64_t* __restrict__ off, float scale,
                                                          const float* __restrict__ window,
                                                          const float* __restrict__ mel_w,
                                                          const int* __restrict__ mel_range,
                                                          float* __restrict__ out, int tpad) {
  __shared__ float re[FB_NFFT], im[FB_NFFT];
  __shared__ float red[4];
  const int f = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t ns = off[c + 1] - off[c];
  const int frames = ns < FB_WIN ? 0 : (int)(1 + (ns - FB_WIN) / FB_SHIFT);
  float* dst = out + ((size_t)c * tpad + f) * FB_BINS;
  if (f >= frames) {
    if (tid < FB_BINS) dst[tid] = 0.f;
    return;
  }
  const float* src = waves + off[c] + (size_t)f * FB_SHIFT;
  float a0 = tid < FB_WIN ? src[tid] * scale : 0.f;
  float a1 = tid + 256 < FB_WIN ? src[tid + 256] * scale : 0.f;
  float s = wave_sum(a0 + a1);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / FB_WIN;
  if (tid < FB_WIN) re[tid] = a0 - mean;
  if (tid + 256 < FB_WIN) re[tid + 256] = a1 - mean;
  __syncthreads();
  float y0 = 0.f, y1 = 0.f;
  if (tid < FB_WIN) y0 = (re[tid] - 0.97f * re[tid == 0 ? 0 : tid - 1]) * window[tid];
  if (tid + 256 < FB_WIN) y1 = (re[tid + 256] - 0.97f * re[tid + 255]) * window[tid + 256];
  __syncthreads();
  {
    const int r0 = __brev((unsigned)tid) >> 23, r1 = __brev((unsigned)(tid + 256)) >> 23;
    re[r0] = y0;
    im[r0] = 0.f;
    re[r1] = y1;
    im[r1] = 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int st = 1; st <= 9; ++st) {
    const int half = 1 << (st - 1);
    const int grp = tid >> (st - 1), pos = tid & (half - 1);
    const int i0 = grp * (half << 1) + pos, i1 = i0 + half;
    float sn, cs;
    sincospif(-(float)pos / (float)half, &sn, &cs);
    const float xr = re[i1], xi = im[i1];
    const float tr = xr * cs - xi * sn, ti = xr * sn + xi * cs;
    const float ur = re[i0], ui = im[i0];
    re[i0] = ur + tr;
    im[i0] = ui + ti;
    re[i1] = ur - tr;
    im[i1] = ui - ti;
    __syncthreads();
  }
  const float pw = re[tid] * re[tid] + im[tid] * im[tid];
  __syncthreads();
  re[tid] = pw;
  __syncthreads();
  if (tid < FB_BINS) {
    const int k0 = mel_range[tid * 2], k1 = mel_range[tid * 2 + 1];
    float e = 0.f;
    for (int k = k0; k < k1; ++k) e += mel_w[tid * 256 + k] * re[k];
    dst[tid] = __logf(fmaxf(e, 1.1920929e-07f));
  }
}

// per-clip standardisation of the batch: one workgroup of 12 x 80 threads per clip walks its frames
// three times (mean, unbiased variance around it, normalise) -- the same arithmetic order per column
// group as the single-clip path's partial sums is not needed for parity (both are two-pass fp32).
__global__ __launch_bounds__(960) void fbank_batch_standardize_kernel(float* __restrict__ fb,
                                                                      const int64_t* __restrict__ off, int tpad) {
  __shared__ float red[12][FB_BINS];
  __shared__ float stat[2][FB_BINS];
  const int c = blockIdx.x, b = threadIdx.x % FB_BINS, g = threadIdx.x / FB_BINS;
  const int64_t ns = off[c + 1] - off[c];
  const int frames = ns < FB_WIN ? 0 : (int)(1 + (ns - FB_WIN) / FB_SHIFT);
  if (frames < 2) return;
  float* x = fb + (size_t)c * tpad * FB_BINS + b;
  // The mean is accumulated around the column's first value: a CONSTANT column (digital silence: every frame is log(eps)) then
  // has mean == that value exactly, deviations 0, variance 0 and 0 * inf = NaN features -- what at::std_mean gives the
  // reference's converter and torch.std_mean the oracle (tests/unit_tests/test_sonar_speech.py:29-32 feeds zeros).  A plain
  // sum of 1 098 equal values is off by a few ulp, and the clip came out as finite noise of unit variance instead.
  const float x0 = x[0];
  for (int pass = 0; pass < 2; ++pass) {
    const float mean = pass ? stat[0][b] : x0;
    float acc = 0.f;
    for (int f = g; f < frames; f += 12) {
      const float d = x[(size_t)f * FB_BINS] - mean;
      acc += pass ? d * d : d;
    }
    red[g][b] = acc;
    __syncthreads();
    if (g == 0) {
      float v = 0.f;
      for (int i = 0; i < 12; ++i) v += red[i][b];
      stat[pass][b] = pass ? 1.0f / sqrtf(v / (frames - 1)) : x0 + v / frames;
    }
    __syncthreads();
  }
  const float mean = stat[0][b], inv = stat[1][b];
  for (int f = g; f < frames; f += 12) x[(size_t)f * FB_BINS] = (x[(size_t)f * FB_BINS] - mean) * inv;
}

hipError_t launch_fbank_batch(const float* waves, const int64_t* off_dev, int n, int tpad, float scale,
                              int standardize, const float* window, const float* mel_w, const int* mel_range,
                              float* out, hipStream_t stream) {
  if (n <= 0 || tpad <= 0) return hipSuccess;
  hipLaunchKernelGGL(fbank_batch_kernel, dim3(tpad, n), dim3(256), 0, stream, waves, off_dev, scale, window, mel_w,
                     mel_range, out, tpad);
  if (standardize)
    hipLaunchKernelGGL(fbank_batch_standardize_kernel, dim3(n), dim3(960), 0, stream, out, off_dev, tpad);
  return hipGetLastError();
}

hipError_t launch_fbank(const float* wave, int64_t nsamples, float scale, int standardize, const float* window,
                        const float* mel_w, const int* mel_range, float* out, hipStream_t stream) {
  if (nsamples < FB_WIN) return hipSuccess;
  const int frames = (int)(1 + (nsamples - FB_WIN) / FB_SHIFT);
  hipLaunchKernelGGL(fbank_kernel, dim3(frames), dim3(256), 0, stream, wave, scale, window, mel_w, mel_range, out);
  if (standardize && frames >= 2) {
    int per_blk = 48;
    if ((frames + per_blk - 1) / per_blk > 256) per_blk = ((frames + 255) / 256 + 11) / 12 * 12;
    const int nblk = (frames + per_blk - 1) / per_blk;
    float* part = nullptr;
    hipError_t e = hipMallocAsync((void**)&part, (size_t)(2 * nblk + 1) * FB_BINS * sizeof(float), stream);
    if (e != hipSuccess) return e;
    for (int pass = 0; pass < 3; ++pass)
      hipLaunchKernelGGL(fbank_standardize_kernel, dim3(nblk), dim3(960), 0, stream, out, frames, per_blk, part, nblk,
                         pass);
    e = hipFreeAsync(part, stream);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

// =========================================================== frame stacking + LayerNorm(160)
// out[row(n, j), 0..159] = f16(LN([fb[n, 2j, :], fb[n, 2j+1, :]])), columns 160..191 zero
// (K padded to a multiple of 64 for the projection GEMM).  One wave per stacked frame.
// (A run-time width with masked lanes: ln_center of ln_core.hpp takes neither, so the LayerNorm arithmetic is spelled out here.)
__global__ __launch_bounds__(256) void stack_ln_kernel(const float* __restrict__ fb, int t, int nb,
                                                       const int32_t* __restrict__ cu,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ b, float eps,
                                                       f16* __restrict__ out, int ldo) {
  const int n = blockIdx.x;
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int start = cu[n], len = cu[n + 1] - start;
  if (j >= len) return;
  const int fd = 2 * nb;  // 160
  const float* src = fb + ((size_t)n * t + 2 * j) * nb;  // 2 consecutive frames are contiguous
  float v[3];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < fd ? src[c] : 0.f;
    s += v[k];
  }
  const float mean = wave_sum(s) / fd;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < fd ? v[k] - mean : 0.f;
    q += v[k] * v[k];
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / fd + eps);
  f16* o = out + (size_t)(start + j) * ldo;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = lane + 64 * k;
    if (c < ldo) o[c] = c < fd ? (f16)(v[k] * rstd * w[c] + b[c]) : (f16)0.f;
  }
}

hipError_t launch_stack_ln(const float* fb, int n, int t, int nb, const int32_t* cu, int max_len, const float* w,
                           const float* b, float eps, f16* out, int ldo, hipStream_t stream) {
  if (2 * nb > 192 || ldo > 192) return hipErrorInvalidValue;
  dim3 grid(n, (max_len + 3) / 4);
  hipLaunchKernelGGL(stack_ln_kernel, grid, dim3(256), 0, stream, fb, t, nb, cu, w, b, eps, out, ldo);
  return hipGetLastError();
}

// =============================================================== LayerNorm variants (fp32 stream)
// x = LN1(x) in place (fp32); h = f16(w2 ? LN2(x) : x).  One wave per row.  (The fp32 x written back carries the accuracy
// stated in ln_core.hpp -- the mean's rounding included; an fp16 x is that rounded once.)
template <int NV, bool TM, typename XT>
__global__ __launch_bounds__(256) void ln2_kernel(XT* __restrict__ x, const float* __restrict__ w1,
                                                  const float* __restrict__ b1,
                                                  const float* __restrict__ w2,
                                                  const float* __restrict__ b2, float eps,
                                                  f16* __restrict__ h, int rows, int x_tm) {
  constexpr int D = NV * 256;
  constexpr float inv_d = 1.0f / D;
  const int lane = threadIdx.x & 63;
  if constexpr (sizeof(XT) == 2 && NV % 2 == 0) {
    // fp16 stream: TWO rows per wave (round 6), lanes 0..31 the even row, 32..63 the odd one, a lane owns the 16-B chunks l, l + 32,
    // ... of its row.  In the tile-major layout (common.hpp) a row's share of a 32-column block is 64 B and the next row's follows
    // it: with one row per wave every access was a 64-B piece of a 128-B line (the stream read, its write-back and the tile-major
    // h); a row pair covers whole lines.  x_tm: the stream itself is tile-major; TM: h is.  8 rows per workgroup.
    const int half = lane >> 5, l = lane & 31;
    const int rr = blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half;
    const bool live = rr < rows;
    const int r2 = live ? rr : rows - 1;
    XT* xr2 = x + (size_t)r2 * D;
    auto xp = [&](int k) { return x_tm ? x + tm_offset(r2, (l + 32 * k) * 8, D) : xr2 + (l + 32 * k) * 8; };
    half8 raw[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) raw[k] = *(const half8*)xp(k);
    float u[NV][8];
    float s8 = ln_widen8(raw, u);
    float rstd8 = ln_center<8>(u, s8, inv_d, eps, half_sum);  // half_sum: the 32 lanes of the row
    s8 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const float* wp = w1 + (l + 32 * k) * 8;
      const float* bp = b1 + (l + 32 * k) * 8;
      const f32x4 wa = *(const f32x4*)wp, wb = *(const f32x4*)(wp + 4), ba = *(const f32x4*)bp, bb = *(const f32x4*)(bp + 4);
      half8 hv;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float y = u[k][i] * rstd8 * (i < 4 ? wa[i] : wb[i - 4]) + (i < 4 ? ba[i] : bb[i - 4]);
        hv[i] = (f16)y;
        u[k][i] = (float)hv[i];  // the second LayerNorm sees what the stream holds
        s8 += u[k][i];
      }
      if (live) *(half8*)xp(k) = hv;
    }
    if (!h) return;
    if (w2) {
      rstd8 = ln_center<8>(u, s8, inv_d, eps, half_sum);
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const float* wp = w2 + (l + 32 * k) * 8;
        const float* bp = b2 + (l + 32 * k) * 8;
        const f32x4 wa = *(const f32x4*)wp, wb = *(const f32x4*)(wp + 4), ba = *(const f32x4*)bp, bb = *(const f32x4*)(bp + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) u[k][i] = u[k][i] * rstd8 * (i < 4 ? wa[i] : wb[i - 4]) + (i < 4 ? ba[i] : bb[i - 4]);
      }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      half8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = (f16)u[k][i];
      if constexpr (TM)
        *(half8*)(h + tm_offset(rr, (l + 32 * k) * 8, D)) = o;  // one 16-B chunk of the tile-major operand
      else
        *(half8*)(h + (size_t)rr * D + (l + 32 * k) * 8) = o;
    }
    return;
  }
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  XT* xr = x + (size_t)r * D;
  f32x4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if constexpr (sizeof(XT) == 4) {
      v[k] = *(const f32x4*)(xr + k * 256 + lane * 4);
    } else {
      const half4 hv = *(const half4*)(xr + k * 256 + lane * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[k][i] = (float)hv[i];
    }
    s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  }
  float rstd = ln_center<4>(v, s, inv_d, eps, wave_sum);
  s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const f32x4 wv = *(const f32x4*)(w1 + k * 256 + lane * 4);
    const f32x4 bv = *(const f32x4*)(b1 + k * 256 + lane * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[k][i] = v[k][i] * rstd * wv[i] + bv[i];
    if constexpr (sizeof(XT) == 4) {
      *(f32x4*)(xr + k * 256 + lane * 4) = v[k];
    } else {
      half4 hv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        hv[i] = (f16)v[k][i];
        v[k][i] = (float)hv[i];  // the second LayerNorm sees what the stream holds
      }
      *(half4*)(xr + k * 256 + lane * 4) = hv;
    }
    s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  }
  if (!h) return;
  if (w2) {
    rstd = ln_center<4>(v, s, inv_d, eps, wave_sum);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const f32x4 wv = *(const f32x4*)(w2 + k * 256 + lane * 4);
      const f32x4 bv = *(const f32x4*)(b2 + k * 256 + lane * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[k][i] = v[k][i] * rstd * wv[i] + bv[i];
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    half4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (f16)v[k][i];
    if constexpr (TM)
      *(half4*)(h + tm_offset(r, k * 256 + lane * 4, D)) = o;  // tile-major GEMM operand (common.hpp)
    else
      *(half4*)(h + (size_t)r * D + k * 256 + lane * 4) = o;
  }
}

hipError_t launch_ln2(void* x, const float* w1, const float* b1, const float* w2, const float* b2, float eps,
                      f16* h, int rows, int d, hipStream_t stream, int out_tm, int x_f16, int x_tm) {
  if (rows <= 0) return hipErrorInvalidValue;
  if (x_tm && (!x_f16 || d % 512)) return hipErrorInvalidValue;  // the tile-major stream is fp16, 16-B chunks per lane
  // 4 rows per workgroup (one wave per row); the fp16 stream with an even NV: 8 (a row pair per wave)
  const bool known = dispatch_nv(d, [&](auto nv) {
    dispatch_f16(x_f16, [&](auto xt) {
      constexpr int NV = decltype(nv)::value;
      using XT = decltype(xt);
      const dim3 grid(sizeof(XT) == 2 && NV % 2 == 0 ? (rows + 7) / 8 : (rows + 3) / 4);
      if (out_tm)
        hipLaunchKernelGGL((ln2_kernel<NV, true, XT>), grid, dim3(256), 0, stream, (XT*)x, w1, b1, w2, b2, eps, h, rows, x_tm);
      else
        hipLaunchKernelGGL((ln2_kernel<NV, false, XT>), grid, dim3(256), 0, stream, (XT*)x, w1, b1, w2, b2, eps, h, rows, x_tm);
    });
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

// ============================================= depthwise conv (k taps, 'same') + BatchNorm + SiLU
// y[t][c] = silu(scale[c] * sum_k w[c][k] x[t + k - (K-1)/2][c] + shift[c]), zero outside the clip.
// Workgroup = 32 output frames x 256 channels of one clip.  The 32 + (K-1) input rows are staged in LDS
// with 16-B loads (a 512-B row per 32 lanes) and the outputs leave through LDS with 16-B stores; in
// between thread = channel reads its column (2 B per lane, conflict-free) once into registers, so every
// tap index is a compile-time constant.  (The first version loaded and stored 2 B per lane straight
// from / to global memory: 126 us per call for 131 MB.)
template <int KT>
__global__ __launch_bounds__(256) void dwconv_bn_silu_kernel(const f16* __restrict__ x,
                                                             const int32_t* __restrict__ cu,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             f16* __restrict__ y, int d, int y_tm, int x_tm) {
  constexpr int TT = 32, HALF = (KT - 1) / 2, NIN = TT + KT - 1;
  __shared__ __attribute__((aligned(16))) f16 xin[NIN][256];
  __shared__ __attribute__((aligned(16))) f16 yout[TT][256];
  const int n = blockIdx.x, t0 = blockIdx.y * TT, c0 = blockIdx.z * 256, tid = threadIdx.x;
  const int start = cu[n], len = cu[n + 1] - start;
  if (t0 >= len) return;
  for (int i = tid; i < NIN * 32; i += 256) {
    const int r = i >> 5, ch = (i & 31) * 8;
    const int t = t0 - HALF + r;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};  // zero outside the clip
    if (t >= 0 && t < len)  // x_tm: the GLU output arrives tile-major (a 16-B chunk of a row is a 16-B chunk there too)
      v = *(const half8*)(x_tm ? x + tm_offset(start + t, c0 + ch, d) : x + (size_t)(start + t) * d + c0 + ch);
    *(half8*)&xin[r][ch] = v;
  }
  const int c = c0 + tid;
  // Two taps per instruction (round 6: the kernel is VALU-bound -- 32 x 31 fp32 FMAs per thread were ~80 % of its time): the
  // window is held as fp16 PAIRS of consecutive frames, once starting at even and once at odd offsets (62 registers, as many as
  // the fp32 window took), the taps as fp16 pairs (the fp16 model's conv weights ARE fp16; an fp32 model's are rounded like every
  // GEMM weight of the engine), and v_dot2_f32_f16 forms a0 b0 + a1 b1 + c with exact products and fp32 accumulation.
  constexpr int NP = (KT + 1) / 2;
  half2v wk2[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float w0 = w[(size_t)c * KT + 2 * j], w1 = 2 * j + 1 < KT ? w[(size_t)c * KT + 2 * j + 1] : 0.f;
    wk2[j] = half2v{(f16)w0, (f16)w1};
  }
  const float sc = scale[c], sh = shift[c];
  __syncthreads();
  constexpr int NW = NIN + 1;  // one padding frame so that the last odd pair exists (its tap is the zero pad of an odd KT)
  half2v pe[NW / 2], po[NW / 2];  // pe[i] = (x[2i], x[2i+1]), po[i] = (x[2i+1], x[2i+2])
  {
    f16 prev = xin[0][tid];
#pragma unroll
    for (int i = 0; i < NW / 2; ++i) {
      const f16 a = xin[2 * i + 1][tid];
      const f16 b = 2 * i + 2 < NIN ? xin[2 * i + 2][tid] : (f16)0.f;
      pe[i] = half2v{prev, a};
      po[i] = half2v{a, b};
      prev = b;
    }
  }
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j)  // frames tt + 2j, tt + 2j + 1
      acc = __builtin_amdgcn_fdot2((tt & 1) ? po[(tt + 2 * j) / 2] : pe[(tt + 2 * j) / 2], wk2[j], acc, false);
    const float v = acc * sc + sh;
    yout[tt][tid] = (f16)(v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v)));  // SiLU
  }
  __syncthreads();
  for (int i = tid; i < TT * 32; i += 256) {
    const int tt = i >> 5, ch = (i & 31) * 8;
    if (t0 + tt < len) {  // y_tm: tile-major X operand of pointwise_conv2 (a 16-B chunk of a row is a 16-B chunk there too)
      f16* dst = y_tm ? y + tm_offset(start + t0 + tt, c0 + ch, d) : y + (size_t)(start + t0 + tt) * d + c0 + ch;
      *(half8*)dst = *(const half8*)&yout[tt][ch];
    }
  }
}

hipError_t launch_dwconv_bn_silu(const f16* x, const int32_t* cu, const float* w, const float* scale,
                                 const float* shift, f16* y, int n, int max_len, int d, int ktaps,
                                 hipStream_t stream, int y_tm, int x_tm) {
  if (d % 256 || n <= 0 || max_len <= 0) return hipErrorInvalidValue;
  dim3 grid(n, (max_len + 31) / 32, d / 256);
  switch (ktaps) {
    case 31:
      hipLaunchKernelGGL(dwconv_bn_silu_kernel<31>, grid, dim3(256), 0, stream, x, cu, w, scale, shift, y, d, y_tm, x_tm);
      break;
    case 7:
      hipLaunchKernelGGL(dwconv_bn_silu_kernel<7>, grid, dim3(256), 0, stream, x, cu, w, scale, shift, y, d, y_tm, x_tm);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ================================================== pooler: one query per clip over its frames
// q: [n][d] (row per clip), kv: [R][2d] (k | v) packed frames; one wave per (clip, head).
__global__ __launch_bounds__(256) void pool_attention_kernel(const f16* __restrict__ q,
                                                             const f16* __restrict__ kv,
                                                             const int32_t* __restrict__ cu,
                                                             f16* __restrict__ ctx, int n, int d, int heads,
                                                             float sl2e) {
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= n * heads) return;
  const int c = wid / heads, h = wid % heads;
  const int lane = threadIdx.x & 63;
  const int start = cu[c], len = cu[c + 1] - start;
  const f16* qp = q + (size_t)c * d + h * 64;
  half8 qf[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) qf[i] = *(const half8*)(qp + i * 8);
  const size_t ld = (size_t)2 * d;
  const f16* kb = kv + (size_t)start * ld + h * 64;
  // P.V: lane (pg, c8) accumulates head dims c8*8..+7 over the positions j0 + 8 it + pg (16-B row pieces,
  // the probability comes from the lane that scored that position), joined across pg at the end
  const int pg = lane >> 3, c8 = lane & 7;
  float m = -1e30f, l = 0.f;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  for (int j0 = 0; j0 < len; j0 += 64) {
    const int j = j0 + lane;
    float s = -INFINITY;
    if (j < len) {
      const f16* kp = kb + (size_t)j * ld;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const half8 kk = *(const half8*)(kp + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (float)qf[i][e] * (float)kk[e];
      }
      s = acc * sl2e;
    }
    const float m_new = fmaxf(m, wave_max(s));
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    const float p = __builtin_amdgcn_exp2f(s - m_new);
    l = l * alpha + wave_sum(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] *= alpha;
    m = m_new;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int t = it * 8 + pg;
      const float pt = __shfl(p, t, 64);  // 0 for positions past the clip
      if (j0 + t < len) {
        const half8 vv = *(const half8*)(kb + (size_t)(j0 + t) * ld + d + c8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += pt * (float)vv[e];
      }
    }
  }
  half8 out;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float v = o[e];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    out[e] = (f16)(len > 0 ? v / l : 0.f);
  }
  if (pg == 0) *(half8*)(ctx + (size_t)c * d + h * 64 + c8 * 8) = out;
}

hipError_t launch_pool_attention(const f16* q, const f16* kv, const int32_t* cu, f16* ctx, int n, int d, int heads,
                                 hipStream_t stream) {
  if (heads <= 0 || d != heads * 64 || n <= 0) return hipErrorInvalidValue;
  const float sl2e = 0.125f * 1.4426950408889634f;
  hipLaunchKernelGGL(pool_attention_kernel, dim3((n * heads + 3) / 4), dim3(256), 0, stream, q, kv, cu, ctx, n, d,
                     heads, sl2e);
  return hipGetLastError();
}

// x[r, :] = row[:] for r < rows (pooler query initialisation)
__global__ void broadcast_row_kernel(const float* __restrict__ row, float* __restrict__ x, int rows, int d) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)rows * d) x[i] = row[i % d];
}

hipError_t launch_broadcast_row(const float* row, float* x, int rows, int d, hipStream_t stream) {
  const size_t total = (size_t)rows * d;
  hipLaunchKernelGGL(broadcast_row_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, row, x, rows, d);
  return hipGetLastError();
}

}  // namespace smi
