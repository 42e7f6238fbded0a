// C-ABI implementation of the text decoder / beam search (see include/sonar_mi355.h).
// Host runtime: weight packing, workspace, and the per-step launch schedule
// (reference op order: sonar/models/sonar_text/factory.py:261-307, pre-LN decoder layers,
// final LayerNorm, tied projection; generation control: fairseq2 BeamSearchSeq2SeqGenerator).
#include <cmath>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "api_common.hpp"

using namespace smi;
using namespace smi_host;

namespace {

struct DecLayer {
  DevBuf ln1_w, ln1_b, w_qkv, b_qkv, w_o, b_o;
  DevBuf wc_v, bc_v, wc_o, bc_o;  // encoder_decoder_attn value / output projections
  DevBuf ln3_w, ln3_b, w_1, b_1, w_2, b_2;
};

constexpr int kMaxParts = 16;  // split-K slabs the `parts` buffer holds

// step processors on the device: the banned sequences as a CSR in buffers of its own, and what the kernels get of it
struct StepProcTable {
  DevBuf tok, off;
  StepProcDev dev{};
};

}  // namespace

// Per-call workspace of ONE decode chain (grow-only).  smi_text_decoder_generate may split a batch into several
// chains of whole sentences: they share nothing but the weights, so each owns its activations, KV cache, beam state
// and stream, and their launch sequences overlap on the GPU.
// A/B switches of the decode step, read from the tuning registry (tuning.hpp, smi_tuning_set; never from the environment)
// when a generate / sample / logits call starts: TUNE_DEC_KS_OUT, TUNE_DEC_KS_FFN (split-K parts of the attention-output /
// FFN-output projections; 0 = automatic, KS_OUT 1 = no split), TUNE_DEC_FFN1_ENGINE (-1 automatic, 0 the GEMM's own choice,
// 1 = 128x128, 2 = 256x256), TUNE_DEC_LOGITS_GRID (persistent workgroups of a chained call's logits GEMM; 0 = all CUs)
struct DecTuning {
  int ks_out = 0, ks_ffn = 0, ffn1_engine = -1, logits_grid = 0;
  void read() {
    ks_out = tune(TUNE_DEC_KS_OUT, 0);
    ks_ffn = tune(TUNE_DEC_KS_FFN, 0);
    ffn1_engine = tune(TUNE_DEC_FFN1_ENGINE, -1);
    logits_grid = tune(TUNE_DEC_LOGITS_GRID, 0);
  }
};

struct DecWork {
  DecTuning tuning;
  DevBuf x, h, ctx, ffn, logits, kv, cc, cvtmp, emb16, parts;
  DevBuf tok, cum, parent, new_tok, new_cum, nactive, done, ndone, fin_count, fin_len, fin_score, fin_tok;
  DevBuf anc[2], hist[2];
  DevBuf pmax, psum, pval, pidx;
  DevBuf tile_max, tile_sum;  // logits-GEMM tile statistics [rows_pad][vocab_pad / 256]
  // the call's prompt(s), int32.  One prompt: [prompt_len], read by sampling under step processors.  Per-sentence prompts
  // (smi_text_decoder_*_prompts): ws[0] holds the whole call's table, tokens [n][stride] then lengths [n]; a chain reads its
  // sentence group's slice of it
  DevBuf prompt_dev;
  DevBuf sc_lens, sc_tgt, sc_bad, sc_cu;  // teacher-forced scoring: lengths, row targets, bad-id flag, [0, seq, 2 seq, ...]
  int kv_positions = 0;       // positions per layer in the current kv allocation
  bool chained = false;       // this call runs next to other chains: per-launch tile choices differ (decoder_step)
  hipStream_t stream = nullptr;  // chains of a split call run on streams of their own
  hipEvent_t done_ev = nullptr;
  hipEvent_t sp_ev = nullptr;    // end of this workspace's last call that read the step-processor table
};

constexpr int kMaxChains = 4;

struct smi_text_decoder {
  smi_text_decoder_config cfg;
  int64_t vocab_pad = 0;
  DevBuf embed, pos, lnf_w, lnf_b;
  DevBuf embed_tm;  // tile-major copy of the (padded) table for the tied output projection
  std::vector<DecLayer> layers;
  DecWork ws[kMaxChains];  // ws[0]: the single-chain calls (logits, sample, unsplit generate)
  hipEvent_t fork_ev = nullptr;
  DevBuf margins;       // [n][2] decision margins of the last generate() call
  int margins_n = 0;
  int chains = 0;       // smi_text_decoder_set_chains: 0 = TUNE_DEC_CHAINS / the default
  int beam_logits_f16 = 0;  // smi_text_decoder_set_beam_logits_dtype: the beam search's logits are stored in fp16
  int beam_slab_f16 = 0;    // smi_text_decoder_set_slab_dtype: the beam search's split-K partial sums are stored in fp16
  StepProcTable sp;  // smi_text_decoder_set_step_processors (dev.ngram 0 = off); read by every chain
  int64_t weight_bytes = 0;
  int ffn_tile_major = 0;  // FFN weights stored tile-major (d, f multiples of 256)
  // Generic-dimension mode (flex.hip): head_dim != 64 or dimensions the MFMA engines do not tile for (the reference's
  // `toy` arch, config.py:232-255).  fp32 weights, activations and KV cache; the beam search / sampling kernels are
  // shared with the fast mode (they only see logits rows and tile statistics).
  bool flex = false;
  size_t act_bytes() const { return flex ? 4 : 2; }  // element size of h / ctx / ffn / the KV cache
  ~smi_text_decoder() {
    for (auto& w : ws) {
      if (w.stream) (void)hipStreamDestroy(w.stream);
      if (w.done_ev) (void)hipEventDestroy(w.done_ev);
      if (w.sp_ev) (void)hipEventDestroy(w.sp_ev);
    }
    if (fork_ev) (void)hipEventDestroy(fork_ev);
  }
};

namespace {

// The ids the selection masks (PAD, blocked EOS, penalised UNK) must live in tile 0, ids 0..255: the tile argument of
// vocab_select_kernel ranks the later tiles by their RAW maximum, and a masked id that is a later tile's maximum would take a
// slot from a tile that holds a real candidate (decoder.hip).  -1 = none; the EOS of a search always exists.
int check_special_ids(int pad_idx, int eos_idx, int unk_idx, int64_t vocab, bool need_eos) {
  const int64_t lim = vocab < 256 ? vocab : 256;
  if (pad_idx < -1 || eos_idx < (need_eos ? 0 : -1) || unk_idx < -1)
    return fail(SMI_ERR_INVALID_ARG, "bad special ids: pad_idx=%d eos_idx=%d unk_idx=%d", pad_idx, eos_idx, unk_idx);
  if (pad_idx >= lim || eos_idx >= lim || unk_idx >= lim)
    return fail(SMI_ERR_UNSUPPORTED, "special ids must be below 256 and the vocabulary: pad_idx=%d eos_idx=%d unk_idx=%d", pad_idx,
                eos_idx, unk_idx);
  return SMI_OK;
}

// SMI_OK and *flex = false: the MFMA engines cover the shape; *flex = true: the generic-dimension kernels do
int check_dec_cfg(const smi_text_decoder_config& c, bool* flex) {
  if (c.model_dim <= 0 || c.num_heads <= 0 || c.model_dim % c.num_heads)
    return fail(SMI_ERR_INVALID_ARG, "model_dim %d must be a positive multiple of num_heads %d", c.model_dim, c.num_heads);
  if (c.ffn_inner_dim <= 0 || c.input_dim <= 0)
    return fail(SMI_ERR_INVALID_ARG, "bad ffn_inner_dim %d / input_dim %d", c.ffn_inner_dim, c.input_dim);
  if (c.num_layers < 0 || c.vocab_size <= 16 || c.max_seq_len <= 1 || c.pos_offset < 0)
    return fail(SMI_ERR_INVALID_ARG, "bad num_layers/vocab_size/max_seq_len/pos_offset");
  const bool fast = c.model_dim == c.num_heads * 64 && c.model_dim % 256 == 0 &&
                    (c.model_dim / 256 <= 4 || c.model_dim == 2048) && c.ffn_inner_dim % 128 == 0 && c.input_dim % 64 == 0;
  if (!fast && c.model_dim / c.num_heads > 256)
    return fail(SMI_ERR_UNSUPPORTED, "head_dim %d > 256 is not covered", c.model_dim / c.num_heads);
  if (int rc = check_special_ids(c.pad_idx, c.eos_idx, c.unk_idx, c.vocab_size, true)) return rc;
  *flex = !fast;
  return SMI_OK;
}

// the sentence vectors of every entry point: fp32 or fp16 rows of input_dim elements
int check_emb_dtype(int emb_dtype) {
  return emb_dtype == SMI_F32 || emb_dtype == SMI_F16 ? SMI_OK : fail(SMI_ERR_INVALID_ARG, "bad emb dtype");
}
size_t emb_row_bytes(const smi_text_decoder_config& c, int emb_dtype) { return (size_t)c.input_dim * (emb_dtype == SMI_F32 ? 4 : 2); }

// per-sentence cross-attention constants cc[l][s] = W_o (W_v e_s + b_v) + b_o  (fp32 [L][n_pad][d])
int compute_cross_constants(smi_text_decoder* D, DecWork& S, const void* emb, int emb_dtype, int n, int n_pad,
                            hipStream_t stream) {
  const int d = D->cfg.model_dim, ci = D->cfg.input_dim;  // the conditioning vector may be wider / narrower than the model
  HIP_TRY(S.cc.reserve((size_t)D->cfg.num_layers * n_pad * d * 4));
  if (D->flex) {
    HIP_TRY(S.emb16.reserve((size_t)n * ci * 4));  // fp32 copy of the sentence vectors
    HIP_TRY(S.cvtmp.reserve((size_t)n * d * 4));
    if (emb_dtype == SMI_F32)
      HIP_TRY(hipMemcpyAsync(S.emb16.p, emb, (size_t)n * ci * 4, hipMemcpyDeviceToDevice, stream));
    else
      HIP_TRY(launch_f16_to_f32((const f16*)emb, S.emb16.as<float>(), (size_t)n * ci, stream));
    for (int l = 0; l < D->cfg.num_layers; ++l) {
      DecLayer& L = D->layers[l];
      HIP_TRY(launch_flex_linear(S.emb16.as<float>(), ci, L.wc_v.as<float>(), L.bc_v.as<float>(), S.cvtmp.as<float>(), d,
                                 n, d, ci, 0, nullptr, 0, stream));
      HIP_TRY(launch_flex_linear(S.cvtmp.as<float>(), d, L.wc_o.as<float>(), L.bc_o.as<float>(),
                                 S.cc.as<float>() + (size_t)l * n_pad * d, d, n, d, d, 0, nullptr, 0, stream));
    }
    return SMI_OK;
  }
  HIP_TRY(S.emb16.reserve((size_t)n_pad * ci * 2));
  HIP_TRY(S.cvtmp.reserve((size_t)n_pad * d * 2));
  HIP_TRY(hipMemsetAsync(S.emb16.p, 0, (size_t)n_pad * ci * 2, stream));
  if (emb_dtype == SMI_F32)
    HIP_TRY(launch_f32_to_f16((const float*)emb, S.emb16.as<f16>(), (size_t)n * ci, stream));
  else
    HIP_TRY(hipMemcpyAsync(S.emb16.p, emb, (size_t)n * ci * 2, hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipMemsetAsync(S.cc.p, 0, (size_t)D->cfg.num_layers * n_pad * d * 4, stream));
  for (int l = 0; l < D->cfg.num_layers; ++l) {
    DecLayer& L = D->layers[l];
    HIP_TRY(launch_gemm_tn(EPI_BIAS_F16, S.emb16.as<f16>(), L.wc_v.as<f16>(), L.bc_v.as<float>(),
                           S.cvtmp.p, n_pad, d, ci, d, stream));
    HIP_TRY(launch_gemm_tn(EPI_RESID_F32, S.cvtmp.as<f16>(), L.wc_o.as<f16>(), L.bc_o.as<float>(),
                           S.cc.as<float>() + (size_t)l * n_pad * d, n_pad, d, d, d, stream));
  }
  return SMI_OK;
}

// The same step on the generic-dimension kernels (flex.hip): fp32 throughout, one launch per reference module.
int flex_decoder_step(smi_text_decoder* D, DecWork& S, int rows, int rows_pad, int group, int n_pad, int pos,
                      const int32_t* anc, int anc_stride, hipStream_t stream, float stats_scale) {
  const smi_text_decoder_config& c = D->cfg;
  const int d = c.model_dim, f = c.ffn_inner_dim;
  float* x = S.x.as<float>();
  float* h = S.h.as<float>();
  float* ctx = S.ctx.as<float>();
  float* ffn = S.ffn.as<float>();
  const size_t slab = (size_t)rows_pad * 3 * d;
  const int P = S.kv_positions;
  HIP_TRY(launch_flex_embed(nullptr, S.tok.as<int32_t>(), D->embed.as<float>(), D->pos.as<float>(), c.embed_scale, x, rows, d,
                            1, c.pos_offset, pos, c.vocab_size, nullptr, stream));
  for (int l = 0; l < c.num_layers; ++l) {
    DecLayer& L = D->layers[l];
    float* kvl = S.kv.as<float>() + (size_t)l * P * slab;
    HIP_TRY(launch_flex_layernorm(x, L.ln1_w.as<float>(), L.ln1_b.as<float>(), c.ln_eps, h, rows, d, stream));
    HIP_TRY(launch_flex_linear(h, d, L.w_qkv.as<float>(), L.b_qkv.as<float>(), kvl + (size_t)pos * slab, 3 * d, rows, 3 * d,
                               d, 0, nullptr, 0, stream));
    HIP_TRY(launch_flex_dec_attention(kvl, anc, anc_stride, ctx, rows, rows_pad, d, c.num_heads, pos, stream));
    HIP_TRY(launch_flex_linear(ctx, d, L.w_o.as<float>(), L.b_o.as<float>(), x, d, rows, d, d, 0, x, d, stream));
    HIP_TRY(launch_flex_add_rows(x, S.cc.as<float>() + (size_t)l * n_pad * d, rows, d, group, stream));
    HIP_TRY(launch_flex_layernorm(x, L.ln3_w.as<float>(), L.ln3_b.as<float>(), c.ln_eps, h, rows, d, stream));
    HIP_TRY(launch_flex_linear(h, d, L.w_1.as<float>(), L.b_1.as<float>(), ffn, f, rows, f, d, 1, nullptr, 0, stream));
    HIP_TRY(launch_flex_linear(ffn, f, L.w_2.as<float>(), L.b_2.as<float>(), x, d, rows, d, f, 0, x, d, stream));
  }
  HIP_TRY(launch_flex_layernorm(x, D->lnf_w.as<float>(), D->lnf_b.as<float>(), c.ln_eps, h, rows, d, stream));
  HIP_TRY(launch_flex_linear(h, d, D->embed.as<float>(), nullptr, S.logits.as<float>(), (int)D->vocab_pad, rows,
                             (int)c.vocab_size, d, 0, nullptr, 0, stream));
  if (stats_scale > 0.f)
    HIP_TRY(launch_flex_tile_stats(S.logits.as<float>(), (int)D->vocab_pad, rows, (int)c.vocab_size, stats_scale,
                                   S.tile_max.as<float>(), S.tile_sum.as<float>(), rows_pad, stream));
  return SMI_OK;
}

// one decoder step at position `pos` for `rows` rows (rows_pad GEMM rows); logits -> S.logits
// logits_f16 (beam search of an fp16 model, round 4): the logits GEMM stores fp16 in the tile-major layout (the reference's
// fp16 model produces fp16 logits too: fairseq2 up-casts them inside log_softmax) and takes the tile statistics of the
// rounded values; needs the tile-major table copy.  Halves the 1.3 GB the 256 x 5-row step wrote per position.
int decoder_step(smi_text_decoder* D, DecWork& S, int rows, int rows_pad, int group, int n_pad, int pos,
                 const int32_t* anc, int anc_stride, hipStream_t stream, float stats_scale = 0.f, int logits_f16 = 0,
                 int slab_f16 = 0) {
  if (D->flex) return flex_decoder_step(D, S, rows, rows_pad, group, n_pad, pos, anc, anc_stride, stream, stats_scale);
  const smi_text_decoder_config& c = D->cfg;
  const int d = c.model_dim, f = c.ffn_inner_dim;
  float* x = S.x.as<float>();
  f16* h = S.h.as<f16>();
  f16* ctx = S.ctx.as<f16>();
  f16* ffn = S.ffn.as<f16>();
  const size_t slab = (size_t)rows_pad * 3 * d;  // elements per (layer, pos)
  const int P = S.kv_positions;
  void* parts = S.parts.p;
  const size_t part_stride = (size_t)rows_pad * d;  // elements
  // fp16 split-K slabs in the fp16 model's beam search (smi_text_decoder_set_slab_dtype; its own setting since round 5: the
  // reference rounds every sublayer output to fp16; here each partial is rounded once -- saturating at +-65504, never inf --,
  // the sum is formed in fp32 and added to the fp32 stream): half the 42 MB the FFN output projection wrote and the next
  // kernel read per layer at 1280 rows.  Tuning switch DEC_SLAB_F16 = 0 / 1 overrides (A/B runs).
  const int sf16 = slab_f16;
  // Split-K parts of the two N = d projections.  FFN output (K = f): 8 parts of 32 K slices = 160 lone units at
  // 1280 rows; 10 / 12 parts (unequal K ranges, 200 / 240 units) were traced and are NOT faster -- a unit's K loop
  // shrinks 20.0 -> 15.3 us but its 256 KiB slab store grows 4.3 -> 6.4 us (the slab writes run at the chip's
  // ~9.8 TB/s write path either way) and the fold reads 4 more slabs (profiles/r03_experiments.txt).
  // Attention output (K = d): as many parts as keep every 128x128 unit on a CU of its own (2 at 1280 rows: 160 units
  // on the lone-tile ring engine); TUNE_DEC_KS_OUT overrides for A/B runs, 1 = no split, residual epilogue.
  const DecTuning& tu = S.tuning;
  // (an override the slab buffer or the K split cannot take falls back to the automatic choice)
  const bool ks_out_ok = tu.ks_out >= 1 && tu.ks_out <= kMaxParts && d % (64 * tu.ks_out) == 0;
  const int ks_out = ks_out_ok ? tu.ks_out : gemm_splitk_parts(rows_pad, d, d, kMaxParts, gemm_env());
  const int ks_ffn = tu.ks_ffn > 0 && tu.ks_ffn <= kMaxParts && f % (256 * tu.ks_ffn) == 0
                         ? tu.ks_ffn : (f % 512 == 0 ? 8 : (f % 256 == 0 ? 4 : 1));
  // A chain of a split call (S.chained) has too few FFN-inner tiles for the automatic engine choice (3 x 32 at 768
  // rows < the 144-tile crossover measured for ONE chain on an idle chip), but its neighbours fill the other CUs:
  // keep it on the 256x256 engine.  Its logits GEMM -- the one launch of a step that wants the whole chip -- may
  // leave CUs to the other chains (tu.logits_grid).
  const int ffn1_engine = tu.ffn1_engine >= 0 ? tu.ffn1_engine
                                              : (S.chained && rows_pad % 256 == 0 && f % 256 == 0 ? 2 : 0);
  const int logits_grid_env = tu.logits_grid;
  HIP_TRY(launch_dec_embed(S.tok.as<int32_t>(), D->embed.as<f16>(),
                           D->pos.as<float>() + (size_t)(pos + c.pos_offset) * d, c.embed_scale, x, rows, d,
                           c.vocab_size, stream));
  for (int l = 0; l < c.num_layers; ++l) {
    DecLayer& L = D->layers[l];
    f16* kvl = S.kv.as<f16>() + (size_t)l * P * slab;
    // x += FFN-out slabs of the previous layer (split-K), then LN1
    // (small batches: the CUs the row kernels leave idle read the layer's FFN matrices ahead, common.hpp: prefetch_range)
    HIP_TRY(launch_sum_layernorm(x, l ? parts : nullptr, ks_ffn, part_stride, nullptr, 1, L.ln1_w.as<float>(),
                                 L.ln1_b.as<float>(), c.ln_eps, h, rows_pad, d, stream, 0, 0, L.w_1.p, (size_t)f * d * 2, sf16));
    HIP_TRY(launch_gemm_tn(EPI_BIAS_F16, h, L.w_qkv.as<f16>(), L.b_qkv.as<float>(), kvl + (size_t)pos * slab,
                           rows_pad, 3 * d, d, 3 * d, stream));
    HIP_TRY(launch_dec_attention(kvl, anc, anc_stride, ctx, rows, rows_pad, d, c.num_heads, pos, stream));
    // the two N = d projections have too few tiles to fill 256 CUs at decode batch sizes:
    // split K into fp32 slabs that the next fused sum+LayerNorm folds into the residual stream
    if (ks_out == 1)  // no split: the projection adds into the fp32 residual stream itself
      HIP_TRY(launch_gemm_tn(EPI_RESID_F32, ctx, L.w_o.as<f16>(), L.b_o.as<float>(), x, rows_pad, d, d, d, stream));
    else
      HIP_TRY(launch_gemm_tn_splitk(ctx, L.w_o.as<f16>(), L.b_o.as<float>(), parts, rows_pad, d, d, ks_out, stream, 0, sf16));
    // the FFN runs on tile-major operands (common.hpp): LN output, hidden activation and both weights
    const int tm = D->ffn_tile_major;
    HIP_TRY(launch_sum_layernorm(x, ks_out == 1 ? nullptr : parts, ks_out, part_stride,
                                 S.cc.as<float>() + (size_t)l * n_pad * d, group, L.ln3_w.as<float>(), L.ln3_b.as<float>(),
                                 c.ln_eps, h, rows, d, stream, tm, 0, L.w_2.p, (size_t)f * d * 2, sf16));
    HIP_TRY(launch_gemm_tn(EPI_RELU_F16 | (tm ? GEMM_IN_TM | GEMM_OUT_TM : 0) | (ffn1_engine << 8), h, L.w_1.as<f16>(),
                           L.b_1.as<float>(), ffn, rows_pad, f, d, f, stream));
    HIP_TRY(launch_gemm_tn_splitk(ffn, L.w_2.as<f16>(), L.b_2.as<float>(), parts, rows_pad, d, f, ks_ffn, stream, tm, sf16));
  }
  const int ltm = D->embed_tm.p != nullptr;  // the tied projection reads a tile-major copy of the table
  HIP_TRY(launch_sum_layernorm(x, c.num_layers ? parts : nullptr, ks_ffn, part_stride, nullptr, 1,
                               D->lnf_w.as<float>(), D->lnf_b.as<float>(), c.ln_eps, h, rows_pad, d, stream, ltm, 0, nullptr, 0,
                               sf16));
  // beam search (stats_scale = 1 / temperature > 0): the GEMM also leaves per-tile softmax
  // statistics, so the candidate selection never re-reads the 1 MB logits rows
  GemmTileStats st{S.tile_max.as<float>(), S.tile_sum.as<float>(), stats_scale, (int)c.vocab_size};
  if (S.chained && logits_grid_env > 0) set_gemm_grid_cap(logits_grid_env);
  const hipError_t le =
      logits_f16 && ltm && stats_scale > 0.f
          ? launch_gemm_tn(EPI_BIAS_F16 | GEMM_IN_TM | GEMM_OUT_TM, h, D->embed_tm.as<f16>(), nullptr, S.logits.p, rows_pad,
                           (int)D->vocab_pad, d, (int)D->vocab_pad, stream, &st)
          : launch_gemm_tn(EPI_STORE_F32 | (ltm ? GEMM_IN_TM : 0), h, (ltm ? D->embed_tm : D->embed).as<f16>(), nullptr,
                           S.logits.p, rows_pad, (int)D->vocab_pad, d, (int)D->vocab_pad, stream,
                           stats_scale > 0.f ? &st : nullptr);
  set_gemm_grid_cap(0);
  HIP_TRY(le);
  return SMI_OK;
}

int ensure_step_workspace(smi_text_decoder* D, DecWork& S, int rows_pad, int positions, hipStream_t stream) {
  const smi_text_decoder_config& c = D->cfg;
  const size_t d = c.model_dim, f = c.ffn_inner_dim;
  const size_t before = S.x.bytes + S.h.bytes + S.ctx.bytes + S.ffn.bytes;
  const size_t es = D->act_bytes();
  S.tuning.read();
  HIP_TRY(S.x.reserve((size_t)rows_pad * d * 4));
  HIP_TRY(S.h.reserve((size_t)rows_pad * d * es));
  HIP_TRY(S.ctx.reserve((size_t)rows_pad * d * es));
  HIP_TRY(S.ffn.reserve((size_t)rows_pad * f * es));
  HIP_TRY(S.logits.reserve((size_t)rows_pad * D->vocab_pad * 4));
  HIP_TRY(S.parts.reserve((size_t)kMaxParts * rows_pad * d * 4));
  // kv cache for this call: [layers][positions][rows_pad][3d] (q|k|v slabs written by the QKV GEMM).
  // `positions` may be smaller than the generation cap: grow_kv() extends the cache when a call
  // actually decodes that far (the cap is max_seq_len = 512 for sentence vectors, fairseq2's
  // a * source_len + b rule; typical outputs stop after a few dozen tokens).
  {
    const size_t per_pos = (size_t)c.num_layers * rows_pad * 3 * d * es;
    const int have = per_pos ? (int)std::min<size_t>(S.kv.bytes / per_pos, (size_t)c.max_seq_len) : 0;
    if (have >= positions) {
      S.kv_positions = have;
    } else {
      HIP_TRY(S.kv.reserve(per_pos * positions));
      S.kv_positions = positions;
    }
  }
  if (S.x.bytes + S.h.bytes + S.ctx.bytes + S.ffn.bytes != before) {
    // tile-padding rows are read by the GEMMs: keep them finite
    // (stream-ordered: a chain's stream does not synchronise with the null stream a plain hipMemset runs on)
    HIP_TRY(hipMemsetAsync(S.x.p, 0, S.x.bytes, stream));
    HIP_TRY(hipMemsetAsync(S.h.p, 0, S.h.bytes, stream));
    HIP_TRY(hipMemsetAsync(S.ctx.p, 0, S.ctx.bytes, stream));
    HIP_TRY(hipMemsetAsync(S.ffn.p, 0, S.ffn.bytes, stream));
  }
  return SMI_OK;
}

// the decode loop reached the end of the kv allocation: move the slabs written so far into a cache
// with room for `positions` positions per layer (layout [layer][position][rows_pad][3d])
int grow_kv(smi_text_decoder* D, DecWork& S, int rows_pad, int positions, hipStream_t stream) {
  const smi_text_decoder_config& c = D->cfg;
  const size_t slab = (size_t)rows_pad * 3 * c.model_dim * D->act_bytes();  // bytes per (layer, position)
  const int old_p = S.kv_positions;
  if (positions <= old_p) return SMI_OK;
  DevBuf bigger;
  HIP_TRY(bigger.alloc((size_t)c.num_layers * positions * slab));
  for (int l = 0; l < c.num_layers; ++l)
    HIP_TRY(hipMemcpyAsync((char*)bigger.p + (size_t)l * positions * slab, (char*)S.kv.p + (size_t)l * old_p * slab,
                           (size_t)old_p * slab, hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  S.kv = std::move(bigger);
  S.kv_positions = positions;
  return SMI_OK;
}

constexpr int kKvInitialPositions = 160;

// Number of independent chains for a beam-search call (smi_text_decoder_set_chains, or the tuning switch TUNE_DEC_CHAINS).
// Measured on the `basic` decoder, beam 5, ms per step (profiles/r04_experiments.txt, experiment 1):
//   sentences (rows)   1 chain   2 chains   3 chains   4 chains
//   256  (1280)          3.88      4.16-4.25    4.97
//   512  (2560)          7.71      6.23
//   768  (3840)         10.03      9.68       9.18
//   1024 (5120)         13.57     13.22      12.61      13.22
// 1280 rows are 160 lone FFN tiles -- one round on 256 CUs -- and splitting them only makes every co-running launch 20-30 %
// slower (kernel trace: 65 % of the time two kernels in flight, each longer than alone); from 2560 rows on the FFN tiles need
// a second round and chains of ~1280 rows win, up to three of them (a fourth costs more in contention than it hides).
int decode_chains(const smi_text_decoder* D, int n, int beam) {
  const int env = tune(TUNE_DEC_CHAINS, 0);
  if (D->flex) return 1;
  const int64_t rows_pad = round_up((int64_t)n * beam, 256);
  const int automatic = rows_pad <= 2048 ? 1 : (int)std::min<int64_t>(3, (rows_pad + 1279) / 1280);
  int g = D->chains > 0 ? D->chains : (env > 0 ? env : automatic);
  g = std::min(g, kMaxChains);
  // every chain keeps at least two 256-row tiles of hypotheses: below that a chain's launches are all fixed cost
  while (g > 1 && (int64_t)((n + g - 1) / g) * beam < 384) --g;
  return std::max(g, 1);
}

// the step-processor table is read by the work queued so far on `stream` (smi_text_decoder_set_step_processors waits for it)
int record_table_use(DecWork& S, hipStream_t stream) {
  if (!S.sp_ev) HIP_TRY(hipEventCreateWithFlags(&S.sp_ev, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(S.sp_ev, stream));
  return SMI_OK;
}

// The prompts and length limits of a generate / sample call, or of one sentence group of it: what the
// launch schedule is planned from.  Per-sentence prompts (the *_prompts entries): sentence s has the prompt
// tok[s * stride .. + len[s]) and its own max_len_s / min_len_s, and `dev` is the same n sentences on the device.  A call
// with ONE prompt is the degenerate plan: stride 0 (every sentence reads tok[0 ..]), no `len`, no device table
// (dev.tok == nullptr), every range below a single value.
struct PromptPlan {
  int n = 0;
  const int64_t* tok = nullptr;  // host, left-aligned rows
  const int32_t* len = nullptr;  // host [n]
  int stride = 0;
  int width = 0;                 // max over the CALL's sentences of max_len_s: the output row length
  PromptTableDev dev{};
  // over the n sentences: prompt lengths, min_len_s, max_len_s
  int pmin = 0, pmax = 0, minlen_lo = 0, minlen_hi = 0, maxlen_lo = 0, maxlen_hi = 0;

  bool one_prompt() const { return dev.tok == nullptr; }
  // the prompt length the kernels get as a scalar (per-sentence prompts: they take it from the table)
  int scalar_prompt_len() const { return one_prompt() ? pmax : 0; }

  static PromptPlan one(int n, const int64_t* prompt, int prompt_len, int max_len, int min_len) {
    PromptPlan p;
    p.n = n; p.tok = prompt; p.width = max_len;
    p.pmin = p.pmax = prompt_len;
    p.minlen_lo = p.minlen_hi = min_len;
    p.maxlen_lo = p.maxlen_hi = max_len;
    return p;
  }
  // the sentences [s0, s0 + ng) of a per-sentence plan (dev holds gen_cap / min_gen / model_max)
  PromptPlan group(int s0, int ng) const {
    PromptPlan p = *this;
    p.n = ng;
    if (one_prompt()) return p;
    p.tok += (size_t)s0 * stride; p.len += s0;
    p.dev.tok += (size_t)s0 * stride; p.dev.len += s0;
    p.pmin = p.minlen_lo = p.maxlen_lo = INT32_MAX;
    p.pmax = p.minlen_hi = p.maxlen_hi = 0;
    for (int s = 0; s < ng; ++s) {
      const int pl = p.len[s], mx = std::min(pl + dev.gen_cap, dev.model_max), mn = std::min(pl + dev.min_gen, mx);
      p.pmin = std::min(p.pmin, pl); p.pmax = std::max(p.pmax, pl);
      p.minlen_lo = std::min(p.minlen_lo, mn); p.minlen_hi = std::max(p.minlen_hi, mn);
      p.maxlen_lo = std::min(p.maxlen_lo, mx); p.maxlen_hi = std::max(p.maxlen_hi, mx);
    }
    return p;
  }
};

// What the plan's sentences have in common at the step that chooses token `step_nr`.  Where every sentence is in one mode
// the step keeps the one-prompt launches (scalar arguments); only a kMixed step -- and a forced step whose tokens differ
// (forced_tok < 0) -- makes the kernels take each sentence's mode from the table.  A one-prompt plan is never mixed.
struct StepMode {
  enum Kind { kForced, kForceEos, kFree, kMixed } kind;
  int forced_tok;  // kForced: the prompt token every sentence takes, or -1 (per-sentence prompts)
  bool block_eos;  // kFree: every sentence is below its min_len
  bool free_step() const { return kind == kFree || kind == kMixed; }
};
StepMode step_mode(const PromptPlan& p, int step_nr) {
  if (step_nr < p.pmin) return {StepMode::kForced, p.one_prompt() ? (int)p.tok[step_nr] : -1, false};
  if (step_nr >= p.pmax && p.maxlen_lo == p.maxlen_hi && step_nr == p.maxlen_lo - 1) return {StepMode::kForceEos, -1, false};
  // every sentence on a free step, and all of them on the same side of their min_len
  if (step_nr >= p.pmax && step_nr < p.maxlen_lo - 1) {
    if (step_nr < p.minlen_lo) return {StepMode::kFree, -1, true};
    if (step_nr >= p.minlen_hi) return {StepMode::kFree, -1, false};
  }
  return {StepMode::kMixed, -1, false};
}

// The plan of a one-prompt call: bp / sp carry absolute lengths that hold for every sentence.
int plan_one_prompt(const smi_text_decoder_config& c, int n, const int64_t* prompt, int prompt_len, int max_len, int min_len,
                    PromptPlan* plan) {
  if (prompt_len <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  if (max_len > c.max_seq_len || max_len <= prompt_len)
    return fail(SMI_ERR_INVALID_ARG, "max_seq_len %d must be in (prompt_len %d, model max %d]", max_len, prompt_len,
                c.max_seq_len);
  for (int i = 0; i < prompt_len; ++i)
    if (prompt[i] < 0 || prompt[i] >= c.vocab_size) return fail(SMI_ERR_INVALID_ARG, "prompt token out of range");
  *plan = PromptPlan::one(n, prompt, prompt_len, max_len, min_len);
  return SMI_OK;
}

// The plan of a *_prompts call: max_len_s = min(len_s + gen_cap, model_max), min_len_s = min(len_s + min_gen, max_len_s).
// Checks the prompts; if they are all equal the call IS a one-prompt call and gets that plan (launch for launch), else the
// table (int32 tokens [n][stride], then lengths [n]) goes to D->ws[0].prompt_dev, uploaded on return.
int plan_prompts(smi_text_decoder* D, int n, const int64_t* prompts, int stride, const int32_t* lens, int gen_cap, int min_gen,
                 int model_max, hipStream_t stream, PromptPlan* plan) {
  const smi_text_decoder_config& c = D->cfg;
  if (stride < 1) return fail(SMI_ERR_INVALID_ARG, "prompt_stride %d must be positive", stride);
  if (gen_cap < 1 || min_gen < 0) return fail(SMI_ERR_INVALID_ARG, "gen_cap %d must be >= 1 and min_gen_len %d >= 0", gen_cap, min_gen);
  if (model_max > c.max_seq_len || model_max < 2)
    return fail(SMI_ERR_INVALID_ARG, "max_seq_len %d must be in [2, model max %d]", model_max, c.max_seq_len);
  std::vector<int32_t> tab((size_t)n * stride + n, 0);
  int width = 0;
  bool all_equal = true;
  for (int s = 0; s < n; ++s) {
    const int pl = lens[s];
    if (pl < 1 || pl > stride) return fail(SMI_ERR_INVALID_ARG, "prompt_lens[%d] = %d outside [1, prompt_stride %d]", s, pl, stride);
    if (std::min(pl + gen_cap, model_max) <= pl)
      return fail(SMI_ERR_INVALID_ARG, "row %d: max_seq_len %d leaves no room for generation after its prompt of %d tokens", s,
                  model_max, pl);
    all_equal = all_equal && pl == lens[0];
    for (int i = 0; i < pl; ++i) {
      const int64_t t = prompts[(size_t)s * stride + i];
      if (t < 0 || t >= c.vocab_size) return fail(SMI_ERR_INVALID_ARG, "row %d: prompt token %lld out of range", s, (long long)t);
      tab[(size_t)s * stride + i] = (int32_t)t;
      all_equal = all_equal && (i >= lens[0] || t == prompts[i]);
    }
    tab[(size_t)n * stride + s] = pl;
    width = std::max(width, std::min(pl + gen_cap, model_max));
  }
  if (all_equal) {  // every max_len_s is the width
    *plan = PromptPlan::one(n, prompts, lens[0], width, std::min(lens[0] + min_gen, width));
    return SMI_OK;
  }
  DevBuf& b = D->ws[0].prompt_dev;
  HIP_TRY(b.reserve(tab.size() * 4));
  HIP_TRY(hipMemcpyAsync(b.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  PromptPlan whole;
  whole.tok = prompts; whole.len = lens; whole.stride = stride; whole.width = width;
  whole.dev = PromptTableDev{b.as<int32_t>(), b.as<int32_t>() + (size_t)n * stride, stride, gen_cap, min_gen, model_max};
  *plan = whole.group(0, n);
  return SMI_OK;
}

// has every one of the n sentences finished?  (waits for the work queued on `stream`)
int all_sentences_done(DecWork& S, int n, hipStream_t stream, bool* done) {
  int32_t nd = 0;
  HIP_TRY(hipMemcpyAsync(&nd, S.ndone.p, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  *done = nd >= n;
  return SMI_OK;
}

// one hypothesis per sentence: anc[0][r][j] = r for the n rows (finished on return)
int upload_identity_ancestry(DecWork& S, int n, int stride, hipStream_t stream) {
  std::vector<int32_t> ident((size_t)n * stride);
  for (int r = 0; r < n; ++r)
    for (int j = 0; j < stride; ++j) ident[(size_t)r * stride + j] = r;
  HIP_TRY(hipMemcpyAsync(S.anc[0].p, ident.data(), ident.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return SMI_OK;
}

// One decode chain: beam search for the n sentences of `emb` on workspace S and stream `stream` (the whole call, or
// one sentence group of a split call).  margins: device [n][2].  The plan carries the prompts and the length limits
// (bp->max_seq_len / min_seq_len are not read here).
int generate_chain(smi_text_decoder* D, DecWork& S, const void* emb, int emb_dtype, const PromptPlan& plan,
                   const smi_beam_search_params* bp, int32_t* out_tokens, int32_t* out_lens, float* out_scores,
                   float* margins, hipStream_t stream) {
  const smi_text_decoder_config& c = D->cfg;
  const int n = plan.n, beam = bp->beam_size;
  // the loop runs to the group's longest cap, the output rows are as wide as the call's
  const int max_len = plan.maxlen_hi, out_stride = plan.width;

  const int rows = n * beam;
  const int rows_pad = (int)round_up(rows, 256), n_pad = (int)round_up(n, 256);
  const int stride = c.max_seq_len + 1;
  const int k2 = 2 * beam;
  if (int rc = ensure_step_workspace(D, S, rows_pad, std::min(max_len, kKvInitialPositions), stream)) return rc;
  HIP_TRY(S.tok.reserve((size_t)rows_pad * 4));
  HIP_TRY(S.cum.reserve((size_t)rows * 4));
  HIP_TRY(S.parent.reserve((size_t)rows * 4));
  HIP_TRY(S.new_tok.reserve((size_t)rows * 4));
  HIP_TRY(S.new_cum.reserve((size_t)rows * 4));
  HIP_TRY(S.nactive.reserve((size_t)n * 4));
  HIP_TRY(S.done.reserve((size_t)n * 4));
  HIP_TRY(S.ndone.reserve(4));
  HIP_TRY(S.fin_count.reserve((size_t)n * 4));
  HIP_TRY(S.fin_len.reserve((size_t)rows * 4));
  HIP_TRY(S.fin_score.reserve((size_t)rows * 4));
  HIP_TRY(S.fin_tok.reserve((size_t)rows * stride * 4));
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(S.anc[i].reserve((size_t)rows_pad * stride * 4));
    HIP_TRY(S.hist[i].reserve((size_t)rows_pad * stride * 4));
  }
  const int ntiles = (int)(D->vocab_pad / 256);
  HIP_TRY(S.pmax.reserve((size_t)rows * 4));
  HIP_TRY(S.psum.reserve((size_t)rows * 4));
  HIP_TRY(S.pval.reserve((size_t)rows * kVocabScanK2Max * 4));
  HIP_TRY(S.pidx.reserve((size_t)rows * kVocabScanK2Max * 4));
  HIP_TRY(S.tile_max.reserve((size_t)rows_pad * ntiles * 4));
  HIP_TRY(S.tile_sum.reserve((size_t)rows_pad * ntiles * 4));

  if (int rc = compute_cross_constants(D, S, emb, emb_dtype, n, n_pad, stream)) return rc;
  HIP_TRY(launch_beam_init(S.tok.as<int32_t>(), S.cum.as<float>(), S.nactive.as<int32_t>(),
                           S.done.as<int32_t>(), S.ndone.as<int32_t>(), S.fin_count.as<int32_t>(),
                           S.hist[0].as<int32_t>(), S.anc[0].as<int32_t>(), margins, rows, n, stride,
                           plan.one_prompt() ? (int)plan.tok[0] : 0, stream, plan.dev.tok, plan.dev.stride, beam));
  const float inv_temp = 1.0f / bp->temperature;
  // fp16 logits: the handle's setting (the tuning switch TUNE_DEC_LOGITS_F16 = 0 / 1 overrides it: A/B runs), MFMA path with the tile-major table
  const int lf_env = tune(TUNE_DEC_LOGITS_F16, -1);
  const int logits_f16 = !D->flex && D->embed_tm.p != nullptr && (lf_env >= 0 ? lf_env != 0 : D->beam_logits_f16 != 0);
  const int sf_env = tune(TUNE_DEC_SLAB_F16, -1);
  const int slab_f16 = !D->flex && (sf_env >= 0 ? sf_env != 0 : D->beam_slab_f16 != 0);
  const StepProcDev proc = D->sp.dev;

  // everything one decode step enqueues (position pos; ancestry/history buffer pos & 1)
  auto enqueue_step = [&](int pos, hipStream_t s) -> int {
    const int cur = pos & 1, step_nr = pos + 1;
    if (int rc = decoder_step(D, S, rows, rows_pad, beam, n_pad, pos, S.anc[cur].as<int32_t>(), stride, s, inv_temp,
                              logits_f16, slab_f16))
      return rc;
    const StepMode mode = step_mode(plan, step_nr);
    // forced steps need only the softmax normaliser (the candidate is a given token): k2 = 0
    const bool free_step = mode.free_step();
    VocabSelectArgs v{};
    v.logits = S.logits.as<float>(); v.ldl = (int)D->vocab_pad; v.f16_tm = logits_f16; v.rows = rows; v.vocab = (int)c.vocab_size;
    v.tile_max = S.tile_max.as<float>(); v.tile_sum = S.tile_sum.as<float>(); v.ntiles = ntiles; v.stat_rows = rows_pad;
    v.k2 = free_step ? k2 : 0; v.inv_temp = inv_temp; v.pad_idx = c.pad_idx; v.eos_idx = c.eos_idx; v.unk_idx = c.unk_idx;
    v.unk_penalty = free_step ? bp->unk_penalty : 0.f; v.block_eos = mode.block_eos ? 1 : 0;
    v.pmax = S.pmax.as<float>(); v.psum = S.psum.as<float>(); v.pval = S.pval.as<float>(); v.pidx = S.pidx.as<int>();
    // step processors act on the free steps only, on the row's sequence so far hist[cur][r][0 .. pos]
    if (free_step && proc.active()) {
      v.hist = S.hist[cur].as<int32_t>(); v.hist_stride = stride; v.hist_len = pos + 1; v.proc = proc;
    }
    if (mode.kind == StepMode::kMixed) v.table = plan.dev;
    v.group = beam; v.step_nr = step_nr;
    HIP_TRY(launch_vocab_select(v, s));
    BeamStepArgs a{};
    a.tok = S.tok.as<int32_t>(); a.cum = S.cum.as<float>(); a.nactive = S.nactive.as<int32_t>();
    a.done = S.done.as<int32_t>(); a.ndone = S.ndone.as<int32_t>();
    a.parent = S.parent.as<int32_t>(); a.new_tok = S.new_tok.as<int32_t>(); a.new_cum = S.new_cum.as<float>();
    a.hist = S.hist[cur].as<int32_t>(); a.fin_tok = S.fin_tok.as<int32_t>(); a.fin_len = S.fin_len.as<int32_t>();
    a.fin_score = S.fin_score.as<float>(); a.fin_count = S.fin_count.as<int32_t>();
    a.margins = margins;
    a.logits = S.logits.as<float>(); a.ldl = (int)D->vocab_pad; a.logits_f16_tm = logits_f16;
    a.pmax = S.pmax.as<float>(); a.psum = S.psum.as<float>(); a.pval = S.pval.as<float>(); a.pidx = S.pidx.as<int>();
    a.n = n; a.beam = beam; a.k2 = k2; a.pos = pos; a.prompt_len = plan.scalar_prompt_len();
    a.forced_tok = mode.forced_tok; a.max_len = max_len;
    if (!plan.one_prompt()) {
      // prompts of one length: past them the sentences differ in nothing the beam step reads -- the one-prompt launch
      if (plan.pmin == plan.pmax && step_nr >= plan.pmax) a.prompt_len = plan.pmax;
      else a.table = plan.dev;
    }
    a.inv_temp = inv_temp; a.len_penalty = bp->len_penalty; a.normalize = bp->normalize_scores;
    a.eos_idx = c.eos_idx; a.hist_stride = stride;
    HIP_TRY(launch_beam_step(a, s));
    HIP_TRY(launch_beam_reorder(S.parent.as<int32_t>(), S.new_tok.as<int32_t>(), S.new_cum.as<float>(),
                                S.anc[cur].as<int32_t>(), S.anc[cur ^ 1].as<int32_t>(), S.hist[cur].as<int32_t>(),
                                S.hist[cur ^ 1].as<int32_t>(), S.tok.as<int32_t>(), S.cum.as<float>(), rows, stride,
                                pos, s));
    return SMI_OK;
  };

  // (A hipGraph cache of this step -- one captured graph per position, replayed on later calls -- was
  // measured at 256 x beam 5 and 16 x beam 5: 447.1 vs 447.3 ms and 185.4 vs 184.9 ms per 65 steps.  The
  // step is bound by the GPU front end's dependent-dispatch latency of ~180 short kernels, not by host
  // launch cost, so plain launches stay; fewer, fatter kernels are the lever.  DESIGN.md 3.4.)
  for (int pos = 0; pos + 1 < max_len; ++pos) {
    const int step_nr = pos + 1;
    if (pos >= S.kv_positions)
      if (int rc = grow_kv(D, S, rows_pad, std::min(max_len, 2 * S.kv_positions), stream)) return rc;
    if (int rc = enqueue_step(pos, stream)) return rc;
    // every 8 steps, and after the last one: has every sentence collected its `beam` hypotheses?
    if ((step_nr & 7) == 0 || step_nr == max_len - 1) {
      bool done = false;
      if (int rc = all_sentences_done(S, n, stream, &done)) return rc;
      if (done) break;
    }
  }
  HIP_TRY(launch_beam_output(S.fin_tok.as<int32_t>(), S.fin_len.as<int32_t>(), S.fin_score.as<float>(),
                             S.fin_count.as<int32_t>(), n, beam, stride, out_stride, out_tokens, out_lens, out_scores,
                             margins, stream));
  if (proc.active())
    if (int rc = record_table_use(S, stream)) return rc;
  return SMI_OK;
}

// Teacher-forced scoring (smi_text_decoder_score).  A group of ns sentences is ns * seq uniform rows
// r = s * seq + j (input position j, target tok[s][j + 1]); the whole forward runs once over them.
constexpr int kScoreRows = 16384;              // rows per sentence group: bounds the activation workspace
constexpr int64_t kScoreLogitBytes = 2ll << 30;  // fp32 logits of one projection chunk

int score_rows_per_chunk(const smi_text_decoder* D, int rows) {
  const int64_t fit = kScoreLogitBytes / (D->vocab_pad * 4) / 256 * 256;
  return (int)std::max<int64_t>(256, std::min<int64_t>(fit, round_up(rows, 256)));
}

int score_group(smi_text_decoder* D, DecWork& S, const void* emb, int emb_dtype, int ns, const int64_t* tokens, int t,
                const int32_t* lens_dev, int seq, float* out, hipStream_t stream) {
  const smi_text_decoder_config& c = D->cfg;
  const int d = c.model_dim, f = c.ffn_inner_dim, L = c.num_layers;
  const int rows = ns * seq, n_pad = (int)round_up(ns, 256);
  // the MFMA GEMMs take 256-row tiles; the flex kernels any row count
  const int rows_pad = D->flex ? rows : (int)round_up(rows, 256);
  const size_t es = D->act_bytes();
  const int chunk = score_rows_per_chunk(D, rows);
  const int ntiles = (int)(D->vocab_pad / 256);
  HIP_TRY(S.x.reserve((size_t)rows_pad * d * 4));
  HIP_TRY(S.h.reserve((size_t)rows_pad * d * es));
  HIP_TRY(S.ctx.reserve((size_t)rows_pad * d * es));
  HIP_TRY(S.ffn.reserve((size_t)rows_pad * f * es));
  HIP_TRY(S.kv.reserve((size_t)rows_pad * 3 * d * es));  // the group's q | k | v rows
  HIP_TRY(S.logits.reserve((size_t)chunk * D->vocab_pad * 4));
  HIP_TRY(S.tile_max.reserve((size_t)chunk * ntiles * 4));
  HIP_TRY(S.tile_sum.reserve((size_t)chunk * ntiles * 4));
  HIP_TRY(S.sc_tgt.reserve((size_t)rows_pad * 4));
  if (int rc = compute_cross_constants(D, S, emb, emb_dtype, ns, n_pad, stream)) return rc;
  // rows past a sentence's length embed the EOS id: finite activations that no scored row reads (causal, padding last)
  HIP_TRY(launch_score_embed(tokens, t, lens_dev, D->embed.p, D->flex ? 0 : 1, D->pos.as<float>(), c.embed_scale, c.pos_offset,
                             S.x.as<float>(), S.sc_tgt.as<int32_t>(), ns, seq, rows_pad, d, c.vocab_size, c.eos_idx,
                             S.sc_bad.as<int32_t>(), stream));
  float* x = S.x.as<float>();
  const float* cc = S.cc.as<float>();
  if (D->flex) {
    float* h = S.h.as<float>();
    float* qkv = S.kv.as<float>();
    float* ctx = S.ctx.as<float>();
    float* ffn = S.ffn.as<float>();
    for (int l = 0; l < L; ++l) {
      DecLayer& Ly = D->layers[l];
      HIP_TRY(launch_flex_layernorm(x, Ly.ln1_w.as<float>(), Ly.ln1_b.as<float>(), c.ln_eps, h, rows, d, stream));
      HIP_TRY(launch_flex_linear(h, d, Ly.w_qkv.as<float>(), Ly.b_qkv.as<float>(), qkv, 3 * d, rows, 3 * d, d, 0, nullptr, 0,
                                 stream));
      HIP_TRY(launch_flex_attention(qkv, 3 * d, qkv + d, qkv + 2 * d, 3 * d, ctx, d, ns, seq, seq, nullptr, c.num_heads,
                                    d / c.num_heads, 1, stream));
      HIP_TRY(launch_flex_linear(ctx, d, Ly.w_o.as<float>(), Ly.b_o.as<float>(), x, d, rows, d, d, 0, x, d, stream));
      HIP_TRY(launch_flex_add_rows(x, cc + (size_t)l * n_pad * d, rows, d, seq, stream));
      HIP_TRY(launch_flex_layernorm(x, Ly.ln3_w.as<float>(), Ly.ln3_b.as<float>(), c.ln_eps, h, rows, d, stream));
      HIP_TRY(launch_flex_linear(h, d, Ly.w_1.as<float>(), Ly.b_1.as<float>(), ffn, f, rows, f, d, 1, nullptr, 0, stream));
      HIP_TRY(launch_flex_linear(ffn, f, Ly.w_2.as<float>(), Ly.b_2.as<float>(), x, d, rows, d, f, 0, x, d, stream));
    }
    HIP_TRY(launch_flex_layernorm(x, D->lnf_w.as<float>(), D->lnf_b.as<float>(), c.ln_eps, h, rows, d, stream));
    for (int c0 = 0; c0 < rows; c0 += chunk) {
      const int m = std::min(chunk, rows - c0);
      HIP_TRY(launch_flex_linear(h + (size_t)c0 * d, d, D->embed.as<float>(), nullptr, S.logits.as<float>(), (int)D->vocab_pad,
                                 m, (int)c.vocab_size, d, 0, nullptr, 0, stream));
      HIP_TRY(launch_flex_tile_stats(S.logits.as<float>(), (int)D->vocab_pad, m, (int)c.vocab_size, 1.f,
                                     S.tile_max.as<float>(), S.tile_sum.as<float>(), m, stream));
      HIP_TRY(launch_score_gather(S.logits.as<float>(), D->vocab_pad, S.tile_max.as<float>(), S.tile_sum.as<float>(), ntiles, m,
                                  S.sc_tgt.as<int32_t>(), c0, m, seq, out, t - 1, stream));
    }
    return SMI_OK;
  }
  f16* h = S.h.as<f16>();
  f16* qkv = S.kv.as<f16>();
  f16* ctx = S.ctx.as<f16>();
  f16* ffn = S.ffn.as<f16>();
  // the attention writes the group's rows only: keep the GEMM padding rows of its output finite
  if (rows_pad > rows) HIP_TRY(hipMemsetAsync(ctx + (size_t)rows * d, 0, (size_t)(rows_pad - rows) * d * 2, stream));
  const int tm = D->ffn_tile_major;
  // the layer GEMMs stay on the 128x128 engine family whatever the row count: the automatic choice moves to the 256x256 and
  // 4-wave engines as M grows, and their fp32 summation orders differ, so a sentence's scores would depend on its company
  const int fam = 1 << 8;
  for (int l = 0; l < L; ++l) {
    DecLayer& Ly = D->layers[l];
    HIP_TRY(launch_sum_layernorm(x, nullptr, 0, 0, nullptr, 1, Ly.ln1_w.as<float>(), Ly.ln1_b.as<float>(), c.ln_eps, h,
                                 rows_pad, d, stream));
    HIP_TRY(launch_gemm_tn(EPI_BIAS_F16 | fam, h, Ly.w_qkv.as<f16>(), Ly.b_qkv.as<float>(), qkv, rows_pad, 3 * d, d, 3 * d, stream));
    HIP_TRY(launch_causal_attention(qkv, S.sc_cu.as<int32_t>(), ctx, ns, seq, d, c.num_heads, stream));
    HIP_TRY(launch_gemm_tn(EPI_RESID_F32 | fam, ctx, Ly.w_o.as<f16>(), Ly.b_o.as<float>(), x, rows_pad, d, d, d, stream));
    // + the sentence's cross-attention constant (row r -> sentence r / seq < ns; the padding rows past ns * seq are not
    // touched, so they never index past the n_pad reserved constant rows), then LN3
    HIP_TRY(launch_sum_layernorm(x, nullptr, 0, 0, cc + (size_t)l * n_pad * d, seq, Ly.ln3_w.as<float>(), Ly.ln3_b.as<float>(),
                                 c.ln_eps, h, rows, d, stream, tm));
    HIP_TRY(launch_gemm_tn(EPI_RELU_F16 | fam | (tm ? GEMM_IN_TM | GEMM_OUT_TM : 0), h, Ly.w_1.as<f16>(), Ly.b_1.as<float>(), ffn,
                           rows_pad, f, d, f, stream));
    HIP_TRY(launch_gemm_tn(EPI_RESID_F32 | fam | (tm ? GEMM_IN_TM : 0), ffn, Ly.w_2.as<f16>(), Ly.b_2.as<float>(), x, rows_pad, d, f,
                           d, stream));
  }
  const int ltm = D->embed_tm.p != nullptr;  // the tied projection reads a tile-major copy of the table
  HIP_TRY(launch_sum_layernorm(x, nullptr, 0, 0, nullptr, 1, D->lnf_w.as<float>(), D->lnf_b.as<float>(), c.ln_eps, h, rows_pad,
                               d, stream, ltm));
  // the logits GEMM in chunks of whole 256-row tiles (a tile-major chunk is contiguous), with the fused per-tile softmax
  // statistics at scale 1: the gather reads the statistics and the target's single logit, never the 1 MB row
  GemmTileStats st{S.tile_max.as<float>(), S.tile_sum.as<float>(), 1.f, (int)c.vocab_size};
  for (int c0 = 0; c0 < rows; c0 += chunk) {
    const int m = std::min(chunk, rows_pad - c0);
    HIP_TRY(launch_gemm_tn(EPI_STORE_F32 | (ltm ? GEMM_IN_TM : 0), h + (size_t)c0 * d, (ltm ? D->embed_tm : D->embed).as<f16>(),
                           nullptr, S.logits.p, m, (int)D->vocab_pad, d, (int)D->vocab_pad, stream, &st));
    HIP_TRY(launch_score_gather(S.logits.as<float>(), D->vocab_pad, S.tile_max.as<float>(), S.tile_sum.as<float>(), ntiles, m,
                                S.sc_tgt.as<int32_t>(), c0, std::min(m, rows - c0), seq, out, t - 1, stream));
  }
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_text_decoder_create(const smi_text_decoder_config* cfg, const smi_text_decoder_weights* w,
                            smi_text_decoder** out) {
  if (!cfg || !w || !out) return fail(SMI_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  bool flex = false;
  if (int rc = check_dec_cfg(*cfg, &flex)) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  if (cfg->num_layers > 0 && !w->layers) return fail(SMI_ERR_INVALID_ARG, "null layers");
  smi_text_decoder* D = new smi_text_decoder();
  D->cfg = *cfg;
  D->flex = flex;
  D->vocab_pad = round_up(cfg->vocab_size, 256);
  const int64_t d = cfg->model_dim, f = cfg->ffn_inner_dim, ci = cfg->input_dim;
  int rc = SMI_OK;
  // flex mode keeps every tensor fp32 (upload converts); the MFMA mode wants fp16 matrices
  auto up = [&](const smi_tensor& t, int64_t numel, bool f16w, DevBuf& dst, const char* name, int64_t pad = 0) {
    if (rc == SMI_OK) rc = upload(t, numel, f16w && !flex, dst, name, pad);
  };
  // the tied output projection multiplies by the embedding table: pad it to 256-row tiles
  up(w->embed, cfg->vocab_size * d, true, D->embed, "decoder_frontend.embed.weight", D->vocab_pad * d);
  if (rc == SMI_OK && !flex && d % 256 == 0) {  // [vocab_pad][d] -> tile-major (common.hpp), ~0.5 GB for NLLB
    rc = upload(w->embed, cfg->vocab_size * d, true, D->embed_tm, "decoder_frontend.embed.weight", D->vocab_pad * d);
    if (rc == SMI_OK) rc = to_tile_major(D->embed_tm, (int)D->vocab_pad, (int)d);
  }
  up(w->pos_table, (int64_t)(cfg->max_seq_len + cfg->pos_offset) * d, false, D->pos, "pos_table");
  up(w->final_layer_norm_w, d, false, D->lnf_w, "decoder.layer_norm.weight");
  up(w->final_layer_norm_b, d, false, D->lnf_b, "decoder.layer_norm.bias");
  D->ffn_tile_major = !flex && d % 256 == 0 && f % 256 == 0;
  D->layers.resize(cfg->num_layers);
  for (int l = 0; l < cfg->num_layers && rc == SMI_OK; ++l) {
    const smi_text_decoder_layer& s = w->layers[l];
    DecLayer& L = D->layers[l];
    up(s.self_attn_layer_norm_w, d, false, L.ln1_w, "self_attn_layer_norm.weight");
    up(s.self_attn_layer_norm_b, d, false, L.ln1_b, "self_attn_layer_norm.bias");
    up(s.ffn_layer_norm_w, d, false, L.ln3_w, "ffn_layer_norm.weight");
    up(s.ffn_layer_norm_b, d, false, L.ln3_b, "ffn_layer_norm.bias");
    up(s.out_w, d * d, true, L.w_o, "self_attn.output_proj.weight");
    up(s.out_b, d, false, L.b_o, "self_attn.output_proj.bias");
    up(s.cross_v_w, d * ci, true, L.wc_v, "encoder_decoder_attn.v_proj.weight");  // [model_dim, input_dim]
    up(s.cross_v_b, d, false, L.bc_v, "encoder_decoder_attn.v_proj.bias");
    up(s.cross_out_w, d * d, true, L.wc_o, "encoder_decoder_attn.output_proj.weight");
    up(s.cross_out_b, d, false, L.bc_o, "encoder_decoder_attn.output_proj.bias");
    up(s.ffn_inner_w, f * d, true, L.w_1, "ffn.inner_proj.weight");
    up(s.ffn_inner_b, f, false, L.b_1, "ffn.inner_proj.bias");
    up(s.ffn_out_w, d * f, true, L.w_2, "ffn.output_proj.weight");
    up(s.ffn_out_b, d, false, L.b_2, "ffn.output_proj.bias");
    if (rc == SMI_OK && D->ffn_tile_major) {
      rc = to_tile_major(L.w_1, (int)f, (int)d);
      if (rc == SMI_OK) rc = to_tile_major(L.w_2, (int)d, (int)f);
    }
    if (rc == SMI_OK) {
      DevBuf tq, tk, tv, bq, bk, bv;
      up(s.q_w, d * d, true, tq, "self_attn.q_proj.weight");
      up(s.k_w, d * d, true, tk, "self_attn.k_proj.weight");
      up(s.v_w, d * d, true, tv, "self_attn.v_proj.weight");
      up(s.q_b, d, false, bq, "self_attn.q_proj.bias");
      up(s.k_b, d, false, bk, "self_attn.k_proj.bias");
      up(s.v_b, d, false, bv, "self_attn.v_proj.bias");
      if (rc == SMI_OK) {
        const size_t wes = flex ? 4 : 2;
        hipError_t he = L.w_qkv.alloc((size_t)3 * d * d * wes);
        if (he == hipSuccess) he = L.b_qkv.alloc((size_t)3 * d * 4);
        const size_t wb = (size_t)d * d * wes, bb = (size_t)d * 4;
        if (he == hipSuccess) he = hipMemcpy(L.w_qkv.p, tq.p, wb, hipMemcpyDeviceToDevice);
        if (he == hipSuccess) he = hipMemcpy((char*)L.w_qkv.p + wb, tk.p, wb, hipMemcpyDeviceToDevice);
        if (he == hipSuccess) he = hipMemcpy((char*)L.w_qkv.p + 2 * wb, tv.p, wb, hipMemcpyDeviceToDevice);
        if (he == hipSuccess) he = hipMemcpy(L.b_qkv.p, bq.p, bb, hipMemcpyDeviceToDevice);
        if (he == hipSuccess) he = hipMemcpy((char*)L.b_qkv.p + bb, bk.p, bb, hipMemcpyDeviceToDevice);
        if (he == hipSuccess) he = hipMemcpy((char*)L.b_qkv.p + 2 * bb, bv.p, bb, hipMemcpyDeviceToDevice);
        if (he != hipSuccess)
          rc = fail(he == hipErrorOutOfMemory ? SMI_ERR_OOM : SMI_ERR_HIP, "packing qkv: %s", hipGetErrorString(he));
      }
    }
  }
  if (rc != SMI_OK) {
    delete D;
    return rc;
  }
  D->weight_bytes = (int64_t)(D->embed.bytes + D->embed_tm.bytes + D->pos.bytes);
  for (auto& L : D->layers)
    D->weight_bytes += (int64_t)(L.w_qkv.bytes + L.w_o.bytes + L.wc_v.bytes + L.wc_o.bytes + L.w_1.bytes + L.w_2.bytes);
  *out = D;
  return SMI_OK;
}

void smi_text_decoder_destroy(smi_text_decoder* dec) {
  if (!dec) return;
  (void)hipDeviceSynchronize();
  delete dec;
}

int smi_text_decoder_logits(smi_text_decoder* D, const void* emb, int32_t emb_dtype, int32_t n,
                            const int64_t* prev_tokens, int32_t t, float* out_logits, void* stream_v) {
  if (!D || !emb || !prev_tokens || !out_logits) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (n <= 0 || t <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  if (t > D->cfg.max_seq_len) return fail(SMI_ERR_INVALID_ARG, "t=%d exceeds max_seq_len %d", t, D->cfg.max_seq_len);
  if (int rc = check_emb_dtype(emb_dtype)) return rc;
  hipStream_t stream = (hipStream_t)stream_v;
  DecWork& S = D->ws[0];
  S.chained = false;
  const int rows_pad = (int)round_up(n, 256), n_pad = rows_pad;
  if (int rc = ensure_step_workspace(D, S, rows_pad, t, stream)) return rc;
  HIP_TRY(S.tok.reserve((size_t)rows_pad * 4));
  // teacher forcing, one hypothesis per sentence: the ancestry is the identity and is never read
  // for j < pos only through anc[r][j] = r
  const int stride = D->cfg.max_seq_len + 1;
  HIP_TRY(S.anc[0].reserve((size_t)rows_pad * stride * 4));
  if (int rc = upload_identity_ancestry(S, n, stride, stream)) return rc;
  if (int rc = compute_cross_constants(D, S, emb, emb_dtype, n, n_pad, stream)) return rc;
  for (int pos = 0; pos < t; ++pos) {
    HIP_TRY(launch_gather_tokens(prev_tokens, t, pos, S.tok.as<int32_t>(), n, stream));
    if (int rc = decoder_step(D, S, n, rows_pad, 1, n_pad, pos, S.anc[0].as<int32_t>(), stride, stream)) return rc;
    HIP_TRY(hipMemcpy2DAsync(out_logits + (size_t)pos * D->cfg.vocab_size, (size_t)t * D->cfg.vocab_size * 4,
                             S.logits.p, (size_t)D->vocab_pad * 4, (size_t)D->cfg.vocab_size * 4, n,
                             hipMemcpyDeviceToDevice, stream));
  }
  return SMI_OK;
}

int smi_text_decoder_score(smi_text_decoder* D, const void* emb, int32_t emb_dtype, int32_t n, const int64_t* tokens,
                           int32_t t, const int32_t* lens, float* out_logprobs, void* stream_v) {
  if (!D || !emb || !tokens || !lens || !out_logprobs) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (n <= 0 || t <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  if (int rc = check_emb_dtype(emb_dtype)) return rc;
  const smi_text_decoder_config& c = D->cfg;
  if (t > c.max_seq_len + 1) return fail(SMI_ERR_INVALID_ARG, "t=%d exceeds max_seq_len + 1 = %d", t, c.max_seq_len + 1);
  int lmax = 1;
  for (int s = 0; s < n; ++s) {
    if (lens[s] < 1 || lens[s] > t) return fail(SMI_ERR_INVALID_ARG, "lens[%d] = %d outside [1, t = %d]", s, lens[s], t);
    lmax = std::max(lmax, (int)lens[s]);
  }
  hipStream_t stream = (hipStream_t)stream_v;
  if (t == 1) return SMI_OK;  // nothing to score
  HIP_TRY(hipMemsetAsync(out_logprobs, 0, (size_t)n * (t - 1) * 4, stream));
  if (lmax == 1) return SMI_OK;
  DecWork& S = D->ws[0];
  S.chained = false;
  // every sentence of the call gets the same seq = lmax - 1 input positions; groups of whole sentences bound the workspace
  const int seq = lmax - 1;
  const int per = std::max(1, std::min(n, kScoreRows / seq));
  std::vector<int32_t> cu((size_t)per + 1);  // the causal attention's sequence starts (every group: uniform seq rows)
  for (int s = 0; s <= per; ++s) cu[s] = s * seq;
  HIP_TRY(S.sc_lens.reserve((size_t)n * 4));
  HIP_TRY(S.sc_cu.reserve(cu.size() * 4));
  HIP_TRY(S.sc_bad.reserve(4));
  HIP_TRY(hipMemcpyAsync(S.sc_lens.p, lens, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(S.sc_cu.p, cu.data(), cu.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(S.sc_bad.p, 0, 4, stream));
  const size_t emb_row = emb_row_bytes(c, emb_dtype);
  for (int s0 = 0; s0 < n; s0 += per) {
    const int ns = std::min(per, n - s0);
    if (int rc = score_group(D, S, (const char*)emb + s0 * emb_row, emb_dtype, ns, tokens + (size_t)s0 * t, t,
                             S.sc_lens.as<int32_t>() + s0, seq, out_logprobs + (size_t)s0 * (t - 1), stream))
      return rc;
  }
  int32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, S.sc_bad.p, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (bad) return fail(SMI_ERR_INVALID_ARG, "a token id inside a sequence's length is outside [0, vocab %d)", (int)c.vocab_size);
  return SMI_OK;
}

}  // extern "C"

namespace {

// what the four generate / sample entries check alike (params: the beam-search / sampling parameter struct)
int check_decode_args(const smi_text_decoder* D, const void* emb, int emb_dtype, int n, bool have_prompts, const void* params,
                      const void* out_tokens, const void* out_lens, const void* out_scores) {
  if (!have_prompts || !D || !emb || !params || !out_tokens || !out_lens || !out_scores)
    return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (n <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  return check_emb_dtype(emb_dtype);
}

int check_beam_params(const smi_text_decoder* D, const smi_beam_search_params* bp) {
  const int beam = bp->beam_size;
  if (beam < 1 || beam > 8) return fail(SMI_ERR_UNSUPPORTED, "beam_size %d outside [1,8]", beam);
  if (2 * beam >= D->cfg.vocab_size) return fail(SMI_ERR_UNSUPPORTED, "vocabulary too small for beam %d", beam);
  if (!(bp->temperature > 0.f)) return fail(SMI_ERR_INVALID_ARG, "temperature must be positive");
  return SMI_OK;
}

// the checked call
int generate_run(smi_text_decoder* D, const void* emb, int emb_dtype, const PromptPlan& plan, const smi_beam_search_params* bp,
                 int32_t* out_tokens, int32_t* out_lens, float* out_scores, hipStream_t stream) {
  const int n = plan.n, beam = bp->beam_size;
  const int max_len = plan.width;  // the output row length
  HIP_TRY(D->margins.reserve((size_t)n * 2 * 4));
  D->margins_n = n;
  float* margins = D->margins.as<float>();

  // Independent chains.  Sentences do not interact, and at decode batch sizes a step is ~170
  // dependent launches of lone tiles: ~8.5 us of every launch is fixed cost (dispatch, pipeline fill, epilogue) and the
  // two FFN projections occupy 160 of 256 CUs.  Two or three sentence groups, each with its own workspace, KV cache,
  // beam state, stream and host thread, put their launch gaps and idle CUs under each other's K loops; the row-count
  // bound kernels (logits GEMM, single-query attention, slab folds) shrink with the group.  Beam bookkeeping is per
  // sentence, so the hypotheses are those of the single chain up to the fp32 summation order of the split-K slabs
  // (the number of K parts follows the group's row count).
  const int chains = decode_chains(D, n, beam);
  if (chains <= 1) {
    D->ws[0].chained = false;
    return generate_chain(D, D->ws[0], emb, emb_dtype, plan, bp, out_tokens, out_lens, out_scores, margins, stream);
  }
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (!D->fork_ev) HIP_TRY(hipEventCreateWithFlags(&D->fork_ev, hipEventDisableTiming));
  for (int g = 0; g < chains; ++g) {
    DecWork& S = D->ws[g];
    if (!S.stream) HIP_TRY(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    if (!S.done_ev) HIP_TRY(hipEventCreateWithFlags(&S.done_ev, hipEventDisableTiming));
  }
  // fork: every chain starts behind the work already queued on the caller's stream (the embeddings' producer)
  HIP_TRY(hipEventRecord(D->fork_ev, stream));
  const size_t emb_row = emb_row_bytes(D->cfg, emb_dtype);
  const int per = (n + chains - 1) / chains;
  int rcs[kMaxChains] = {};
  std::string errs[kMaxChains];
  std::thread workers[kMaxChains];
  for (int g = 0; g < chains; ++g) {
    const int s0 = g * per, ng = std::min(per, n - s0);
    if (ng <= 0) continue;
    workers[g] = std::thread([&, g, s0, ng] {
      DecWork& S = D->ws[g];
      S.chained = true;
      int rc = SMI_OK;
      hipError_t he = hipSetDevice(dev);
      if (he == hipSuccess) he = hipStreamWaitEvent(S.stream, D->fork_ev, 0);
      if (he != hipSuccess) rc = fail(SMI_ERR_HIP, "chain %d set-up: %s", g, hipGetErrorString(he));
      if (rc == SMI_OK) {
        // (per-sentence prompts: the table is sliced per sentence group)
        rc = generate_chain(D, S, (const char*)emb + (size_t)s0 * emb_row, emb_dtype, plan.group(s0, ng), bp,
                            out_tokens + (size_t)s0 * beam * max_len, out_lens + (size_t)s0 * beam,
                            out_scores + (size_t)s0 * beam, margins + 2 * (size_t)s0, S.stream);
      }
      if (rc == SMI_OK && (he = hipEventRecord(S.done_ev, S.stream)) != hipSuccess)
        rc = fail(SMI_ERR_HIP, "chain %d: %s", g, hipGetErrorString(he));
      rcs[g] = rc;
      if (rc != SMI_OK) errs[g] = last_error();  // thread-local: hand the text to the calling thread
    });
  }
  for (int g = 0; g < chains; ++g)
    if (workers[g].joinable()) workers[g].join();
  for (int g = 0; g < chains; ++g)
    if (rcs[g] != SMI_OK) {
      for (int h = 0; h < chains; ++h)
        if (D->ws[h].stream) (void)hipStreamSynchronize(D->ws[h].stream);
      return fail(rcs[g], "%s", errs[g].c_str());
    }
  // join: the caller's stream continues behind every chain
  for (int g = 0; g < chains; ++g)
    if (g * per < n)
      HIP_TRY(hipStreamWaitEvent(stream, D->ws[g].done_ev, 0));
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_text_decoder_generate(smi_text_decoder* D, const void* emb, int32_t emb_dtype, int32_t n,
                              const int64_t* prompt, int32_t prompt_len, const smi_beam_search_params* bp,
                              int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream_v) {
  if (int rc = check_decode_args(D, emb, emb_dtype, n, prompt != nullptr, bp, out_tokens, out_lens, out_scores)) return rc;
  if (int rc = check_beam_params(D, bp)) return rc;
  PromptPlan plan;
  if (int rc = plan_one_prompt(D->cfg, n, prompt, prompt_len, bp->max_seq_len, bp->min_seq_len, &plan)) return rc;
  return generate_run(D, emb, emb_dtype, plan, bp, out_tokens, out_lens, out_scores, (hipStream_t)stream_v);
}

int smi_text_decoder_generate_prompts(smi_text_decoder* D, const void* emb, int32_t emb_dtype, int32_t n,
                                      const int64_t* prompts, int32_t prompt_stride, const int32_t* prompt_lens,
                                      int32_t gen_cap, int32_t min_gen_len, const smi_beam_search_params* bp,
                                      int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream_v) {
  if (int rc = check_decode_args(D, emb, emb_dtype, n, prompts && prompt_lens, bp, out_tokens, out_lens, out_scores)) return rc;
  if (int rc = check_beam_params(D, bp)) return rc;
  hipStream_t stream = (hipStream_t)stream_v;
  PromptPlan plan;
  if (int rc = plan_prompts(D, n, prompts, prompt_stride, prompt_lens, gen_cap, min_gen_len, bp->max_seq_len, stream, &plan))
    return rc;
  return generate_run(D, emb, emb_dtype, plan, bp, out_tokens, out_lens, out_scores, stream);
}

int smi_text_decoder_set_chains(smi_text_decoder* D, int32_t chains) {
  if (!D) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (chains < 0 || chains > kMaxChains) return fail(SMI_ERR_INVALID_ARG, "chains %d outside [0, %d]", chains, kMaxChains);
  D->chains = chains;
  return SMI_OK;
}

int smi_text_decoder_set_beam_logits_dtype(smi_text_decoder* D, int32_t dtype) {
  if (!D) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (dtype != SMI_F16 && dtype != SMI_F32) return fail(SMI_ERR_INVALID_ARG, "dtype %d: SMI_F16 or SMI_F32", dtype);
  D->beam_logits_f16 = dtype == SMI_F16;
  return SMI_OK;
}

int smi_text_decoder_set_slab_dtype(smi_text_decoder* D, int32_t dtype) {
  if (!D) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (dtype != SMI_F16 && dtype != SMI_F32) return fail(SMI_ERR_INVALID_ARG, "dtype %d: SMI_F16 or SMI_F32", dtype);
  D->beam_slab_f16 = dtype == SMI_F16;
  return SMI_OK;
}

int smi_text_decoder_last_margins(smi_text_decoder* D, float* out_margins, int32_t n, void* stream_v) {
  if (!D || !out_margins) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (n <= 0 || n != D->margins_n || !D->margins.p)
    return fail(SMI_ERR_INVALID_ARG, "n=%d does not match the last generate() call (%d sentences)", n, D->margins_n);
  HIP_TRY(hipMemcpyAsync(out_margins, D->margins.p, (size_t)n * 2 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream_v));
  return SMI_OK;
}

}  // extern "C"

namespace {

int check_sampler(int sampler, int top_k, float top_p) {
  if (sampler == SMI_SAMPLER_TOP_K) {
    if (top_k < 1) return fail(SMI_ERR_INVALID_ARG, "top_k must be >= 1");
  } else if (sampler == SMI_SAMPLER_TOP_P) {
    if (!(top_p > 0.f && top_p <= 1.f)) return fail(SMI_ERR_INVALID_ARG, "top_p must be in (0, 1]");
  } else {
    return fail(SMI_ERR_INVALID_ARG, "unknown sampler %d", sampler);
  }
  return SMI_OK;
}

int check_sampling_params(const smi_text_decoder* D, const smi_sampling_params* sp) {
  if (int rc = check_sampler(sp->sampler, sp->top_k, sp->top_p)) return rc;
  if (D->cfg.vocab_size > (1 << 18))
    return fail(SMI_ERR_UNSUPPORTED, "vocab %d: sampling covers up to 2^18 tokens", (int)D->cfg.vocab_size);
  if (!(sp->temperature > 0.f)) return fail(SMI_ERR_INVALID_ARG, "temperature must be positive");
  return SMI_OK;
}

// the checked call (sp->max_seq_len / min_seq_len are not read here: the plan carries the length limits)
int sample_run(smi_text_decoder* D, const void* emb, int emb_dtype, const PromptPlan& plan, const smi_sampling_params* sp,
               int32_t* out_tokens, int32_t* out_lens, float* out_scores, hipStream_t stream) {
  const smi_text_decoder_config& c = D->cfg;
  const int n = plan.n;
  const int max_len = plan.width;  // loop bound and output row length (one sentence group: the longest cap)
  // one hypothesis per sentence (fairseq2 num_gens = 1): rows = sentences, identity ancestry
  DecWork& S = D->ws[0];
  S.chained = false;
  const int rows_pad = (int)round_up(n, 256), n_pad = rows_pad;
  const int stride = c.max_seq_len + 1;
  if (int rc = ensure_step_workspace(D, S, rows_pad, std::min(max_len, kKvInitialPositions), stream)) return rc;
  HIP_TRY(S.tok.reserve((size_t)rows_pad * 4));
  HIP_TRY(S.cum.reserve((size_t)n * 4));
  HIP_TRY(S.done.reserve((size_t)n * 4));
  HIP_TRY(S.ndone.reserve(4));
  HIP_TRY(S.new_tok.reserve((size_t)n * 4));
  HIP_TRY(S.new_cum.reserve((size_t)n * 4));
  HIP_TRY(S.anc[0].reserve((size_t)rows_pad * stride * 4));
  {
    std::vector<int32_t> first((size_t)n);
    for (int r = 0; r < n; ++r) first[r] = (int32_t)plan.tok[(size_t)r * plan.stride];
    HIP_TRY(hipMemcpyAsync(S.tok.p, first.data(), first.size() * 4, hipMemcpyHostToDevice, stream));
    if (int rc = upload_identity_ancestry(S, n, stride, stream)) return rc;  // finishes both copies
  }
  const StepProcDev proc = D->sp.dev;
  const int prompt_len = plan.scalar_prompt_len();
  if (proc.active() && plan.one_prompt()) {  // the bans read the prompt on the device (per-sentence prompts: from the table)
    std::vector<int32_t> p32(plan.tok, plan.tok + prompt_len);
    HIP_TRY(S.prompt_dev.reserve((size_t)prompt_len * 4));
    HIP_TRY(hipMemcpyAsync(S.prompt_dev.p, p32.data(), p32.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  HIP_TRY(hipMemsetAsync(S.cum.p, 0, (size_t)n * 4, stream));
  HIP_TRY(hipMemsetAsync(S.done.p, 0, (size_t)n * 4, stream));
  HIP_TRY(hipMemsetAsync(S.ndone.p, 0, 4, stream));
  HIP_TRY(hipMemsetAsync(out_tokens, 0xff, (size_t)n * max_len * 4, stream));
  HIP_TRY(hipMemsetAsync(out_lens, 0, (size_t)n * 4, stream));
  HIP_TRY(hipMemsetAsync(out_scores, 0, (size_t)n * 4, stream));
  if (int rc = compute_cross_constants(D, S, emb, emb_dtype, n, n_pad, stream)) return rc;

  for (int pos = 0; pos + 1 < max_len; ++pos) {
    const int step_nr = pos + 1;
    if (pos >= S.kv_positions)
      if (int rc = grow_kv(D, S, rows_pad, std::min(max_len, 2 * S.kv_positions), stream)) return rc;
    if (int rc = decoder_step(D, S, n, rows_pad, 1, n_pad, pos, S.anc[0].as<int32_t>(), stride, stream)) return rc;
    // the sentences' prompt tokens differ: a forced step reads the table too
    const StepMode mode = step_mode(plan, step_nr);
    const bool mixed = mode.kind == StepMode::kMixed || (mode.kind == StepMode::kForced && mode.forced_tok < 0);
    SampleRowsArgs a{};
    a.logits = S.logits.as<float>(); a.ld = D->vocab_pad; a.rows = n; a.vocab = (int)c.vocab_size;
    a.inv_temp = 1.0f / sp->temperature; a.pad_idx = c.pad_idx; a.eos_idx = c.eos_idx;
    a.block_eos = mode.block_eos;
    a.unk_idx = c.unk_idx; a.unk_penalty = sp->unk_penalty;
    a.forced_tok = mode.kind == StepMode::kForceEos ? c.eos_idx : mode.forced_tok;
    a.mode = sp->sampler; a.top_k = sp->top_k; a.top_p = sp->top_p; a.z = nullptr; a.seed = sp->seed; a.step = step_nr;
    a.done = S.done.as<int32_t>(); a.out_tok = S.new_tok.as<int32_t>(); a.out_logp = S.new_cum.as<float>();
    if (a.forced_tok < 0 && proc.active()) {
      a.proc = proc; a.prompt = S.prompt_dev.as<int32_t>(); a.prompt_len = prompt_len; a.gen = out_tokens; a.gen_stride = max_len;
    }
    // (a free step of every sentence under step processors: the bans still read each row's own prompt)
    if (mixed || (!plan.one_prompt() && a.forced_tok < 0 && proc.active())) a.table = plan.dev;
    HIP_TRY(launch_sample_rows(a, stream));
    SampleUpdateArgs u{};
    u.samp_tok = S.new_tok.as<int32_t>(); u.samp_logp = S.new_cum.as<float>(); u.tok = S.tok.as<int32_t>();
    u.cum = S.cum.as<float>(); u.done = S.done.as<int32_t>(); u.ndone = S.ndone.as<int32_t>();
    u.out_tokens = out_tokens; u.out_lens = out_lens; u.out_scores = out_scores; u.n = n; u.out_stride = max_len;
    u.pos = pos; u.prompt_len = prompt_len; u.eos_idx = c.eos_idx; u.normalize = sp->normalize_scores;
    u.len_penalty = sp->len_penalty; u.prompt_lens = plan.dev.len;
    HIP_TRY(launch_sample_update(u, stream));
    if ((step_nr & 7) == 0 && mode.kind != StepMode::kForceEos) {  // (after a forced EOS everything is done anyway)
      bool done = false;
      if (int rc = all_sentences_done(S, n, stream, &done)) return rc;
      if (done) break;
    }
  }
  if (proc.active())
    if (int rc = record_table_use(S, stream)) return rc;
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_text_decoder_sample(smi_text_decoder* D, const void* emb, int32_t emb_dtype, int32_t n,
                            const int64_t* prompt, int32_t prompt_len, const smi_sampling_params* sp,
                            int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream_v) {
  if (int rc = check_decode_args(D, emb, emb_dtype, n, prompt != nullptr, sp, out_tokens, out_lens, out_scores)) return rc;
  if (int rc = check_sampling_params(D, sp)) return rc;
  PromptPlan plan;
  if (int rc = plan_one_prompt(D->cfg, n, prompt, prompt_len, sp->max_seq_len, sp->min_seq_len, &plan)) return rc;
  return sample_run(D, emb, emb_dtype, plan, sp, out_tokens, out_lens, out_scores, (hipStream_t)stream_v);
}

int smi_text_decoder_sample_prompts(smi_text_decoder* D, const void* emb, int32_t emb_dtype, int32_t n,
                                    const int64_t* prompts, int32_t prompt_stride, const int32_t* prompt_lens,
                                    int32_t gen_cap, int32_t min_gen_len, const smi_sampling_params* sp,
                                    int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream_v) {
  if (int rc = check_decode_args(D, emb, emb_dtype, n, prompts && prompt_lens, sp, out_tokens, out_lens, out_scores)) return rc;
  if (int rc = check_sampling_params(D, sp)) return rc;
  hipStream_t stream = (hipStream_t)stream_v;
  PromptPlan plan;
  if (int rc = plan_prompts(D, n, prompts, prompt_stride, prompt_lens, gen_cap, min_gen_len, sp->max_seq_len, stream, &plan))
    return rc;
  return sample_run(D, emb, emb_dtype, plan, sp, out_tokens, out_lens, out_scores, stream);
}

}  // extern "C"

namespace {
// smi_step_processors -> checked host CSR (SMI_OK) or an error
int check_step_processors(const smi_step_processors* p, int64_t vocab, int max_seq_len) {
  if (p->ngram_size < 0 || p->ngram_size > max_seq_len)
    return fail(SMI_ERR_INVALID_ARG, "ngram_size %d outside [0, max_seq_len %d]", p->ngram_size, max_seq_len);
  if (p->num_banned < 0 || p->num_banned > kStepProcMaxBanned)
    return fail(SMI_ERR_INVALID_ARG, "num_banned %d outside [0, %d]", p->num_banned, kStepProcMaxBanned);
  if (p->num_banned == 0) return SMI_OK;
  if (!p->banned_tokens || !p->banned_offsets) return fail(SMI_ERR_INVALID_ARG, "null banned_tokens / banned_offsets");
  if (p->banned_offsets[0] != 0) return fail(SMI_ERR_INVALID_ARG, "banned_offsets[0] must be 0");
  for (int q = 0; q < p->num_banned; ++q) {
    const int len = p->banned_offsets[q + 1] - p->banned_offsets[q];
    if (len < 1) return fail(SMI_ERR_INVALID_ARG, "banned sequence %d is empty", q);
    if (len > max_seq_len) return fail(SMI_ERR_INVALID_ARG, "banned sequence %d is longer than max_seq_len %d", q, max_seq_len);
  }
  for (int i = 0; i < p->banned_offsets[p->num_banned]; ++i)
    if (p->banned_tokens[i] < 0 || p->banned_tokens[i] >= vocab)
      return fail(SMI_ERR_INVALID_ARG, "banned token %d outside the vocabulary [0, %lld)", p->banned_tokens[i], (long long)vocab);
  return SMI_OK;
}

int upload_i32(DevBuf& dst, const int32_t* src, size_t count) {
  HIP_TRY(dst.reserve(count * 4));
  HIP_TRY(hipMemcpy(dst.p, src, count * 4, hipMemcpyHostToDevice));
  return SMI_OK;
}

// checked processors -> the device table (uploaded on return)
int upload_step_processors(const smi_step_processors* p, StepProcTable* st) {
  if (p->num_banned > 0) {
    if (int rc = upload_i32(st->off, p->banned_offsets, (size_t)p->num_banned + 1)) return rc;
    if (int rc = upload_i32(st->tok, p->banned_tokens, (size_t)p->banned_offsets[p->num_banned])) return rc;
  }
  st->dev = StepProcDev{p->ngram_size, p->num_banned, st->tok.as<int32_t>(), st->off.as<int32_t>()};
  return SMI_OK;
}
}  // namespace

extern "C" {

int smi_text_decoder_set_step_processors(smi_text_decoder* D, const smi_step_processors* procs) {
  if (!D) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (!procs || (procs->ngram_size == 0 && procs->num_banned == 0)) {
    D->sp.dev.ngram = D->sp.dev.num_banned = 0;
    return SMI_OK;
  }
  if (D->cfg.max_seq_len >= kStepProcMaxLen)
    return fail(SMI_ERR_UNSUPPORTED, "step processors cover max_seq_len up to %d", kStepProcMaxLen - 1);
  if (int rc = check_step_processors(procs, D->cfg.vocab_size, D->cfg.max_seq_len)) return rc;
  // stage the new table in buffers of its own: a failed upload leaves the handle's setting as it was
  StepProcTable st;
  if (int rc = upload_step_processors(procs, &st)) return rc;
  // the handle's earlier calls may still read the old table: wait for them (not for the rest of the device)
  for (auto& w : D->ws)
    if (w.sp_ev) HIP_TRY(hipEventSynchronize(w.sp_ev));
  D->sp = std::move(st);
  return SMI_OK;
}

int smi_vocab_select_banned(const void* logits, int32_t ldl, int32_t logits_f16_tm, int32_t rows, int32_t vocab,
                            const float* tile_max, const float* tile_sum, int32_t k2, int32_t pad_idx,
                            const int32_t* hist, int32_t hist_stride, int32_t hist_len, const smi_step_processors* procs,
                            float* pval, int32_t* pidx, float* pmax, float* psum, void* stream) {
  if (!logits || !tile_max || !tile_sum || !hist || !procs || !pval || !pidx || !pmax || !psum)
    return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (rows <= 0 || vocab <= 0 || ldl % 256 || ldl < vocab || ldl / 256 > 2048)
    return fail(SMI_ERR_INVALID_ARG, "ldl %d must be a multiple of 256 >= vocab %d, at most 2048 tiles", ldl, vocab);
  if (k2 < 1 || k2 > kVocabScanK2Max) return fail(SMI_ERR_INVALID_ARG, "k2 %d outside [1, %d]", k2, kVocabScanK2Max);
  if (hist_len < 1 || hist_len > kStepProcMaxLen - 1 || hist_stride < hist_len)
    return fail(SMI_ERR_INVALID_ARG, "hist_len %d outside [1, %d] or above hist_stride %d", hist_len, kStepProcMaxLen - 1,
                hist_stride);
  if (logits_f16_tm && rows % 256) return fail(SMI_ERR_INVALID_ARG, "tile-major logits need rows padded to 256");
  if (int rc = check_special_ids(pad_idx, -1, -1, vocab, false)) return rc;
  if (int rc = check_step_processors(procs, vocab, kStepProcMaxLen - 1)) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  StepProcTable st;
  if (int rc = upload_step_processors(procs, &st)) return rc;
  // (no processor in `procs`: the launcher runs the engine's default selection, as generate() does)
  VocabSelectArgs v{};
  v.logits = (const float*)logits; v.ldl = ldl; v.f16_tm = logits_f16_tm; v.rows = rows; v.vocab = vocab;
  v.tile_max = tile_max; v.tile_sum = tile_sum; v.ntiles = ldl / 256; v.stat_rows = rows;
  v.k2 = k2; v.inv_temp = 1.0f; v.pad_idx = pad_idx; v.eos_idx = -1; v.unk_idx = -1;
  v.pmax = pmax; v.psum = psum; v.pval = pval; v.pidx = pidx;
  v.hist = hist; v.hist_stride = hist_stride; v.hist_len = hist_len; v.proc = st.dev;
  HIP_TRY(launch_vocab_select(v, (hipStream_t)stream));
  // the CSR copies are freed on return: finish with them first
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return SMI_OK;
}

// ---- the beam search's state kernels on caller-owned arrays (tests/test_gpu_beam_kernels.py): the launchers of generate_chain
namespace {
PromptTableDev table_dev(const smi_prompt_table& t) { return PromptTableDev{t.tok, t.len, t.stride, t.gen_cap, t.min_gen, t.model_max}; }
int check_prompt_table(const smi_prompt_table& t) {
  if (!t.tok) return SMI_OK;
  if (!t.len) return fail(SMI_ERR_INVALID_ARG, "prompt table without lengths");
  if (t.stride < 1 || t.gen_cap < 1 || t.min_gen < 0 || t.model_max < 2)
    return fail(SMI_ERR_INVALID_ARG, "prompt table: stride=%d gen_cap=%d min_gen=%d model_max=%d", t.stride, t.gen_cap, t.min_gen,
                t.model_max);
  return SMI_OK;
}
int check_beam_state(const smi_beam_state* st) {
  if (!st) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (!st->tok || !st->cum || !st->nactive || !st->done || !st->ndone || !st->parent || !st->new_tok || !st->new_cum || !st->fin_tok ||
      !st->fin_len || !st->fin_score || !st->fin_count || !st->anc[0] || !st->anc[1] || !st->hist[0] || !st->hist[1])
    return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (st->n < 1 || st->beam < 1 || st->beam > 8 || st->stride < 2 || (int64_t)st->n * st->beam > (1 << 24))
    return fail(SMI_ERR_INVALID_ARG, "n=%d beam=%d (1..8) stride=%d", st->n, st->beam, st->stride);
  return SMI_OK;
}
// (a tile-major buffer holds (rows + 255) / 256 * 256 rows: the caller's allocation, as in generate_chain)
int check_logits_shape(int ldl, int64_t rows, int vocab) {
  if (rows <= 0 || vocab <= 0 || ldl % 256 || ldl < vocab || ldl / 256 > 2048)
    return fail(SMI_ERR_INVALID_ARG, "ldl %d must be a multiple of 256 >= vocab %d, at most 2048 tiles", ldl, vocab);
  return SMI_OK;
}
}  // namespace

int smi_vocab_select(const smi_vocab_select_args* a, void* stream) {
  if (!a || !a->logits || !a->tile_max || !a->tile_sum || !a->pmax || !a->psum || !a->pval || !a->pidx)
    return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (int rc = check_logits_shape(a->ldl, a->rows, a->vocab)) return rc;
  if (a->stat_rows < a->rows) return fail(SMI_ERR_INVALID_ARG, "stat_rows %d below rows %d", a->stat_rows, a->rows);
  if (a->k2 < 0 || a->k2 > kVocabScanK2Max) return fail(SMI_ERR_INVALID_ARG, "k2 %d outside [0, %d]", a->k2, kVocabScanK2Max);
  if (!(a->inv_temp > 0.f) || !std::isfinite(a->inv_temp) || !std::isfinite(a->unk_penalty))
    return fail(SMI_ERR_INVALID_ARG, "inv_temp must be positive and finite, unk_penalty finite");
  if (int rc = check_special_ids(a->pad_idx, a->eos_idx, a->unk_idx, a->vocab, false)) return rc;
  if (int rc = check_prompt_table(a->table)) return rc;
  if (a->table.tok && (a->group < 1 || a->step_nr < 1 || a->rows % a->group))
    return fail(SMI_ERR_INVALID_ARG, "prompt table: group=%d must divide rows=%d, step_nr=%d >= 1", a->group, a->rows, a->step_nr);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  VocabSelectArgs v{};
  v.logits = (const float*)a->logits; v.ldl = a->ldl; v.f16_tm = a->logits_f16_tm ? 1 : 0; v.rows = a->rows; v.vocab = a->vocab;
  v.tile_max = a->tile_max; v.tile_sum = a->tile_sum; v.ntiles = a->ldl / 256; v.stat_rows = a->stat_rows;
  v.k2 = a->k2; v.inv_temp = a->inv_temp; v.pad_idx = a->pad_idx; v.eos_idx = a->eos_idx; v.unk_idx = a->unk_idx;
  v.unk_penalty = a->unk_penalty; v.block_eos = a->block_eos ? 1 : 0;
  v.pmax = a->pmax; v.psum = a->psum; v.pval = a->pval; v.pidx = a->pidx;
  if (a->table.tok) v.table = table_dev(a->table);
  v.group = a->group; v.step_nr = a->step_nr;
  HIP_TRY(launch_vocab_select(v, (hipStream_t)stream));
  return SMI_OK;
}

int smi_beam_init(const smi_beam_state* st, int32_t first_tok, const int32_t* first_toks, int32_t first_stride, void* stream) {
  if (int rc = check_beam_state(st)) return rc;
  if (first_toks ? first_stride < 1 : first_tok < 0)
    return fail(SMI_ERR_INVALID_ARG, "first_tok=%d first_stride=%d", first_tok, first_stride);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(launch_beam_init(st->tok, st->cum, st->nactive, st->done, st->ndone, st->fin_count, st->hist[0], st->anc[0], st->margins,
                           st->n * st->beam, st->n, st->stride, first_tok, (hipStream_t)stream, first_toks, first_stride, st->beam));
  return SMI_OK;
}

int smi_beam_step(const smi_beam_state* st, const smi_beam_step_args* a, void* stream) {
  if (int rc = check_beam_state(st)) return rc;
  if (!a || !a->logits || !a->pmax || !a->psum || !a->pval || !a->pidx) return fail(SMI_ERR_INVALID_ARG, "null argument");
  const int64_t rows = (int64_t)st->n * st->beam;
  if (int rc = check_logits_shape(a->ldl, rows, a->vocab)) return rc;
  if (a->k2 != 2 * st->beam) return fail(SMI_ERR_INVALID_ARG, "k2=%d must be 2 * beam=%d", a->k2, st->beam);
  if (a->pos < 0 || a->pos + 2 > st->stride) return fail(SMI_ERR_INVALID_ARG, "pos=%d needs stride=%d >= pos + 2", a->pos, st->stride);
  if (!(a->inv_temp > 0.f) || !std::isfinite(a->inv_temp) || !std::isfinite(a->len_penalty))
    return fail(SMI_ERR_INVALID_ARG, "inv_temp must be positive and finite, len_penalty finite");
  if (a->eos_idx < 0 || a->eos_idx >= a->vocab) return fail(SMI_ERR_INVALID_ARG, "eos_idx=%d outside the vocabulary", a->eos_idx);
  if (int rc = check_prompt_table(a->table)) return rc;
  if (!a->table.tok) {
    if (a->prompt_len < 1 || a->max_len < 2) return fail(SMI_ERR_INVALID_ARG, "prompt_len=%d max_len=%d", a->prompt_len, a->max_len);
    if (a->pos + 1 < a->prompt_len && (a->forced_tok < 0 || a->forced_tok >= a->vocab))
      return fail(SMI_ERR_INVALID_ARG, "forced_tok=%d outside the vocabulary", a->forced_tok);
    if (a->pos + 1 > a->max_len - 1) return fail(SMI_ERR_INVALID_ARG, "pos=%d is past the forced EOS of max_len=%d", a->pos, a->max_len);
  }
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  const int cur = a->pos & 1;
  BeamStepArgs b{};
  b.tok = st->tok; b.cum = st->cum; b.nactive = st->nactive; b.done = st->done; b.ndone = st->ndone;
  b.parent = st->parent; b.new_tok = st->new_tok; b.new_cum = st->new_cum;
  b.hist = st->hist[cur]; b.fin_tok = st->fin_tok; b.fin_len = st->fin_len; b.fin_score = st->fin_score; b.fin_count = st->fin_count;
  b.margins = st->margins;
  b.logits = (const float*)a->logits; b.ldl = a->ldl; b.logits_f16_tm = a->logits_f16_tm ? 1 : 0;
  b.pmax = a->pmax; b.psum = a->psum; b.pval = a->pval; b.pidx = a->pidx;
  b.n = st->n; b.beam = st->beam; b.k2 = a->k2; b.pos = a->pos; b.prompt_len = a->prompt_len; b.forced_tok = a->forced_tok;
  b.max_len = a->max_len; b.inv_temp = a->inv_temp; b.len_penalty = a->len_penalty; b.normalize = a->normalize ? 1 : 0;
  b.eos_idx = a->eos_idx; b.hist_stride = st->stride;
  if (a->table.tok) b.table = table_dev(a->table);
  HIP_TRY(launch_beam_step(b, (hipStream_t)stream));
  return SMI_OK;
}

int smi_beam_reorder(const smi_beam_state* st, int32_t pos, void* stream) {
  if (int rc = check_beam_state(st)) return rc;
  if (pos < 0 || pos + 2 > st->stride) return fail(SMI_ERR_INVALID_ARG, "pos=%d needs stride=%d >= pos + 2", pos, st->stride);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  const int cur = pos & 1;
  HIP_TRY(launch_beam_reorder(st->parent, st->new_tok, st->new_cum, st->anc[cur], st->anc[cur ^ 1], st->hist[cur], st->hist[cur ^ 1],
                              st->tok, st->cum, st->n * st->beam, st->stride, pos, (hipStream_t)stream));
  return SMI_OK;
}

int smi_beam_output(const smi_beam_state* st, int32_t out_stride, int32_t* out_tok, int32_t* out_len, float* out_score, void* stream) {
  if (int rc = check_beam_state(st)) return rc;
  if (!out_tok || !out_len || !out_score) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (out_stride < 1) return fail(SMI_ERR_INVALID_ARG, "out_stride=%d", out_stride);
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(launch_beam_output(st->fin_tok, st->fin_len, st->fin_score, st->fin_count, st->n, st->beam, st->stride, out_stride, out_tok,
                             out_len, out_score, st->margins, (hipStream_t)stream));
  return SMI_OK;
}

int smi_sample_rows_banned(const float* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t sampler, int32_t top_k,
                           float top_p, float temperature, int32_t pad_idx, int32_t eos_idx, int32_t block_eos,
                           int32_t unk_idx, float unk_penalty, const int32_t* hist, int32_t hist_len,
                           const smi_step_processors* procs, const uint64_t* z, int32_t* out_token, float* out_logprob,
                           uint64_t* out_kept_mass, int32_t* out_kept_count, void* stream) {
  if (!logits || !hist || !procs || !z || !out_token || !out_logprob) return fail(SMI_ERR_INVALID_ARG, "null argument");
  if (rows <= 0 || vocab <= 0) return fail(SMI_ERR_INVALID_ARG, "empty input");
  if (vocab > (1 << 18)) return fail(SMI_ERR_UNSUPPORTED, "vocab %d: sampling covers up to 2^18 tokens", vocab);
  if (ld % 4 || ld < (vocab + 3) / 4 * 4) return fail(SMI_ERR_INVALID_ARG, "ld %lld must be a multiple of 4 >= vocab", (long long)ld);
  if (!(temperature > 0.f)) return fail(SMI_ERR_INVALID_ARG, "temperature must be positive");
  if (int rc = check_sampler(sampler, top_k, top_p)) return rc;
  if (hist_len < 1 || hist_len > kStepProcMaxLen - 1) return fail(SMI_ERR_INVALID_ARG, "hist_len %d outside [1, %d]", hist_len, kStepProcMaxLen - 1);
  if (int rc = check_step_processors(procs, vocab, kStepProcMaxLen - 1)) return rc;
  if (!have_device()) return fail(SMI_ERR_NO_DEVICE, "no HIP device visible");
  StepProcTable st;
  if (int rc = upload_step_processors(procs, &st)) return rc;
  SampleRowsArgs a{};
  a.logits = logits; a.ld = ld; a.rows = rows; a.vocab = vocab; a.inv_temp = 1.0f / temperature;
  a.pad_idx = pad_idx; a.eos_idx = eos_idx; a.block_eos = block_eos; a.forced_tok = -1;
  a.unk_idx = unk_idx; a.unk_penalty = unk_penalty;
  a.mode = sampler; a.top_k = top_k; a.top_p = top_p; a.z = (const unsigned long long*)z;
  a.out_tok = out_token; a.out_logp = out_logprob; a.out_kept_mass = (unsigned long long*)out_kept_mass;
  a.out_kept_count = out_kept_count;
  // every row's sequence so far is hist[0 .. hist_len): a prompt with nothing generated yet
  a.proc = st.dev;
  a.prompt = hist; a.prompt_len = hist_len; a.gen = hist; a.gen_stride = 0; a.step = hist_len;
  HIP_TRY(launch_sample_rows(a, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the CSR copies are freed on return
  return SMI_OK;
}

}  // extern "C"
