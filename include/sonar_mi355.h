/*
 * sonar_mi355.h -- C ABI of the MI355X-native SONAR inference hot path.
 *
 * The reference (facebookresearch/SONAR v0.4.0) has no native code and no FFI:
 * its hot path is `model(batch)` inside the Python pipelines.  The entry points
 * below are what a binding for that path attaches to; each one cites the
 * reference interface it stands in for (paths relative to the reference repo).
 * INTEGRATION.md shows the ctypes stub a SONAR maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types cross this boundary;
 *  - every call returns SMI_OK (0) or a negative smi_status; smi_last_error()
 *    returns a thread-local human readable message for the last failure;
 *  - device buffers passed in are borrowed for the duration of the call (it is
 *    stream-ordered: the call enqueues work on `stream` and returns);
 *  - the engine owns its packed weights and workspace; the caller may free its
 *    own weight buffers as soon as *_create returns;
 *  - a handle is not re-entrant: use one handle per device and per thread;
 *  - nothing here falls back to the CPU: without a HIP device every compute
 *    entry point fails with SMI_ERR_NO_DEVICE.
 */
#ifndef SONAR_MI355_H
#define SONAR_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum smi_status {
  SMI_OK = 0,
  SMI_ERR_INVALID_ARG = -1,
  SMI_ERR_UNSUPPORTED = -2, /* shape/config outside what the kernels cover */
  SMI_ERR_NO_DEVICE = -3,
  SMI_ERR_OOM = -4,
  SMI_ERR_HIP = -5 /* a HIP runtime call failed; see smi_last_error() */
} smi_status;

/* SMI_BF16 exists at the BOUNDARY only (smi_cast): the engines take and return fp32 / fp16 tensors and compute with
 * fp16 operands and fp32 accumulation whatever a model's nominal dtype is.  A bf16 model (the reference's pipelines
 * accept any dtype, sonar/inference_pipelines/text.py:36-54,161-162) is served by casting: its weights are exactly
 * representable in fp16 over the normal range, its outputs are rounded to bf16 once, on the way out. */
typedef enum smi_dtype { SMI_F32 = 0, SMI_F16 = 1, SMI_BF16 = 2 } smi_dtype;
/* SMI_POOL_ATTENTION: the trainable pooler of sonar/nn/encoder_pooler.py:49-95 (factory.py:155-226) */
typedef enum smi_pooling { SMI_POOL_MEAN = 0, SMI_POOL_MAX = 1, SMI_POOL_LAST = 2, SMI_POOL_ATTENTION = 3 } smi_pooling;

/* A dense tensor handed to the engine at create time.  `data` may live in host
 * or device memory (`on_device`); fp32 or fp16. */
typedef struct smi_tensor {
  const void* data;
  int32_t dtype;     /* smi_dtype */
  int32_t on_device; /* 0 host, 1 device (current HIP device) */
  int64_t numel;
} smi_tensor;

/* Mirrors SonarTextEncoderConfig (sonar/models/sonar_text/config.py:14-85) for
 * the fields that affect the forward pass of the `basic`/`small` archs. */
typedef struct smi_text_encoder_config {
  int32_t model_dim;     /* 1024 (see "Shapes" below) */
  int32_t num_layers;    /* 24 */
  int32_t num_heads;     /* 16 */
  int32_t ffn_inner_dim; /* 8192; multiple of 128 */
  int64_t vocab_size;    /* 256206 */
  int32_t max_seq_len;   /* 514 = 512 + pad_idx + 1 (factory.py:56-59) */
  int32_t pos_offset;    /* 2 = pad_idx + 1 (_legacy_pad_idx, factory.py:88-92) */
  float embed_scale;     /* sqrt(model_dim), or 1 if no_scale_embedding */
  float ln_eps;          /* 1e-5 */
  int32_t pooling;       /* smi_pooling (config.py: pooling="mean") */
  int32_t flags;         /* SMI_ENC_* */
  /* Attention pooling (all 0 for the released models): width of the sentence vector (config.py `embedding_dim`,
   * 0 = model_dim) and the shape of the pooler's decoder layers (num_decoder_layers, num_decoder_attn_heads,
   * decoder_ffn_inner_dim or ffn_inner_dim; factory.py:190-226). */
  int32_t embedding_dim;
  int32_t pooler_layers;
  int32_t pooler_heads;
  int32_t pooler_ffn_dim;
} smi_text_encoder_config;
/* Shapes: the MFMA engines serve model_dim = num_heads * 64 in {256, 512, 768, 1024, 2048}, ffn_inner_dim % 128 == 0,
 * static pooling -- the released models.  EVERY OTHER shape the reference's factory accepts (any model_dim divisible by
 * num_heads with head_dim <= 256, attention pooling, the flags below other than FP16_RESIDUAL) runs on the library's
 * generic-dimension fp32 kernels (csrc/flex.hip), chosen inside smi_text_encoder_create. */

/* smi_text_encoder_config.flags */
/* Keep the residual stream in fp16 instead of fp32.  The reference's fp16 model does exactly this
 * (every tensor of the model is fp16, sonar/inference_pipelines/text.py:161-162 `.to(device, dtype)`);
 * the engine's default fp32 stream costs 2x the residual traffic and buys ~100x margin on the 1e-3
 * parity bound.  With the flag each residual add is one fp32 add rounded once to fp16. */
#define SMI_ENC_FP16_RESIDUAL 1
/* config.py `normalize_before`: the encoder stack ends in its own LayerNorm (StandardTransformerEncoder norm_order PRE,
 * factory.py:107-109, weights encoder_layer_norm_*) and the pooler's layers are pre-norm with a final LayerNorm. */
#define SMI_ENC_NORMALIZE_BEFORE 2
/* config.py `layernorm_embedding`: LayerNorm on the frontend output (weights embed_layer_norm_*). */
#define SMI_ENC_LAYERNORM_EMBEDDING 4
/* config.py `no_token_positional_embeddings`: pos_table is absent (data NULL).  (`learned_pos` needs no flag: the caller
 * passes encoder_frontend.pos_encoder.weight as pos_table with pos_offset 0.) */
#define SMI_ENC_NO_POSITIONS 8

/* Per-layer parameters, names as produced by the reference's checkpoint
 * conversion (sonar/models/sonar_text/handler.py:71-82).  Linear weights are
 * [out, in] row-major as in torch.nn.Linear. */
typedef struct smi_text_encoder_layer {
  smi_tensor self_attn_layer_norm_w, self_attn_layer_norm_b;
  smi_tensor q_w, q_b, k_w, k_b, v_w, v_b, out_w, out_b;
  smi_tensor ffn_layer_norm_w, ffn_layer_norm_b;
  smi_tensor ffn_inner_w, ffn_inner_b, ffn_out_w, ffn_out_b;
} smi_text_encoder_layer;

/* One decoder layer of the attention pooler (factory.py:199-218).  Its self-attention sees ONE token, so only the
 * value and output projections matter (softmax over one key is 1); the cross-attention reads the encoder output:
 * its k / v projections are [embedding_dim, model_dim]. */
typedef struct smi_text_pooler_layer {
  smi_tensor self_attn_layer_norm_w, self_attn_layer_norm_b;
  smi_tensor self_v_w, self_v_b, self_out_w, self_out_b;
  smi_tensor cross_layer_norm_w, cross_layer_norm_b;
  smi_tensor cross_q_w, cross_q_b, cross_k_w, cross_k_b, cross_v_w, cross_v_b, cross_out_w, cross_out_b;
  smi_tensor ffn_layer_norm_w, ffn_layer_norm_b;
  smi_tensor ffn_inner_w, ffn_inner_b, ffn_out_w, ffn_out_b;
} smi_text_pooler_layer;

typedef struct smi_text_encoder_weights {
  smi_tensor embed;     /* encoder_frontend.embed.weight [vocab, model_dim] */
  smi_tensor pos_table; /* position table [max_seq_len + pos_offset, model_dim] fp32 (sinusoidal or learned); data NULL =
                         * no_token_positional_embeddings */
  smi_tensor final_layer_norm_w, final_layer_norm_b; /* model-level layer_norm (factory.py:117) */
  const smi_text_encoder_layer* layers;              /* num_layers entries */
  /* the rest is read only when the configuration asks for it */
  smi_tensor encoder_layer_norm_w, encoder_layer_norm_b; /* encoder.layer_norm (SMI_ENC_NORMALIZE_BEFORE) */
  smi_tensor embed_layer_norm_w, embed_layer_norm_b;     /* encoder_frontend.layer_norm (SMI_ENC_LAYERNORM_EMBEDDING) */
  smi_tensor pooler_query;  /* [embedding_dim] fp32: pooler.decoder_frontend.embed.weight[bos] * sqrt(embedding_dim) +
                             * PE[0] -- the pooler's one input token after its frontend (encoder_pooler.py:78-92) */
  const smi_text_pooler_layer* pooler;                        /* pooler_layers entries */
  smi_tensor pooler_layer_norm_w, pooler_layer_norm_b;   /* pooler.decoder.layer_norm (SMI_ENC_NORMALIZE_BEFORE) */
  smi_tensor pooler_proj_w, pooler_proj_b;               /* pooler.projection_out [embedding_dim, embedding_dim] */
} smi_text_encoder_weights;

typedef struct smi_text_encoder smi_text_encoder; /* opaque */

/* Library / device ------------------------------------------------------- */
const char* smi_version(void);
/* ABI revision of this header: bumped whenever a struct grows, an argument list changes or a workspace formula
 * changes (round 2 = 2, round 3 = 3, ...).  A binding compares it with SMI_ABI_VERSION at load time and refuses a
 * library built from another revision (the structs carry no size field). */
#define SMI_ABI_VERSION 7
int smi_abi_version(void);
const char* smi_last_error(void);
/* Tuning registry (round 5).  Every A/B switch of the library -- engine-family thresholds, split-K part counts, storage
 * types, layout choices; the list with meanings and defaults is sonar_amd/csrc/tuning.hpp, enumerated here by
 * smi_tuning_name(0..) until it returns NULL -- is one process-wide integer that is set through these calls and read with
 * an atomic load.  THE LIBRARY NEVER READS THE ENVIRONMENT: a host that calls none of them runs the shipped defaults, and
 * results are a deterministic function of (inputs, batch row count, the switches set here) -- see INTEGRATION.md
 * "Numerics contract".  `name` with or without the "SMI_" prefix.  (The reference has no counterpart: its kernels are
 * ATen's, selected by torch's own heuristics.) */
int smi_tuning_set(const char* name, int32_t value);
int smi_tuning_unset(const char* name);
int smi_tuning_get(const char* name, int32_t* value, int32_t* is_set);
const char* smi_tuning_name(int32_t index);
/* Selects the HIP device for this thread (hipSetDevice). */
int smi_init(int device_id);
int smi_device_count(void);

/* Text encoder ------------------------------------------------------------
 * Stands in for: SonarTextEncoderFactory.create_model + checkpoint load
 * (sonar/models/sonar_text/factory.py:72-120, handler.py:52-94) and
 * SonarTextTransformerEncoderModel.forward (sonar/models/sonar_text/model.py:130-143)
 * as invoked by `.map(self.model)` in
 * TextToEmbeddingModelPipeline.predict (sonar/inference_pipelines/text.py:244). */
int smi_text_encoder_create(const smi_text_encoder_config* cfg, const smi_text_encoder_weights* w,
                            int64_t max_tokens_hint, smi_text_encoder** out);
void smi_text_encoder_destroy(smi_text_encoder* enc);

/* ids:      device int64 [n, s] right-padded token ids (SequenceBatch.seqs)
 * seq_lens: HOST int32 [n] valid lengths, or NULL when the batch is not ragged
 *           (PaddingMask is None, sonar/inference_pipelines/utils.py:18-21)
 * out_emb:  device [n, embedding_dim or model_dim] sentence_embeddings, out_dtype
 * out_encoded: optional device [n, s, model_dim] encoded_seqs (out_dtype), pads zeroed; may be NULL
 * stream:   hipStream_t (NULL = default stream) */
int smi_text_encoder_forward(smi_text_encoder* enc, const int64_t* ids, const int32_t* seq_lens,
                             int32_t n, int32_t s, void* out_emb, void* out_encoded,
                             int32_t out_dtype, void* stream);

/* Synchronises `stream` and reports what the device found while running the forward calls enqueued on
 * it: SMI_ERR_INVALID_ARG if a batch held token ids outside [0, vocab_size) -- the reference's
 * embedding lookup raises an IndexError there (tokenizer / model vocabulary mismatch); the engine never
 * reads outside the table and flags the batch instead.  The flag is reported (and cleared) ONLY here, after
 * the synchronisation -- smi_text_encoder_forward never refuses a later, valid batch because of it.
 * predict() calls this before it returns embeddings. */
int smi_text_encoder_status(smi_text_encoder* enc, void* stream);

/* Bytes of device memory currently held by the handle (weights + workspace). */
int64_t smi_text_encoder_device_bytes(const smi_text_encoder* enc);

/* Per-kernel timing with HIP events recorded on the caller's stream around every
 * launch of smi_text_encoder_forward (measurement aid for the roofline report; the
 * reference has no profiler).  Off by default. */
typedef enum smi_prof_slot {
  SMI_PROF_EMBED = 0,
  SMI_PROF_LAYERNORM = 1,
  SMI_PROF_GEMM_QKV = 2,
  SMI_PROF_ATTENTION = 3,
  SMI_PROF_GEMM_OUT = 4,
  SMI_PROF_GEMM_FFN1 = 5,
  SMI_PROF_GEMM_FFN2 = 6,
  SMI_PROF_LN_POOL = 7,
  SMI_PROF_SLOTS = 8
} smi_prof_slot;
int smi_text_encoder_set_profiling(smi_text_encoder* enc, int32_t enable);
/* Synchronises the recorded events, ADDS elapsed milliseconds and launch counts per
 * slot into ms[SMI_PROF_SLOTS] / launches[SMI_PROF_SLOTS], then clears the record. */
int smi_text_encoder_read_profile(smi_text_encoder* enc, double* ms, int64_t* launches);

/* Text decoder + beam search ---------------------------------------------------
 * Stands in for: SonarTextDecoderFactory.create_model + checkpoint load
 * (sonar/models/sonar_text/factory.py:229-315, handler.py:122-172), the
 * SonarEncoderDecoderModel.encode/decode/project calls of one generation step
 * (sonar/models/sonar_translation/model.py:48-78, DummyEncoderModel :81-95) and fairseq2's
 * BeamSearchSeq2SeqGenerator as driven by EmbeddingToTextModelPipeline.predict
 * (sonar/inference_pipelines/text.py:305-346). */
typedef struct smi_text_decoder_config {
  int32_t model_dim;     /* 1024; num_heads * 64 in {256, 512, 768, 1024, 2048} runs on the MFMA engines, any other
                          * multiple of num_heads with head_dim <= 256 (e.g. the `toy` arch) on the generic fp32 kernels */
  int32_t num_layers;    /* 24 */
  int32_t num_heads;     /* 16 */
  int32_t ffn_inner_dim; /* 8192 */
  int64_t vocab_size;    /* 256206 */
  int32_t max_seq_len;   /* 512: longest target sequence incl. prompt (config.py:197-219) */
  int32_t pos_offset;    /* 2 = model pad_idx + 1 (_legacy_pad_idx, factory.py:248-252) */
  int32_t input_dim;     /* conditioning vector dimension (config.py input_dim; model_dim when unset) */
  float embed_scale;     /* sqrt(model_dim) */
  float ln_eps;          /* 1e-5 */
  int32_t pad_idx, unk_idx, bos_idx, eos_idx; /* TOKENIZER ids: 0, 1, 2, 3.  pad / unk (-1 = none) and eos must be below 256 and
                                               * below vocab_size (SPECIAL IDS at smi_vocab_select), else SMI_ERR_UNSUPPORTED */
} smi_text_decoder_config;

/* encoder_decoder_attn q/k projections and its LayerNorm are not needed: the encoder output is
 * ONE vector, so the attention weight is 1 and the block reduces to W_o (W_v e + b_v) + b_o. */
typedef struct smi_text_decoder_layer {
  smi_tensor self_attn_layer_norm_w, self_attn_layer_norm_b;
  smi_tensor q_w, q_b, k_w, k_b, v_w, v_b, out_w, out_b;
  smi_tensor cross_v_w, cross_v_b, cross_out_w, cross_out_b;
  smi_tensor ffn_layer_norm_w, ffn_layer_norm_b;
  smi_tensor ffn_inner_w, ffn_inner_b, ffn_out_w, ffn_out_b;
} smi_text_decoder_layer;

typedef struct smi_text_decoder_weights {
  smi_tensor embed;     /* decoder_frontend.embed.weight [vocab, model_dim]; also the tied final_proj */
  smi_tensor pos_table; /* sinusoidal table [max_seq_len + pos_offset, model_dim] fp32 */
  smi_tensor final_layer_norm_w, final_layer_norm_b; /* decoder.layer_norm */
  const smi_text_decoder_layer* layers;
} smi_text_decoder_weights;

typedef struct smi_beam_search_params {
  int32_t beam_size;        /* 1..8 (fairseq2 default 5) */
  int32_t max_seq_len;      /* min(prompt_len + max_gen_len, model max): EOS is forced at max_seq_len-1 */
  int32_t min_seq_len;      /* prompt_len + min_gen_len: EOS blocked while step < min_seq_len */
  int32_t normalize_scores; /* 1: score / (len - 1)^len_penalty */
  float len_penalty;        /* 1.0 */
  float unk_penalty;        /* 0.0 */
  float temperature;        /* 1.0 */
  int32_t reserved;
} smi_beam_search_params;

typedef struct smi_text_decoder smi_text_decoder; /* opaque */

int smi_text_decoder_create(const smi_text_decoder_config* cfg, const smi_text_decoder_weights* w,
                            smi_text_decoder** out);
void smi_text_decoder_destroy(smi_text_decoder* dec);

/* Teacher-forced logits (the reference test's call, tests/integration_tests/test_text_sonar.py:61-105):
 * emb device [n, model_dim] (emb_dtype), prev_tokens device int64 [n, t], out_logits device fp32 [n, t, vocab]. */
int smi_text_decoder_logits(smi_text_decoder* dec, const void* emb, int32_t emb_dtype, int32_t n,
                            const int64_t* prev_tokens, int32_t t, float* out_logits, void* stream);

/* Teacher-forced scoring (forced decoding): log p(text | sentence embedding), token by token, in one parallel forward.
 * emb device [n, input_dim] (emb_dtype SMI_F32 / SMI_F16); tokens device int64 [n, t], row s's sequence is
 * tokens[s, 0 .. lens[s]) with the prompt first; lens HOST int32 [n], 1 <= lens[s] <= t <= max_seq_len + 1.
 * out_logprobs device fp32 [n, t - 1]:
 *   out[s, j] = log_softmax(logits(emb_s, tokens[s, 0 .. j]))[tokens[s, j + 1]]   for j < lens[s] - 1,   0 beyond.
 * Plain log-softmax at temperature 1: no PAD / EOS masking, no unk_penalty, no step processors -- the beam search applies
 * those after its log-softmax, so the normaliser is the same.  Positions >= lens[s] are never read (any value, out-of-range
 * ids included).  An id outside [0, vocab) inside a length fails the call with SMI_ERR_INVALID_ARG (it is never used as an
 * index; the handle stays usable).  Synchronises `stream` once, at the end. */
int smi_text_decoder_score(smi_text_decoder* dec, const void* emb, int32_t emb_dtype, int32_t n, const int64_t* tokens,
                           int32_t t, const int32_t* lens, float* out_logprobs, void* stream);

/* Beam search for n sentence embeddings.  prompt: HOST int64 [prompt_len] (= [</s>, __lang__]).
 * Outputs (device): out_tokens int32 [n, beam, max_seq_len] generated tokens after the prompt incl. the
 * final EOS, -1 padded; out_lens int32 [n, beam]; out_scores fp32 [n, beam]; hypotheses best first
 * (the reference decodes hypotheses[0]).  Synchronises `stream` every 8 steps to test for completion. */
int smi_text_decoder_generate(smi_text_decoder* dec, const void* emb, int32_t emb_dtype, int32_t n,
                              const int64_t* prompt, int32_t prompt_len, const smi_beam_search_params* params,
                              int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream);

/* smi_text_decoder_generate with one prompt PER SENTENCE: different target languages in one call, or forced prefixes that
 * differ from sentence to sentence (fairseq2's `prompt_seqs` [n, P] with a padding mask).  prompts: HOST int64
 * [n, prompt_stride], left-aligned; prompt_lens: HOST int32 [n], 1 <= prompt_lens[s] <= prompt_stride; entries past a
 * sentence's length are not read.  Sentence s returns exactly what smi_text_decoder_generate returns for it when called
 * with the same n embeddings and the one prompt prompts[s]: its result does not depend on the other sentences' prompts.
 * Every sentence sits at the same position each step; sentence s is forced to prompts[s][step] while step <
 * prompt_lens[s] (those log-probabilities count towards its score) and free afterwards.
 * How the length fields are read here -- they cannot carry per-sentence values:
 *   params->max_seq_len  the model-side cap of prompt + generated tokens, in [2, the decoder's max_seq_len];
 *   params->min_seq_len  not read;
 *   gen_cap (>= 1)       most generated tokens per sentence:  max_len_s = min(prompt_lens[s] + gen_cap, params->max_seq_len);
 *   min_gen_len (>= 0)   fewest:                              min_len_s = min(prompt_lens[s] + min_gen_len, max_len_s).
 * EOS is blocked while step < min_len_s and forced at step == max_len_s - 1; unk_penalty, the step processors and the
 * decision margins act on a sentence's own free steps.  A sentence with max_len_s <= prompt_lens[s], or a prompt token
 * outside the vocabulary, fails the call with SMI_ERR_INVALID_ARG naming the row.
 * Outputs as smi_text_decoder_generate, the row length of out_tokens being W = max over s of max_len_s:
 * out_tokens int32 [n, beam, W], sentence s's tokens after ITS prompt, -1 padded.  A call whose prompts are all equal runs
 * as the one-prompt call, launch for launch. */
int smi_text_decoder_generate_prompts(smi_text_decoder* dec, const void* emb, int32_t emb_dtype, int32_t n,
                                      const int64_t* prompts, int32_t prompt_stride, const int32_t* prompt_lens,
                                      int32_t gen_cap, int32_t min_gen_len, const smi_beam_search_params* params,
                                      int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream);

/* Decision margins of the LAST smi_text_decoder_generate / smi_text_decoder_generate_prompts call on this handle: out_margins device fp32
 * [n, 2].  [s][0] = the smallest gap, over all free decoding steps of sentence s, between neighbouring
 * entries of the sorted beam x vocab candidate list among the candidates the beam rules consumed plus
 * the first one they did not (log-prob units; for beam_size 1 this is the greedy top-1 / top-2 margin);
 * [s][1] = normalised score of the returned hypothesis minus the runner-up's (+inf if there is none).
 * "Exact token-id match for greedy decode" (BASELINE north_star) is tested as: every token equal to the
 * fp32 CPU oracle's unless [s][0] is below the epsilon stated in the test. */
int smi_text_decoder_last_margins(smi_text_decoder* dec, float* out_margins, int32_t n, void* stream);

/* Independent decode chains of smi_text_decoder_generate (round 4).  Sentences do not interact in
 * EmbeddingToTextModelPipeline.predict (sonar/inference_pipelines/text.py:329-346 decodes buckets of sentences), so a
 * large batch may run as `chains` sentence groups, each with its own workspace, KV cache, beam state, stream and host
 * thread: one group's per-launch fixed costs fall under the other's K loops.  0 = the engine's choice (tuning
 * switch DEC_CHAINS, else the built-in default), 1 = one chain, up to 4.  Hypotheses equal the single chain's up to the
 * fp32 summation order of split-K slabs. */
int smi_text_decoder_set_chains(smi_text_decoder* dec, int32_t chains);

/* Storage type of the logits inside smi_text_decoder_generate (round 4): SMI_F32 (default) or SMI_F16.  The reference's fp16
 * model produces fp16 logits (the tied final_proj is an fp16 Linear; fairseq2's beam search up-casts them inside
 * log_softmax, sonar/inference_pipelines/text.py:305-346 -> BeamSearchSeq2SeqGenerator), so SMI_F16 is what an fp16 model's
 * pipeline selects: the logits GEMM then rounds its fp32 accumulators to fp16 once, takes the softmax statistics of the
 * ROUNDED values and writes half the bytes (0.66 instead of 1.31 GB per position at 256 sentences x beam 5).
 * smi_text_decoder_logits and smi_text_decoder_sample keep fp32 logits and fp32 partial sums. */
int smi_text_decoder_set_beam_logits_dtype(smi_text_decoder* dec, int32_t dtype);

/* Storage type of the split-K PARTIAL sums of the attention-output and FFN-output projections inside
 * smi_text_decoder_generate: SMI_F32 (default) or SMI_F16 (round 4; its own setting since round 5, it used to follow the
 * logits dtype).  With SMI_F16 each partial is rounded to fp16 once -- SATURATING at +-65504 (MODE.FP16_OVFL), so a partial
 * outside fp16's range cannot turn a representable sum into inf --, the consumer widens, sums in fp32 in slab order and adds to
 * the fp32 residual stream.  The reference's fp16 model rounds the FULL sublayer output to fp16 once
 * (sonar/inference_pipelines/text.py:36-54 puts the whole model in fp16); rounding 2-8 partials instead bounds the error by
 * 2^-11 x the sum of the partials' magnitudes rather than of the result's -- the same order unless the K ranges cancel
 * (tests/test_gpu_kernels.py::test_splitk_f16_slabs_cancellation_and_saturation).  It halves the 42 MB per layer the FFN
 * output projection writes and the next kernel reads at 1 280 rows (-3.9 % of a C5 step).  An fp16 model's Python engine
 * (TextDecoderEngine(dtype=float16)) selects it; a C caller gets fp32 partial sums unless it asks. */
int smi_text_decoder_set_slab_dtype(smi_text_decoder* dec, int32_t dtype);

/* Step processors of smi_text_decoder_generate / smi_text_decoder_sample (fairseq2's NGramRepeatBlockProcessor and
 * BannedSequenceProcessor, handed over as `step_processors=` by the reference's pipelines).  They act on the FREE steps only
 * (not on the teacher-forced prompt steps, not on the forced EOS at max_seq_len - 1), on the row's sequence so far, prompt
 * included:
 *   ngram_size n >= 1: for every window start i in [0, L - n] whose n - 1 tokens equal the last n - 1 tokens of the
 *     sequence (length L), the token s[i + n - 1] is banned; n = 1 bans every token present, the prompt's EOS included
 *     (generation then runs to the length cap); 0 = off.
 *   banned sequence b (HOST CSR: tokens banned_tokens[banned_offsets[q] .. banned_offsets[q + 1]), num_banned of them, each
 *     non-empty): b[-1] is banned when the last len(b) - 1 tokens equal b[:-1]; a length-1 sequence is banned always.
 * Beam search: a banned token's log-probability is -inf AFTER log_softmax (the normaliser is the untouched row's).
 * Sampling: its probability is 0 before the top-k / top-p filter (not renormalised first). */
typedef struct smi_step_processors {
  int32_t ngram_size;
  int32_t num_banned;
  const int32_t* banned_tokens;   /* host */
  const int32_t* banned_offsets;  /* host [num_banned + 1], banned_offsets[0] == 0 */
} smi_step_processors;

/* Per-handle setting, as smi_text_decoder_set_chains: NULL (or all off) clears it.  The banned-sequence table is copied to
 * the device here.  Errors: token ids outside the vocabulary, empty sequences, more than 1024 sequences, a sequence or an
 * ngram_size longer than the decoder's max_seq_len, or a max_seq_len above 1023.  A row whose every token is banned (a
 * small vocabulary can be covered) gets no candidate in the beam search (its slot goes inert, as when fewer than `beam`
 * continuations exist) and, when sampling, ends with EOS at log-probability -inf. */
int smi_text_decoder_set_step_processors(smi_text_decoder* dec, const smi_step_processors* procs);

/* The beam search's vocabulary selection under step processors on given logits, for the parity tests: logits device fp32
 * [rows, ldl] row-major, or (logits_f16_tm) fp16 in the tile-major layout with K = ldl; tile_max / tile_sum device fp32
 * [ldl / 256][rows] (per 256-column tile: maximum and sum of exp(v - maximum)); hist device int32 [rows, hist_stride], row r's
 * sequence so far hist[r][0 .. hist_len); pad_idx (-1 = none, else below 256 and below vocab: SPECIAL IDS at smi_vocab_select) is
 * never a candidate.  Outputs (device): pval fp32 / pidx
 * int32 [rows, 16], the first k2 (<= 16) entries = the top-k2 of the masked row (value desc, token asc; -inf / INT32_MAX
 * when fewer remain), and pmax / psum fp32 [rows], the untouched row's softmax normaliser.  With no processor active the
 * engine's default selection runs, as in smi_text_decoder_generate. */
int smi_vocab_select_banned(const void* logits, int32_t ldl, int32_t logits_f16_tm, int32_t rows, int32_t vocab,
                            const float* tile_max, const float* tile_sum, int32_t k2, int32_t pad_idx,
                            const int32_t* hist, int32_t hist_stride, int32_t hist_len, const smi_step_processors* procs,
                            float* pval, int32_t* pidx, float* pmax, float* psum, void* stream);

/* smi_sample_rows under step processors, for the parity tests: every row's sequence so far is hist (device int32
 * [hist_len]), and the ids the processors ban get mass 0 in the filter and the draw.  When the kept set's Q40 mass is 0 (a
 * banned token holds the row maximum far above every kept one) the most probable kept token is returned, lowest id on a tie,
 * with its exact log-probability. */
int smi_sample_rows_banned(const float* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t sampler, int32_t top_k,
                           float top_p, float temperature, int32_t pad_idx, int32_t eos_idx, int32_t block_eos,
                           int32_t unk_idx, float unk_penalty, const int32_t* hist, int32_t hist_len,
                           const smi_step_processors* procs, const uint64_t* z, int32_t* out_token, float* out_logprob,
                           uint64_t* out_kept_mass, int32_t* out_kept_count, void* stream);

/* Sampling generation (sonar/inference_pipelines/text.py:315-320: a `sampler` makes predict() build
 * fairseq2's SamplingSeq2SeqGenerator instead of the beam search; one hypothesis per sentence).
 * Per step: probs = softmax(logits / temperature) in fp32, pad -> 0, EOS -> 0 before min_seq_len,
 * probs[unk] -= unk_penalty (a result <= 0 removes the token), EOS forced at max_seq_len - 1; TopKSampler keeps the k most probable tokens, TopPSampler the sorted
 * prefix whose exclusive cumulative probability stays <= p; one token is drawn from the renormalised
 * kept set; the step score is log(probs[token]).  The draw is a counter-based hash of
 * (seed, sentence, step): a call is reproducible, and independent of the batch it runs in. */
#define SMI_SAMPLER_TOP_K 0
#define SMI_SAMPLER_TOP_P 1
typedef struct smi_sampling_params {
  int32_t sampler;          /* SMI_SAMPLER_TOP_K / SMI_SAMPLER_TOP_P */
  int32_t top_k;            /* TopKSampler(k), k >= 1 */
  float top_p;              /* TopPSampler(p), 0 < p <= 1 */
  float temperature;        /* 1.0 */
  int32_t max_seq_len;      /* as smi_beam_search_params */
  int32_t min_seq_len;
  int32_t normalize_scores; /* 1: score / (len - 1)^len_penalty */
  float len_penalty;        /* 1.0 */
  uint64_t seed;
  float unk_penalty;        /* 0.0; subtracted from the PROBABILITY of the UNK token (fairseq2's sampling generator) */
} smi_sampling_params;

/* Outputs (device): out_tokens int32 [n, max_seq_len] generated tokens after the prompt incl. the final
 * EOS, -1 padded; out_lens int32 [n]; out_scores fp32 [n].  prompt: HOST int64 [prompt_len]. */
int smi_text_decoder_sample(smi_text_decoder* dec, const void* emb, int32_t emb_dtype, int32_t n,
                            const int64_t* prompt, int32_t prompt_len, const smi_sampling_params* params,
                            int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream);

/* smi_text_decoder_sample with one prompt per sentence: the prompt triple, gen_cap / min_gen_len and the reading of
 * params->max_seq_len (the model-side cap) / params->min_seq_len (not read) are those of smi_text_decoder_generate_prompts;
 * out_tokens int32 [n, W].  The draw of a sentence depends on (seed, sentence, step) only, so sentence s returns what
 * smi_text_decoder_sample returns for it with the one prompt prompts[s]. */
int smi_text_decoder_sample_prompts(smi_text_decoder* dec, const void* emb, int32_t emb_dtype, int32_t n,
                                    const int64_t* prompts, int32_t prompt_stride, const int32_t* prompt_lens,
                                    int32_t gen_cap, int32_t min_gen_len, const smi_sampling_params* params,
                                    int32_t* out_tokens, int32_t* out_lens, float* out_scores, void* stream);

/* The filter + draw of one sampling step on given logits (device fp32 [rows, ld], ld % 4 == 0,
 * ld >= vocab rounded up to 4, vocab <= 2^18), exposed for the parity tests: z device uint64 [rows]
 * random words (the draw is floor(z * kept_mass / 2^64) into the kept mass); outputs device:
 * out_token int32 [rows], out_logprob fp32 [rows], and optionally the kept set's size and its mass in
 * Q40 fixed point relative to exp(max scaled logit). */
int smi_sample_rows(const float* logits, int64_t ld, int32_t rows, int32_t vocab, int32_t sampler, int32_t top_k,
                    float top_p, float temperature, int32_t pad_idx, int32_t eos_idx, int32_t block_eos,
                    int32_t unk_idx, float unk_penalty, const uint64_t* z, int32_t* out_token, float* out_logprob,
                    uint64_t* out_kept_mass, int32_t* out_kept_count, void* stream);

/* Speech encoder -------------------------------------------------------------------
 * Stands in for: WaveformToFbankConverter(num_mel_bins=80, waveform_scale=2**15,
 * standardize=True) (sonar/inference_pipelines/speech.py:283-290), SonarSpeechEncoderFactory +
 * checkpoint load (sonar/models/sonar_speech/factory.py:53-152, handler.py:46-110) and
 * SonarSpeechEncoderModel.forward (sonar/models/sonar_speech/model.py:59-77) as invoked by
 * SpeechToEmbeddingModelPipeline.predict (speech.py:431-474). */
typedef struct smi_speech_encoder_config {
  int32_t model_dim;        /* 1024 = num_heads*64 */
  int32_t num_layers;       /* 24 conformer blocks */
  int32_t num_heads;        /* 16 */
  int32_t ffn_inner_dim;    /* 4096 */
  int32_t conv_kernel;      /* 31 (7 also built, for tests) */
  int32_t num_mel_bins;     /* 80; two frames are stacked -> feature_dim 160 */
  int32_t pooler_layers;    /* 3 ("english") / 6 ("non_english") */
  int32_t pooler_heads;     /* 16 */
  int32_t pooler_ffn_dim;   /* 4096 */
  int32_t pooler_vocab;     /* rows of the pooler embedding (= model_dim, factory.py:94-100) */
  int32_t bos_idx;          /* 2 */
  int32_t max_frames;       /* largest number of STACKED frames per clip (rel-pos table), e.g. 4096 */
  float ln_eps, bn_eps;     /* 1e-5, 1e-5 */
  int32_t flags;            /* SMI_ENC_FP16_RESIDUAL: fp16 residual stream, as the reference's `.half()` model */
  int32_t reserved;
} smi_speech_encoder_config;

typedef struct smi_conformer_layer {
  smi_tensor ffn1_layer_norm_w, ffn1_layer_norm_b, ffn1_inner_w, ffn1_inner_b, ffn1_out_w, ffn1_out_b;
  smi_tensor self_attn_layer_norm_w, self_attn_layer_norm_b;
  smi_tensor q_w, q_b, k_w, k_b, v_w, v_b, out_w, out_b;
  smi_tensor r_proj_w, u_bias, v_bias;             /* self_attn.sdpa.* */
  smi_tensor conv_layer_norm_w, conv_layer_norm_b;
  smi_tensor pointwise_conv1_w;                    /* [2d, d] (kernel size 1 squeezed), no bias */
  smi_tensor depthwise_conv_w;                     /* [d, k] */
  smi_tensor batch_norm_w, batch_norm_b, batch_norm_mean, batch_norm_var;
  smi_tensor pointwise_conv2_w;                    /* [d, d] */
  smi_tensor ffn2_layer_norm_w, ffn2_layer_norm_b, ffn2_inner_w, ffn2_inner_b, ffn2_out_w, ffn2_out_b;
  smi_tensor layer_norm_w, layer_norm_b;           /* final LayerNorm of the block */
} smi_conformer_layer;

/* POST-norm decoder layer of the attention pooler.  The self-attention runs over ONE token, so
 * its q/k projections cannot influence the output and are not needed. */
typedef struct smi_pooler_layer {
  smi_tensor self_v_w, self_v_b, self_out_w, self_out_b, self_attn_layer_norm_w, self_attn_layer_norm_b;
  smi_tensor cross_q_w, cross_q_b, cross_k_w, cross_k_b, cross_v_w, cross_v_b, cross_out_w, cross_out_b;
  smi_tensor cross_layer_norm_w, cross_layer_norm_b;
  smi_tensor ffn_inner_w, ffn_inner_b, ffn_out_w, ffn_out_b, ffn_layer_norm_w, ffn_layer_norm_b;
} smi_pooler_layer;

typedef struct smi_speech_encoder_weights {
  smi_tensor post_extract_layer_norm_w, post_extract_layer_norm_b; /* [2*num_mel_bins] */
  smi_tensor model_dim_proj_w, model_dim_proj_b;                   /* [d, 2*num_mel_bins], [d] */
  smi_tensor layer_norm_w, layer_norm_b;                           /* model-level LN (handler.py:102-108) */
  smi_tensor pooler_embed;                                         /* [pooler_vocab, d] */
  smi_tensor pooler_projection_out_w;                              /* [d, d], no bias */
  const smi_conformer_layer* layers;
  const smi_pooler_layer* pooler;
} smi_speech_encoder_weights;

typedef struct smi_speech_encoder smi_speech_encoder; /* opaque */

int smi_speech_encoder_create(const smi_speech_encoder_config* cfg, const smi_speech_encoder_weights* w,
                              smi_speech_encoder** out);
void smi_speech_encoder_destroy(smi_speech_encoder* enc);

/* fbank: device fp32 [n, t, num_mel_bins] zero-padded, t even (Collater pad_to_multiple=2,
 * speech.py:444); fbank_lens: HOST int32 [n] frames per clip or NULL; out_emb device [n, model_dim]. */
int smi_speech_encoder_forward(smi_speech_encoder* enc, const float* fbank, const int32_t* fbank_lens,
                               int32_t n, int32_t t, void* out_emb, int32_t out_dtype, void* stream);

/* Kaldi-compatible log-mel filterbank of ONE 16 kHz clip: wave device fp32 [nsamples] in [-1, 1],
 * out device fp32 [smi_fbank_num_frames(nsamples), 80].  25 ms / 10 ms frames, povey window,
 * pre-emphasis 0.97, DC removal, 512-point FFT, 80 mel bins from 20 Hz, log power, snip_edges. */
int64_t smi_fbank_num_frames(int64_t nsamples);
int smi_fbank(const float* wave, int64_t nsamples, float waveform_scale, int32_t standardize, float* out,
              void* stream);

/* The same filterbank for a whole batch in one launch: waves device fp32, the clips back to back;
 * offsets HOST int64 [n + 1] (clip i = samples offsets[i] .. offsets[i+1]); out device fp32
 * [n, tpad, 80], tpad >= every clip's frame count, rows past a clip's frames are set to 0 (the
 * reference's Collater pad value, speech.py:444).  Stands in for the per-file
 * WaveformToFbankConverter map + Collater of SpeechToEmbeddingModelPipeline.predict (speech.py:431-452). */
int smi_fbank_batch(const float* waves, const int64_t* offsets, int32_t n, float waveform_scale, int32_t standardize,
                    float* out, int64_t tpad, void* stream);

/* Sample-rate conversion in front of the filterbank: the windowed-sinc polyphase resampler that torchaudio's
 * functional.resample applies by default (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).  With g = gcd(orig, new),
 * o = orig / g, n = new / g:
 *   base = min(o, n) * 0.99, width = ceil(6 o / base), 2 width + o taps per phase
 *   k[p][i] = sinc(t) cos(pi t / 12)^2 base / o,  t = ((i - width) / o - p / n) base clamped to [-6, 6]   (double, stored fp32)
 *   y[m n + p] = sum_i k[p][i] x[m o + i - width],  x zero outside the clip;  ceil(n L / o) outputs for L samples
 * Per phase only `support` = floor(12 o / base) + 1 consecutive taps are non-zero in fp32; the engine keeps that compact
 * table and the first tap index of every phase, cached per (o, n) for the life of the process.  Rates <= 0 or above 2^20
 * and pairs whose compact table exceeds 16 MiB return SMI_ERR_UNSUPPORTED.
 * smi_resample_num_samples: the output length (< 0 on bad rates).  smi_resample_filter: the table itself, host only, needs
 * no device; taps [phases * support] and first [phases] may be NULL to ask for the sizes alone. */
int64_t smi_resample_num_samples(int64_t nsamples, int32_t orig_rate, int32_t new_rate);
int smi_resample_filter(int32_t orig_rate, int32_t new_rate, int32_t* phases, int32_t* support, int32_t* width, float* taps,
                        int32_t* first);
/* One launch for a ragged batch: waves device fp32, the clips back to back at their own rates; in_offsets HOST int64
 * [n + 1], rates HOST int32 [n]; out device fp32, clip i at out_offsets[i] .. out_offsets[i + 1] (HOST int64 [n + 1]), which
 * must hold exactly smi_resample_num_samples(len_i, rates[i], new_rate) samples; nothing outside out_offsets[0] ..
 * out_offsets[n] is written.  A clip already at new_rate is copied bit for bit, an empty clip produces nothing.  Every output is accumulated in fp32 over its taps in
 * ascending order, so its value depends on its clip, the two rates and its index alone -- not on the rest of the batch.
 * Asynchronous on `stream`. */
int smi_resample_batch(const float* waves, const int64_t* in_offsets, const int32_t* rates, int32_t n, int32_t new_rate,
                       float* out, const int64_t* out_offsets, void* stream);

/* xsim mining ---------------------------------------------------------------
 * Stands in for the similarity search the reference performs as
 * F.normalize(x) @ F.normalize(y).T (tests/integration_tests/test_text_sonar.py:42-53)
 * and that xsim (README.md:5) evaluates: for each of the nx rows of X return the
 * k (<= 8) most cosine-similar rows of Y, best first.
 *
 * smi_xsim_normalize: dst = f16 row-normalised copy of src, padded with zero
 *   rows to a multiple of 256 rows (dst must hold smi_xsim_padded_rows(rows)*d f16).
 * smi_xsim_topk: Xn/Yn are such normalised, padded matrices.  idx [nx,k] int32
 *   (row index in Y plus y_index_offset; -1 if fewer than k candidates),
 *   score [nx,k] fp32.  workspace: smi_xsim_workspace_bytes() bytes of device memory (the per-chunk partial
 *   lists and, for k <= 4, tile-major copies of both matrices: the mining kernel streams those); workspace_bytes =
 *   what the caller allocated -- a buffer smaller than the formula of THIS library is refused, not overrun. */
int64_t smi_xsim_padded_rows(int64_t rows);
int smi_xsim_normalize(const void* src, int32_t src_dtype, int64_t rows, int32_t d, void* dst_f16,
                       void* stream);
int64_t smi_xsim_workspace_bytes(int64_t nx, int64_t ny, int32_t k, int32_t d);
int smi_xsim_topk(const void* xn_f16, int64_t nx, const void* yn_f16, int64_t ny, int32_t d,
                  int32_t k, int64_t y_index_offset, int32_t* idx, float* score, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* smi_xsim_topk on int8 rows: the brute-force pass with the score of the int8 IVF index,
 *   score = fl32(fl32((float)acc * y_scales[n]) * x_scales[m]),  acc = the int32 dot product of the two code rows (exact),
 * so the bits are those smi_ivf_i8_search returns for the same two fp16 rows (X is the query side, Y the stored side).
 * x_codes / y_codes: int8 [smi_xsim_padded_rows(rows), d], x_scales / y_scales: fp32 [padded rows], as smi_ivf_i8_encode writes
 * them over the WHOLE padded output of smi_xsim_normalize (a zero pad row encodes to codes 0 and scale 0); all four 16-byte
 * aligned.  idx / score: smi_xsim_topk's layout, total order (score descending, ties to the lower index) and (-1, -inf) fill.
 * A list orders by the bits of a score, where -0 sorts below +0 (the rule of the IVF scans); no row smi_ivf_i8_encode writes
 * scores -0.  workspace: smi_xsim_workspace_bytes(nx, ny, k, d / 2) bytes, 16-byte aligned -- the fp16 pass's sizing call at
 * HALF the dimension (an int8 [rows, d] matrix is an fp16 [rows, d / 2] matrix in bytes); there is no sizing call of its own.
 * The call uses the partial lists fp32 + int32 [min(padded ny / 256, 8)][padded nx][k rounded up to 1, 2, 4, 8] and the
 * tile-major copies of both code matrices: exactly that many bytes from 2048 padded y rows on, a few lists fewer below.
 * (The sizing call knows nothing of int8: it returns a size for a d this entry refuses.)
 * Refused before any launch: k outside [1, 8], d not a multiple of 64, d > SMI_IVF_I8_MAX_DIM, empty input, rows that do not fit
 * int32, null or misaligned pointers, a short workspace.  Nothing is read back or allocated: the call can be captured into a
 * graph. */
int smi_xsim_topk_i8(const void* x_codes, const float* x_scales, int64_t nx, const void* y_codes, const float* y_scales,
                     int64_t ny, int32_t d, int32_t k, int64_t y_index_offset, int32_t* idx, float* score, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* Paged top-k (restated in tests/topk_wide_ref.py): k above the list length of one pass, 16 results at a time.
 * THE CONTRACT OF A PAGE, for this entry and smi_ivf_search_page: for every row, the k <= 16 best candidates (s, i) in the total
 * order (score descending, ties to the lower id) that come strictly AFTER the row's exclusive ceiling (cs, ci) = (ceil_score[r],
 * ceil_idx[r]): s < cs, or s == cs and i > ci, i being the id as returned (the y row number plus y_index_offset here, the
 * effective id of an index).  ceil_score / ceil_idx null (both or neither): no ceiling, the first page.  A row whose ceiling
 * id is negative is exhausted and returns only fill; fill is (-1, -inf) as everywhere.  A ceiling need not be a candidate.  A
 * NaN ceiling score is not in the order: unspecified.  The last entry of page p is the ceiling of page p + 1 (a fill entry
 * exhausts the row), and the pages concatenated are the top-k bit for bit: the bits of a row's result depend on the two rows
 * and the ceiling alone, whatever the batch, the run or the split into pages.  A zero score is returned and compared as +0.
 * smi_xsim_topk_page: the arguments of smi_xsim_topk and the ceilings, fp32 / int32 [nx].  workspace:
 *   smi_xsim_topk_page_ws_bytes(nx, ny, k, d) bytes, 16-byte aligned (lists of 16 whatever k, the tile-major copies, one
 *   64-bit ceiling key per padded row).  Refused before any launch: k outside [1, 16], d not a multiple of 64, empty input, rows
 *   that do not fit int32, a null pointer, one ceiling array without the other, a short or misaligned workspace; the sizing call
 *   returns 0 for such a shape.  Nothing is read back or allocated: the call can be captured into a graph. */
int64_t smi_xsim_topk_page_ws_bytes(int64_t nx, int64_t ny, int32_t k, int32_t d);
int smi_xsim_topk_page(const void* xn_f16, int64_t nx, const void* yn_f16, int64_t ny, int32_t d, int32_t k,
                       int64_t y_index_offset, const float* ceil_score, const int32_t* ceil_idx, int32_t* idx, float* score,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Squared-Euclidean and inner-product search on rows AS THEY ARE (restated in tests/l2_ref.py).  With
 * b[j] = -1/2 ||y_j||^2, argmax_j (x . y_j + b[j]) = argmin_j ||x - y_j||^2 and ||x - y_j||^2 = 2 (1/2 ||x||^2 - score): one
 * additive term per y row makes the brute-force pass an L2 search.  The zero bias is maximum inner product; for that
 * smi_xsim_topk itself serves on prepared rows (it never needed unit rows: its score is the fp32 sum of the tile).
 * smi_l2_prepare: dst_f16 = the fp16 copy of src (round to nearest even from fp32), [smi_xsim_padded_rows(rows), d], the
 *   rows from `rows` on zero: smi_xsim_normalize without the division.  half_norms (fp32 [padded rows], or NULL):
 *   h[r] = fl32(1/2 S_r), S_r = the sum of the squares of the ROUNDED row, pad rows 0.  The squares are exact in fp64 and are
 *   added in fp64 in THIS ORDER, which depends on d alone: the row is d / 8 chunks of 8 consecutive columns; for l = 0 .. 63,
 *   p[l] = the sum, from 0, of the squares of chunks l, l + 64, l + 128, ... in that order, the 8 columns of a chunk in
 *   ascending order; then six steps off = 32, 16, 8, 4, 2, 1, each replacing every p[l] by p[l] + p[l ^ off] at once; S_r = p[0].
 *   A row holding a value that is not finite in fp16 (after the rounding) gives unspecified results, here and downstream.
 *   d a multiple of 8; src and dst 16-byte aligned.
 * smi_l2_topk: x_f16 / y_f16 are such prepared, padded matrices (or any fp16 rows in that layout), y_bias fp32
 *   [smi_xsim_padded_rows(ny)], finite (otherwise unspecified), 16-byte aligned.  score(i, j) = fl32(acc(i, j) + y_bias[j]), acc
 *   the fp32 sum smi_xsim_topk's tile produces for the two rows.  idx / score: smi_xsim_topk's layout, total order (score
 *   descending, ties to the lower index) and (-1, -inf) fill; rows j >= ny never enter, whatever their bias.  A zero score is
 *   +0.  The bits of a row's result depend on the two rows and the bias alone: the same alone or in any batch, on any run.
 *   workspace: smi_l2_topk_ws_bytes(nx, ny, k, d) bytes, 16-byte aligned.  Refused before any launch: what smi_xsim_topk
 *   refuses for the shape (k outside [1, 8], d not a multiple of 64, empty input, a null pointer, a short workspace), rows that
 *   do not fit int32, a null or misaligned bias; the sizing call returns 0 for such a shape.  Nothing is read back or
 *   allocated: the call can be captured into a graph.
 * smi_l2_slot_bias: out[s] = -half_norms[list_ids[s]], and 0 where list_ids[s] < 0 (a pad or unused slot), for the `slots`
 *   entries of an IVF index's list_ids: the bias of every slot, in slot order.
 * smi_l2_flat_search: smi_ivf_search with its arguments and list_bias (fp32 [capacity_slots], 16-byte aligned,
 *   from smi_l2_slot_bias) behind list_rows: q_f16 prepared queries, the lists built by smi_ivf_build over prepared rows, probes
 *   from smi_l2_topk against the centroids with their bias.  score = fl32(sum + list_bias[slot]), sum what smi_ivf_search
 *   returns for the two rows; everything else -- order, fill, unit rule, probes that name no list, pad slots (out by their id,
 *   whatever their bias), refusals, the workspace (smi_l2_flat_search_ws_bytes = the flat search's size) -- is smi_ivf_search's.
 *   A row mask works as there: ids of -1.  k and nprobe in [1, 8].
 * Euclidean k-means (restated in tests/l2_ref.py).  x_f16: prepared rows.  The update is smi_kmeans_update, unchanged: its
 *   integer sums are exact for any finite fp16 rows.
 * smi_l2_kmeans_finalize: for a cluster with counts[c] > 0, centroids_f32[c][j] = fl32(fl64(sums[c][j]) * 2^-24 /
 *   fl64(counts[c])) (int64 -> fp64 by round to nearest even; that expression is the contract), row c of centroids_f16 its round
 *   to nearest even, centroid_half_norms[c] the half norm of that fp16 row in smi_l2_prepare's order.  A cluster without
 *   members keeps all three; *empty_count (device int32, overwritten) = the number of those.  centroids_f16 has
 *   smi_xsim_padded_rows(K) rows and centroid_half_norms as many entries; those from K on are zeroed.
 * smi_l2_kmeans_fit: smi_kmeans_fit's loop, records and arguments, and centroid_half_norms behind centroids_f16.
 *   resume = 0: centroids_f32 holds the K initial centroids; centroids_f16 / centroid_half_norms = smi_l2_prepare of them;
 *   every row is assigned by smi_l2_topk's pass at k = 1 with the bias -centroid_half_norms (ties to the lower index: a
 *   duplicate centroid stays empty); then n_iter rounds of update -> finalise -> assign.  resume = 1 continues on the same
 *   buffers; fit(0) followed by T calls of fit(1, resume) equals fit(T) bit for bit.  scores: the score of every row against
 *   its centroid, x . c - h_c; objective: their fp64 sum in smi_kmeans_fit's fixed order, so the inertia sum ||x - c||^2 is
 *   2 (sum_i h_x[i] - objective).  moved / empty / sums / counts as there.  Nothing is read back: capturable.
 *   workspace: smi_l2_kmeans_fit_ws_bytes(n, K, d) bytes, 16-byte aligned.  Refusals: smi_kmeans_fit's, and misaligned rows. */
int smi_l2_prepare(const void* src, int32_t src_dtype, int64_t rows, int32_t d, void* dst_f16, float* half_norms, void* stream);
int64_t smi_l2_topk_ws_bytes(int64_t nx, int64_t ny, int32_t k, int32_t d);
int smi_l2_topk(const void* x_f16, int64_t nx, const void* y_f16, int64_t ny, int32_t d, int32_t k, int64_t y_index_offset,
                const float* y_bias, int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, void* stream);
int smi_l2_slot_bias(const int32_t* list_ids, int64_t slots, const float* half_norms, float* out, void* stream);
int64_t smi_l2_flat_search_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d);
int smi_l2_flat_search(const void* q_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                       const float* list_bias, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k,
                       int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, void* stream);
int smi_l2_kmeans_finalize(const int64_t* sums, const int32_t* counts, int64_t K, int32_t d, float* centroids_f32,
                           void* centroids_f16, float* centroid_half_norms, int32_t* empty_count, void* stream);
int64_t smi_l2_kmeans_fit_ws_bytes(int64_t n, int64_t K, int32_t d);
int smi_l2_kmeans_fit(const void* x_f16, int64_t n, int32_t d, int64_t K, int32_t n_iter, int32_t resume, float* centroids_f32,
                      void* centroids_f16, float* centroid_half_norms, int32_t* labels, float* scores, int64_t* sums,
                      int32_t* counts, double* objective, int32_t* moved, int32_t* empty, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* L2 search over the product-quantised lists, plain and residual (restated in tests/ivf_pq_l2_ref.py).  The
 * row a slot stands for is what its codes decode to: y^ = smi_pq_decode of the codes (plain), or y^ = c + r^ with c the fp16
 * Euclidean centroid of the slot's list and r^ the decoded fp16 residual (residual; FAISS's IVFx,PQy with METRIC_L2 and
 * by_residual).  The nearest row has the largest q . y^ - 1/2 ||y^||^2, and
 *   q . y^ - 1/2 ||y^||^2 = (q . c - 1/2 ||c||^2) + q . r^ - (c . r^ + 1/2 ||r^||^2).
 * THE SCORE CONTRACT.  acc = the fp32 sum smi_ivf_pq_search produces for (query, decoded codes): the bits of smi_ivf_search
 * on the decoded row.
 *   plain     bias = -fl32(1/2 ||y^||^2): the half norm of the decoded row in smi_l2_prepare's fp64 order, negated -- the bits
 *             of -half_norms of smi_l2_prepare(smi_pq_decode(codes)).             score = fl32(acc + bias)
 *   residual  bias = -fl32(S1 + S2), S1 = sum_j c_j r^_j, S2 = 1/2 sum_j r^_j r^_j: each an fp64 sum of exact products in
 *             smi_l2_prepare's lane, chunk and xor order (S2 halved exactly), joined by ONE fp64 add, rounded to fp32 once.
 *             coarse = the biased score smi_l2_topk returns for the query against the list's centroid, q . c - 1/2 ||c||^2.
 *                                                                                 score = fl32(fl32(acc + bias) + coarse)
 *   both      ||q - y^||^2 = 2 (1/2 ||q||^2 - score).  A zero score is +0.  A pad slot has bias 0 and stays out by its id < 0,
 *             whatever its bias.  On integer-valued operands every term is a multiple of 1/2 and, while below 2^24, exact:
 *             the score is then exact and the distance the exact squared distance to the reconstructed row.
 * smi_l2_pq_bias: out[i] (fp32 [n]) = the bias of item i of codes (uint8 [n, d / dsub]) against codebooks (fp16
 *   [d / dsub][256][dsub], 16-byte aligned), one wave per item, no n x d temporary.  slot_ids (int32 [n], or NULL): the items
 *   are the slots of a storage and an item whose id is below 0 gets 0 (its codes are not read).  centroids NULL: the plain
 *   bias (labels and list_offsets must be NULL).  centroids (fp16 [K, d], 16-byte aligned): the residual bias against the
 *   centroid of the item's list, which is labels[i] (int32 [n]: the stand-alone form over encoded rows) or the list whose
 *   range of list_offsets (int32 [K + 1], with slot_ids) holds slot i -- exactly one of the two; a list number outside [0, K)
 *   means no centroid (c = 0).  One device function serves both forms, so the bias of a row does not depend on the form.
 *   Refusals: null codes / out, empty n, d not a multiple of 64, dsub, null or misaligned codebooks or centroids, K, labels
 *   or list_offsets without centroids, neither or both of them with centroids, list_offsets without slot_ids.
 * smi_l2_pq_search / smi_l2_pq_search_residual: smi_ivf_pq_search / smi_ivf_pq_search_residual with list_bias (fp32
 *   [capacity_slots], 16-byte aligned, from smi_l2_pq_bias) behind codebooks, on prepared queries (smi_l2_prepare) and the
 *   score above; everything else -- order, fill, unit rule, probes that name no list (their coarse entry is not read), pad
 *   slots, a row mask as ids of -1, the workspace (smi_l2_pq_search_ws_bytes = smi_ivf_pq_search_workspace_bytes) -- is
 *   theirs.  There are no keyed twins.  Refusals: smi_l2_flat_search's, and dsub, null or misaligned codebooks, a null or
 *   misaligned list_bias, a null coarse.  Nothing is read back or allocated: capturable. */
int smi_l2_pq_bias(const void* codes, int64_t n, int32_t d, int32_t dsub, const void* codebooks, const int32_t* slot_ids,
                   const int32_t* list_offsets, const int32_t* labels, const void* centroids, int64_t K, float* out,
                   void* stream);
int64_t smi_l2_pq_search_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d, int32_t dsub);
int smi_l2_pq_search(const void* q_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_codes,
                     int32_t dsub, const void* codebooks, const float* list_bias, const int32_t* list_ids,
                     const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* workspace,
                     int64_t workspace_bytes, void* stream);
int smi_l2_pq_search_residual(const void* q_f16, int64_t nq, int32_t d, const int32_t* probes, const float* coarse,
                              int32_t nprobe, const void* list_codes, int32_t dsub, const void* codebooks, const float* list_bias,
                              const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx,
                              float* score, void* workspace, int64_t workspace_bytes, void* stream);

/* k-way merge of `parts` per-shard top-k lists (device fp32 / int32 [parts, n, k], each sorted as
 * smi_xsim_topk returns them) into the k best of their union, same total order (score desc, index asc).
 * Folds the per-rank partial y-side neighbour lists of the sharded margin scoring; part_idx /
 * out_idx may be NULL when only the scores are needed (the margin uses the neighbour MEAN). */
int smi_xsim_merge_topk(const float* part_scores, const int32_t* part_idx, int32_t parts, int64_t n, int32_t k,
                        float* out_scores, int32_t* out_idx, void* stream);

/* Margin re-scoring of the k-NN candidates, LASER's xsim (facebookresearch/LASER source/xsim.py,
 * _score_margin / _score_knn; un-vendored, restated in oracle/xsim.py):
 *   score(i, j) = margin(cos(x_i, y_j), (mean_k cos(x_i, NN_k(x_i)) + mean_k cos(y_j, NN_k(y_j))) / 2)
 * fwd_scores / fwd_idx: device [nx, k] from smi_xsim_topk(X, Y, k) (indices into the rows of bwd_scores);
 * bwd_scores: device [ny, k] from smi_xsim_topk(Y, X, k) (or its cross-rank merge).  pred_idx[i] = the
 * candidate with the best score (first on ties), pred_margin[i] (nullable) its score; err_count (nullable,
 * device int32, ACCUMULATED) += #rows with pred_idx[i] != i + x_index_offset (aligned pairs). */
#define SMI_MARGIN_RATIO 0    /* a / b */
#define SMI_MARGIN_DISTANCE 1 /* a - b */
#define SMI_MARGIN_COSINE 2   /* a (bwd_scores unused) */
int smi_xsim_margin_select(const float* fwd_scores, const int32_t* fwd_idx, int64_t nx, int32_t k,
                           const float* bwd_scores, int64_t ny, int32_t margin, int64_t x_index_offset,
                           int32_t* pred_idx, float* pred_margin, int32_t* err_count, void* stream);

/* Bitext mining, LASER's mine_bitexts.py (facebookresearch/LASER source/mine_bitexts.py; un-vendored, the algorithm is
 * restated in DESIGN.md 3.13 and, loop for loop, in tests/mining_ref.py).
 *
 * smi_xsim_pair_scores: the margin score of m GIVEN pairs (LASER's --mode score),
 *   out[p] = margin(cos(x_s, y_t), (mean(fwd_scores[s]) + mean(bwd_scores[t])) / 2),  s = src_idx[p], t = trg_idx[p],
 *   with the cosine computed from row s of xn and row t of yn (matrices from smi_xsim_normalize; every d smi_xsim_topk
 *   accepts) and the means in smi_xsim_margin_select's arithmetic.  src_idx / trg_idx: device int64 [m]; fwd_scores
 *   [nx, k] / bwd_scores [ny, k] as for smi_xsim_margin_select, NULL allowed only for SMI_MARGIN_COSINE.  A pair with an
 *   index outside [0, nx) / [0, ny) scores NaN and reads nothing.
 *
 * smi_xsim_mine: the retrieval step (LASER's --mode mine) over the best candidates of both directions,
 *   fwd_best / fwd_score [nx] = smi_xsim_margin_select(fwd lists, bwd scores), bwd_best / bwd_score [ny] = the same call
 *   with the roles swapped.  Candidate c < nx is (c, fwd_best[c], fwd_score[c]), candidate c >= nx is
 *   (bwd_best[c - nx], c - nx, bwd_score[c - nx]).  A candidate with a NaN score or with its source / target outside
 *   [0, nx) / [0, ny) is excluded: never returned, never blocking another, nothing read or written at that index.
 *     SMI_MINE_FWD        the forward candidates                                  (capacity nx; bwd_* may be NULL)
 *     SMI_MINE_BWD        the backward candidates                                 (capacity ny; fwd_* may be NULL)
 *     SMI_MINE_INTERSECT  forward candidates with bwd_best[fwd_best[i]] == i      (capacity nx; bwd_score may be NULL)
 *     SMI_MINE_MAX        walk all nx + ny candidates by (score descending, -0 = +0, candidate number ascending) and
 *                         accept one iff neither its source nor its target belongs to an accepted one (capacity min(nx, ny))
 *   threshold: only pairs with score > threshold (strict) are returned; -INFINITY = no threshold (every non-excluded pair,
 *   a score of -inf included).  What SMI_MINE_MAX accepts does not depend on it.  out_src / out_trg (int32) / out_score
 *   receive the pairs in CANDIDATE ORDER (not by score), *out_count (device int32) their number; entries past the count
 *   are not written.  workspace: smi_xsim_mine_workspace_bytes() bytes of device memory, 8-byte aligned; a smaller buffer
 *   is refused before any launch.  nx + ny must fit int32.
 *   SMI_MINE_MAX BLOCKS ON `stream`: it runs as data-dependent rounds (typically a handful, in principle up to min(nx, ny)) and
 *   the host reads one int32 back after each, so it cannot be captured into a graph.  The other retrievals are
 *   asynchronous like the rest of this section. */
#define SMI_MINE_FWD 0
#define SMI_MINE_BWD 1
#define SMI_MINE_INTERSECT 2
#define SMI_MINE_MAX 3
int smi_xsim_pair_scores(const void* xn_f16, int64_t nx, const void* yn_f16, int64_t ny, int32_t d,
                         const int64_t* src_idx, const int64_t* trg_idx, int64_t m, const float* fwd_scores,
                         const float* bwd_scores, int32_t k, int32_t margin, float* out, void* stream);
int64_t smi_xsim_mine_workspace_bytes(int64_t nx, int64_t ny, int32_t retrieval);
int smi_xsim_mine(const int32_t* fwd_best, const float* fwd_score, int64_t nx, const int32_t* bwd_best,
                  const float* bwd_score, int64_t ny, int32_t retrieval, float threshold, int32_t* out_src,
                  int32_t* out_trg, float* out_score, int32_t* out_count, void* workspace, int64_t workspace_bytes,
                  void* stream);

/* DTW alignment of two sentence-embedding sequences that are known to be translations of each other, in order -- the
 * application of the reference's examples/bilingual_document.ipynb (fastdtw over cosine distances; un-vendored, the
 * contract is restated in DESIGN.md 3.15 and, loop for loop, in tests/alignment_ref.py).  A ragged batch of n_pairs
 * document pairs: pair b is rows x_offsets[b] .. x_offsets[b+1] of X against rows y_offsets[b] .. y_offsets[b+1] of Y,
 * nx x ny cells.  All arithmetic fp32:
 *   D[0][0] = c[0][0];  D[i][j] = min(D[i-1][j], D[i][j-1], D[i-1][j-1]) + c[i][j]   (one rounding: the add)
 * over the predecessors that exist and are admissible; a tie goes to the first of up (i-1, j), left (i, j-1), diagonal
 * (i-1, j-1).  +inf costs mark forbidden cells; NaN costs are outside the contract.
 *   radius: 0 = the full matrix; r >= 1 = a Sakoe-Chiba band, cell (i, j) admissible iff
 *           |i (ny-1) - j (nx-1)| <= r max(nx-1, ny-1, 1)  (in int64); the DP visits only the steps the band reaches.
 *   path: int32 [sum over the non-empty pairs of (nx + ny - 1), 2]; pair b's entries start at the sum over the pairs before
 *         it and run from (0, 0) to (nx-1, ny-1) in ascending order, path_len[b] (int32) of them, pair-local indices; the
 *         rest of its nx + ny - 1 entries is scratch.  distance[b] (fp32) = D[nx-1][ny-1].  A pair with an empty side has
 *         path_len 0 and distance +inf and leaves the other pairs alone.
 *   offsets: int64 [n_pairs + 1], given TWICE: *_host (host memory: validated, sizes the launches) and the same values in
 *         device memory (what the kernels read) -- the entries copy nothing and read nothing back, so they are stream-ordered
 *         and can be captured into a graph.
 *   workspace: smi_dtw_workspace_bytes() bytes of device memory (enough for either entry), 8-byte aligned; the costs and the
 *         direction codes are kept for the full nx x ny matrix even under a band.  D is never stored.
 * smi_dtw_align_cost: the costs are given, device fp32, the pairs' row-major [nx, ny] blocks one after the other.
 * smi_dtw_align: c[i][j] = 1 - x_i . y_j from rows of smi_xsim_normalize (fp16; every d smi_xsim_topk accepts), the dot
 *   product one fp32 chain in ascending k, so a pair has the same bits alone or in any batch.
 * Refused before any launch: n_pairs < 1, a negative radius, negative or decreasing offsets, a workspace that is too small
 * or misaligned (SMI_ERR_INVALID_ARG); n_pairs > 65535, a pair with more than 2^31 - 1 cells or a side above 2^30, d not a
 * multiple of 64 (SMI_ERR_UNSUPPORTED).  One workgroup works on a pair: a single huge pair does not fill the chip. */
int64_t smi_dtw_workspace_bytes(int32_t n_pairs, const int64_t* x_offsets_host, const int64_t* y_offsets_host);
int smi_dtw_align_cost(const float* cost, int32_t n_pairs, const int64_t* x_offsets_host, const int64_t* y_offsets_host,
                       const int64_t* x_offsets, const int64_t* y_offsets, int64_t radius, int32_t* path,
                       int32_t* path_len, float* distance, void* workspace, int64_t workspace_bytes, void* stream);
int smi_dtw_align(const void* xn_f16, const void* yn_f16, int32_t d, int32_t n_pairs, const int64_t* x_offsets_host,
                  const int64_t* y_offsets_host, const int64_t* x_offsets, const int64_t* y_offsets, int64_t radius,
                  int32_t* path, int32_t* path_len, float* distance, void* workspace, int64_t workspace_bytes,
                  void* stream);

/* Spherical k-means over sentence embeddings (restated in tests/kmeans_ref.py).  Similarity is cosine, as
 * everywhere in this section: a row belongs to the nearest of K unit centroids, and a centroid is the normalised sum of its
 * members.  xn is a matrix from smi_xsim_normalize (fp16, smi_xsim_padded_rows(n) rows; the update reads the first n).
 *
 * smi_kmeans_update: sums[c][j] = sum over the rows i with labels[i] == c of xn[i][j] * 2^24, as an EXACT integer (every
 *   finite fp16 is a multiple of 2^-24), counts[c] = the number of such rows.  sums (int64 [K, d]) and counts (int32 [K]) are
 *   overwritten.  A row whose label is outside [0, K) is skipped: nothing is read or written through that label (the
 *   convention of smi_xsim_mine).  An Inf or NaN element contributes 0.  Integer sums do not depend on the order: the same
 *   bits for any permutation of the rows, any grid, any run.  The rows are bucketed by label and summed in registers by work
 *   units of SMI_KMEANS_UNIT_ROWS consecutive members; one cluster holding every row is spread over n / SMI_KMEANS_UNIT_ROWS
 *   units.
 * smi_kmeans_finalize: for a cluster with counts[c] > 0 and a sum that is not all zero,
 *   centroids_f32[c][j] = (float)sums[c][j] * 2^-24 (one round to nearest even, then an exact scale) and row c of
 *   centroids_f16 = what smi_xsim_normalize makes of that fp32 row (it is called, not restated).  Any other cluster keeps
 *   both of its rows as they were; *empty_count (device int32, overwritten) = the number of those.  centroids_f16 has
 *   smi_xsim_padded_rows(K) rows; the rows from K on are zeroed.
 * smi_kmeans_fit: the round loop on one stream, with no host read-back (it can be captured).
 *   resume = 0: centroids_f32 holds the K initial centroids; centroids_f16 = smi_xsim_normalize of them; every row is
 *     assigned (smi_xsim_topk, k = 1, unchanged: ties between equal centroids go to the lower index, so a duplicate centroid
 *     stays empty); then n_iter rounds of update -> finalise -> assign.  objective / moved get n_iter + 1 entries, empty
 *     n_iter.
 *   resume = 1: continues an earlier call on the same buffers (labels, centroids): n_iter rounds of update -> finalise ->
 *     assign, n_iter entries in each record.  fit(0) followed by T calls of fit(1, resume) equals fit(T) bit for bit.
 *   labels (int32 [n]) / scores (fp32 [n]) always belong to the returned centroids.  objective (fp64): the sum of the scores
 *   of an assignment, added in a fixed order; moved (int32): the rows whose label differs from the assignment before (n for
 *   the first one); empty (int32): smi_kmeans_finalize's count.  sums / counts: those of the last update.
 * workspace: device memory, 16-byte aligned.  update and finalise: smi_kmeans_workspace_bytes(n, K, d) bytes (finalise does
 *   not depend on n: any n >= 1).  fit: smi_kmeans_workspace_bytes(n, K, d) + smi_xsim_workspace_bytes(n, K, 1, d) + 4 n, each
 *   term rounded up to a multiple of 16, + 3072.  A smaller buffer is refused, not overrun.
 * Refused before any launch: a null pointer, n < 1, K < 1, n_iter < 0, a small or misaligned workspace
 *   (SMI_ERR_INVALID_ARG); d not a multiple of 64, n or K above 2^31 - 256 (SMI_ERR_UNSUPPORTED); for these shapes
 *   smi_kmeans_workspace_bytes returns 0. */
#define SMI_KMEANS_UNIT_ROWS 64
int64_t smi_kmeans_workspace_bytes(int64_t n, int64_t K, int32_t d);
int smi_kmeans_update(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, int64_t K, int64_t* sums,
                      int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int smi_kmeans_finalize(const int64_t* sums, const int32_t* counts, int64_t K, int32_t d, float* centroids_f32,
                        void* centroids_f16, int32_t* empty_count, void* workspace, int64_t workspace_bytes, void* stream);
int smi_kmeans_fit(const void* xn_f16, int64_t n, int32_t d, int64_t K, int32_t n_iter, int32_t resume,
                   float* centroids_f32, void* centroids_f16, int32_t* labels, float* scores, int64_t* sums,
                   int32_t* counts, double* objective, int32_t* moved, int32_t* empty, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* IVF-Flat index over sentence embeddings (restated in tests/ivf_ref.py).  K inverted lists over the n fp16
 * rows of a matrix from smi_xsim_normalize: a search scores a query against the rows of the lists it probes only, about
 * nprobe / K of smi_xsim_topk's work.  The coarse quantiser is not part of these entries: labels and probes are what
 * smi_xsim_topk against the centroids returns (k = 1 for the labels, k = nprobe for the probes).
 *
 * Storage, list-contiguous: list_rows fp16 [capacity_slots, d] (row copies), list_ids int32 [capacity_slots] (the original
 *   row number of every slot), list_offsets int32 [K + 1] (list c is the slots list_offsets[c] .. list_offsets[c + 1];
 *   list_offsets[K] = the slots in use), list_sizes int32 [K] (its rows).  Every list begins at a multiple of
 *   smi_ivf_list_align() = SMI_IVF_LIST_ALIGN slots (one 16-row block of the scan's MFMA) and is padded to that multiple
 *   with zero rows whose id is -1, so a 16-slot block of the scan never spans two lists.  smi_ivf_slots_bound(n, K) = the
 *   largest number of slots any labelling of n rows over K lists can need, min(n, K) * A + floor((n - min(n, K)) / A) * A.
 * smi_ivf_build: row i goes to list labels[i]; a label outside [0, K) leaves the row out of the index and nothing is
 *   addressed through it (smi_kmeans_update's convention).  The order of the rows inside a list depends on the arrival order
 *   of atomics; no search result depends on it.  The host has not seen the labels, so capacity_slots must cover every
 *   labelling: capacity_slots >= smi_ivf_slots_bound(n, K).  Slots from list_offsets[K] on are not written, except
 *   list_ids, which is -1 there.
 * smi_ivf_search: qn = normalised queries [smi_xsim_padded_rows(nq), d]; probes = device int32 [nq, nprobe], the lists
 *   each query scans; an entry outside [0, K) names no list.  idx [nq, k] / score [nq, k]: the k best rows of the probed
 *   lists in smi_xsim_topk's total order (score descending, ties to the lower ORIGINAL row number, across lists as inside
 *   them); (-1, -inf) where fewer than k candidates exist.  A score is the fp32 accumulation of the fp16 products in one
 *   fixed order over d (MFMA K slices ascending): its bits do not depend on the list the row is in, on its slot, on the
 *   other queries of the call or on their order.  A probe row that names one list twice (smi_xsim_topk never makes one)
 *   may return that list's rows twice.  Reads nothing back, allocates nothing; list_rows / list_ids / list_offsets must be
 *   what smi_ivf_build wrote (they are trusted, as device data is everywhere here).
 * workspace: device memory, 16-byte aligned, smi_ivf_build_workspace_bytes / smi_ivf_search_workspace_bytes bytes.
 * Refused before any launch: a null pointer, n / nq / K < 1, k or nprobe outside [1, 8], a small or misaligned workspace,
 *   capacity_slots below the bound (SMI_ERR_INVALID_ARG); d not a multiple of 64, n, K, nq * nprobe or the slots bound above
 *   2^31 - 256 (SMI_ERR_UNSUPPORTED).  For these shapes the sizing functions return 0.  One work unit of the scan is one
 *   list and SMI_IVF_UNIT_QUERIES of the queries that probe it (twice that where nq * nprobe >= 256 K; no bit of the result
 *   depends on it): a long list probed by few queries runs on few CUs. */
#define SMI_IVF_LIST_ALIGN 16
#define SMI_IVF_UNIT_QUERIES 64
int32_t smi_ivf_list_align(void);
int64_t smi_ivf_slots_bound(int64_t n, int64_t K);
int64_t smi_ivf_build_workspace_bytes(int64_t n, int64_t K, int32_t d);
int smi_ivf_build(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, int64_t K, void* list_rows,
                  int32_t* list_ids, int64_t capacity_slots, int32_t* list_offsets, int32_t* list_sizes, void* workspace,
                  int64_t workspace_bytes, void* stream);
int64_t smi_ivf_search_workspace_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d);
int smi_ivf_search(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                   const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* Regrouping of IVF storage: extend, remove and merge on the device (restated in tests/ivf_regroup_ref.py).
 * All five index kinds keep the storage of smi_ivf_build: payload rows of row_bytes bytes (fp16 rows, int8 codes, PQ codes),
 * one int32 id per slot and at most one 32-bit aux value per slot (the scales of the int8 lists, the bias of the L2 lists).
 * smi_lists_regroup writes FRESH storage of that layout from the surviving slots of a filled index and a set of new rows that
 * are already encoded (smi_ivf_i8_encode, smi_pq_encode, smi_pq_encode_residual; fp16 rows as they are).
 *
 * Survivors: old slot s survives iff old_ids[s] >= 0 (and s < old_offsets[K]).  old_ids may be the effective ids smi_slot_filter
 *   writes for a row mask: that is how rows are removed.  old_rows_bound = the caller's upper bound on the number of survivors,
 *   at most old_slots.
 * New rows: row i goes to list new_labels[i]; a label outside [0, K) leaves it out (smi_ivf_build's convention).  Its id is
 *   new_ids[i] where new_ids is given -- a given id below 0 leaves the row out too -- else new_id_base + i.
 * Output: list c holds the survivors of old list c and the new rows labelled c, each with its row_bytes payload bytes, its
 *   aux value (where the aux pointers are given) and its id, unchanged.  The layout is smi_ivf_build's: every list starts at a
 *   multiple of SMI_IVF_LIST_ALIGN, pad slots are zero bytes with aux 0 and id -1, list_sizes[c] = the rows of list c, and
 *   list_ids is -1 from list_offsets[K] to capacity_slots.  The order inside a list is unspecified, as in the build.
 *   capacity_slots >= smi_ivf_slots_bound(old_rows_bound + n_new, K): the host checks it without seeing device data.
 * No store leaves the caller's buffers whatever the device data say: destination slots are bounded by that slots bound and
 *   list numbers by K; were there more survivors than old_rows_bound, the rows beyond the bound are dropped.
 * row_bytes: any value from 1 up.  16-byte accesses where row_bytes % 16 == 0 and old_rows, new_rows and list_rows are
 *   16-byte aligned; byte accesses otherwise.
 * Empty sides: n_new = 0 (null new_*) is a pure compaction; old_slots = 0 (null old_*) is a build from encoded rows.
 * workspace: device memory, 16-byte aligned, smi_lists_regroup_ws_bytes(old_slots, n_new, K) bytes.  Nothing is read back or
 *   allocated: the call can be captured in a graph.
 * Refused before any launch: a null output pointer, a null input on a side that has rows, K < 1, both sides empty, a negative
 *   count, row_bytes < 1, old_rows_bound outside [0, old_slots], aux pointers given on some sides that have rows and not on
 *   others (list_aux counts as a side), an output pointer equal to an input pointer, capacity_slots below the bound, a small
 *   or misaligned workspace (SMI_ERR_INVALID_ARG); old_slots + n_new, K, new_id_base + n_new or the slots bound above
 *   2^31 - 256, new_id_base < 0 (SMI_ERR_UNSUPPORTED).  The sizing function returns 0 for a refused shape. */
int64_t smi_lists_regroup_ws_bytes(int64_t old_slots, int64_t n_new, int64_t K);
int smi_lists_regroup(const void* old_rows, const float* old_aux, const int32_t* old_ids, const int32_t* old_offsets,
                    int64_t old_slots, int64_t old_rows_bound, const void* new_rows, const float* new_aux,
                    const int32_t* new_labels, const int32_t* new_ids, int32_t new_id_base, int64_t n_new, int32_t row_bytes,
                    int64_t K, void* list_rows, float* list_aux, int32_t* list_ids, int64_t capacity_slots,
                    int32_t* list_offsets, int32_t* list_sizes, void* workspace, int64_t workspace_bytes, void* stream);

/* A page of the flat search (the contract of a page: smi_xsim_topk_page): the arguments of smi_ivf_search and,
 * BEHIND them as the keyed twins take theirs, the ceilings ceil_score fp32 / ceil_idx int32 [nq], null for none -- ONE ceiling per query, shared by its probes: the result
 * is the k <= 16 best rows strictly after the ceiling over all the lists the query probes, in smi_ivf_search's order, layout
 * and score bits (a zero score as +0).  nprobe in [1, 64].  list_ids may be the effective ids of a row mask (3.24).  workspace:
 * smi_ivf_search_page_ws_bytes(nq, K, nprobe, k, d) bytes, 16-byte aligned.  Refused before any launch: what
 * smi_ivf_search refuses, with k outside [1, 16] and nprobe outside [1, 64] in place of its limits, and one ceiling array
 * without the other; the sizing call returns 0 for a refused shape.  Nothing is read back or allocated. */
int64_t smi_ivf_search_page_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d);
int smi_ivf_search_page(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe, const void* list_rows,
                        const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score,
                        void* workspace, int64_t workspace_bytes, void* stream, const float* ceil_score,
                        const int32_t* ceil_idx);

/* Range search over the IVF-Flat lists (restated in tests/ivf_range_ref.py): EVERY row of the lists a query
 * probes whose score is at least the query's threshold, where smi_ivf_search returns the k <= 8 best.  How many rows that
 * is is known only after the lists were walked, so there are two calls and the caller sizes the output between them.
 *
 * Inputs of both calls: qn, nq, d, probes, nprobe in [1, 8], list_rows, list_ids, list_offsets, K are smi_ivf_search's (an
 *   entry of probes outside [0, K) names no list; a list named twice contributes its rows twice); threshold = device fp32
 *   [nq].  Pair q * nprobe + p is query q against the list probes[q, p].
 * Hit: row i of a probed list is a hit of query q iff score(q, i) >= threshold[q], an fp32 compare: a NaN threshold gives
 *   no hit, -inf every row of the probed lists.  The score has the bits smi_ivf_search returns for the same two rows; pad
 *   slots are never hits.
 * smi_range_search_count: inverts the probe table into the workspace and writes pair_counts int32 [nq * nprobe], the hits
 *   of every pair (0 for a pair that names no list).  No atomics on global memory: the counts do not depend on the run.
 * smi_range_search_emit: pair_base = device int64 [nq * nprobe + 1], the exclusive prefix sum of pair_counts, its last entry
 *   = total (also passed by value); score fp32 [total] / idx int32 [total]: the hits of pair j are the entries pair_base[j]
 *   .. pair_base[j + 1], in no specified order, so those of query q are pair_base[q * nprobe] .. pair_base[(q + 1) * nprobe].
 *   NEEDS THE WORKSPACE AS smi_range_search_count LEFT IT, and the same inputs: it does not invert the probe table again.
 *   A pair that has more hits than its segment holds (thresholds lowered between the calls) loses the surplus: nothing is
 *   written outside [pair_base[j], min(pair_base[j + 1], total)).  With fewer hits the segment's tail is not written.
 * Neither call reads anything back or allocates; one work unit is smi_ivf_search's (no bit of the result depends on its size).
 * workspace: device memory, 16-byte aligned, smi_range_search_ws_bytes bytes.
 * Refused before any launch: a null pointer, nq / K < 1, nprobe outside [1, 8], a small or misaligned workspace, total < 0
 *   (SMI_ERR_INVALID_ARG); d not a multiple of 64, nq, K or nq * nprobe above 2^31 - 256 (SMI_ERR_UNSUPPORTED).  For these
 *   shapes the sizing function returns 0. */
int64_t smi_range_search_ws_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t d);
int smi_range_search_count(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                           const float* threshold, const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets,
                           int64_t K, int32_t* pair_counts, void* workspace, int64_t workspace_bytes, void* stream);
int smi_range_search_emit(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                          const float* threshold, const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets,
                          int64_t K, const int64_t* pair_base, int64_t total, float* score, int32_t* idx, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* Filtered search over the IVF lists (restated in tests/ivf_filter_ref.py): a candidate (query q, row i)
 * counts iff the row is VISIBLE (a row mask shared by all queries of a call) and the pair passes the KEY PREDICATE: every row
 * has a signed int32 key, every query one, and `row key REL query key` holds for the relation of the call.  Everything else is
 * the contract of the unfiltered entry: a query's filtered result is, bit for bit, the unfiltered result over lists that hold
 * only the rows this query may see.
 *
 * smi_slot_filter: the filter in slot order, once per filter and reusable: slot_ids_out int32 [slots] = list_ids[slot] where
 *   the row is visible (row_mask null, or row_mask[id] != 0; one byte per row), else -1; slot_keys_out int32 [slots] =
 *   row_keys[id], 0 where the slot holds no visible row.  row_keys / row_mask = device [n], either may be null, not both;
 *   row_keys and slot_keys_out go together.  An id outside [0, n) is treated as masked out and never read.  slots = the
 *   slots of the storage (list_ids' length); slots from list_offsets[K] on get id -1.  Both outputs 16-byte aligned.
 *   Enqueued; nothing is read back.  THE MASK NEEDS NO OTHER ENTRY: every scan skips a slot whose id is -1, so the unfiltered
 *   entries run on slot_ids_out in place of list_ids.
 * smi_*_keyed: the entry of the same name with the key predicate.  The arguments of the twin (list_ids may be slot_ids_out),
 *   then slot_keys = device int32 [slots], 16-byte aligned (the key of a slot whose id is -1 is never looked at), query_keys =
 *   device int32 [nq], accept = the relation as a 3-bit mask over the outcome of ONE signed compare of the row's key with the
 *   query's: bit 0 less, bit 1 equal, bit 2 greater -- == 2, != 5, < 1, <= 3, > 4, >= 6; 0 lets nothing pass, 7 everything
 *   (the twin's result, bit for bit).  Workspace: the twin's sizing function.  smi_range_search_emit_keyed needs the workspace
 *   as smi_range_search_count_keyed left it and the same keys.
 * Refused before any launch: what the twin refuses, in its order and words; behind its null-pointer check a null slot_keys or
 *   query_keys, slot_keys not 16-byte aligned, accept outside [0, 7] (SMI_ERR_INVALID_ARG). */
int smi_slot_filter(const int32_t* list_ids, const int32_t* list_offsets, int64_t K, const int32_t* row_keys,
                    const uint8_t* row_mask, int64_t n, int32_t* slot_ids_out, int32_t* slot_keys_out, int64_t slots,
                    void* stream);
int smi_ivf_search_keyed(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                         const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k,
                         int32_t* idx, float* score, void* workspace, int64_t workspace_bytes, void* stream,
                         const int32_t* slot_keys, const int32_t* query_keys, int32_t accept);
int smi_ivf_i8_search_keyed(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                            const void* list_codes, const float* list_scales, const int32_t* list_ids,
                            const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* workspace,
                            int64_t workspace_bytes, void* stream, const int32_t* slot_keys, const int32_t* query_keys,
                            int32_t accept);
int smi_ivf_pq_search_keyed(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                            const void* list_codes, int32_t dsub, const void* codebooks_f16, const int32_t* list_ids,
                            const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* workspace,
                            int64_t workspace_bytes, void* stream, const int32_t* slot_keys, const int32_t* query_keys,
                            int32_t accept);
int smi_ivf_pq_search_residual_keyed(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, const float* coarse,
                                     int32_t nprobe, const void* list_codes, int32_t dsub, const void* codebooks_f16,
                                     const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx,
                                     float* score, void* workspace, int64_t workspace_bytes, void* stream,
                                     const int32_t* slot_keys, const int32_t* query_keys, int32_t accept);
int smi_range_search_count_keyed(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                                 const float* threshold, const void* list_rows, const int32_t* list_ids,
                                 const int32_t* list_offsets, int64_t K, int32_t* pair_counts, void* workspace,
                                 int64_t workspace_bytes, void* stream, const int32_t* slot_keys, const int32_t* query_keys,
                                 int32_t accept);
int smi_range_search_emit_keyed(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                                const float* threshold, const void* list_rows, const int32_t* list_ids,
                                const int32_t* list_offsets, int64_t K, const int64_t* pair_base, int64_t total, float* score,
                                int32_t* idx, void* workspace, int64_t workspace_bytes, void* stream, const int32_t* slot_keys,
                                const int32_t* query_keys, int32_t accept);

/* Semantic de-duplication over the IVF-Flat lists (restated in tests/dedup_ref.py): the per-list self-join of
 * SemDeDup (Abbas et al. 2023).  For every row, the best score against the rows of its own list that PRECEDE it in a keep
 * order; a caller thresholds it (keep = !(max_sim > threshold), strict) and may sweep the threshold over one stored result.
 *
 * Input: the storage smi_ivf_build wrote, unchanged: list_rows fp16 [slots, d], list_ids int32 [slots] (-1 = pad or unused
 *   slot), list_offsets int32 [K + 1].  n = the number of original rows; ids lie in [0, n).  priority = device fp32 [n]
 *   indexed by ORIGINAL row number, or NULL: every priority compares equal.  NaN priorities are outside the contract.
 * Precedence: row j precedes row i iff both are in the same list and (priority[j] > priority[i] or (priority[j] ==
 *   priority[i] and j < i)).  A row never precedes itself; with no priority this reads "keep the first occurrence".
 * Output, indexed by original row number and pre-filled on the device: max_sim fp32 [n] = the best score of row i against
 *   the rows that precede it, -inf if none does (also for a row that is in no list); nearest int32 [n] = the id of that row,
 *   or -1.  "Best" is smi_xsim_topk's total order: score descending, ties to the lower original id.
 * Score: what smi_ivf_search returns for the same two rows (fp32 accumulation of the fp16 products, MFMA K slices
 *   ascending).  Its bits depend on the two rows alone -- not on the list, the slot, the tile shape, the unit size, the order
 *   of the corpus or the run -- and the score of (i, j) has the bits of the score of (j, i).
 * A row is compared with its own list only.  One work unit is one list and 64 consecutive slots of it (128 where n >= 256 K;
 *   no bit depends on it) and walks the whole list: a very long list costs its size squared, on size / unit CUs.
 * Reads nothing back, allocates nothing, is capturable.  workspace: device memory, 16-byte aligned,
 *   smi_ivf_dedup_workspace_bytes bytes.
 * Refused before any launch: a null pointer except priority, n / K / slots < 1, slots not a multiple of SMI_IVF_LIST_ALIGN, a
 *   small or misaligned workspace (SMI_ERR_INVALID_ARG); d not a multiple of 64, n, K or slots above 2^31 - 256
 *   (SMI_ERR_UNSUPPORTED).  For these shapes the sizing function returns 0. */
int64_t smi_ivf_dedup_workspace_bytes(int64_t slots, int64_t n, int64_t K, int32_t d);
int smi_ivf_dedup(const void* list_rows, const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int64_t slots,
                  int32_t d, const float* priority_or_null, int64_t n, float* max_sim, int32_t* nearest, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* IVF index with int8 scalar-quantised rows (restated in tests/ivf_i8_ref.py).  The lists of smi_ivf_build
 * with one signed byte per element and one fp32 scale per row, half the bytes of the fp16 copies, scanned with an integer
 * MFMA (v_mfma_i32_16x16x64_i8) whose int32 sums are exact, so a score is specified down to its bits for ANY data.
 *
 * Encoding of one fp16 row x of length d (per-row symmetric; non-finite elements are outside the contract):
 *   amax = max_j |x_j|;  inv = 127.0f / amax and scale = amax / 127.0f, both correctly rounded fp32 divisions;
 *   code_j = clamp(rint(fl32(x_j * inv)), -127, 127), ties to even.  A zero row has all codes 0 and scale 0.
 * Score of a query row (cq, scale_q) against a stored row (cx, scale_x):
 *   acc = sum_j cq_j * cx_j in int32 (exact: |acc| <= 127^2 d);  score = fl32(fl32((float)acc * scale_x) * scale_q), an
 *   int -> fp32 conversion to nearest even and two fp32 multiplies in that order.  Its bits depend on the two fp16 rows
 *   alone: not on the list, the slot, the tile shape, the unit size, the other queries of the call or the run.
 * smi_ivf_i8_encode: codes int8 [n, d] and scales fp32 [n] of the first n rows of xn (fp16 [>= n, d]).  The row quantiser on
 *   its own; smi_ivf_i8_build and smi_ivf_i8_search (for the queries) call the same device function.
 * Storage: smi_ivf_build's layout with list_codes int8 [capacity_slots, d] in place of list_rows and a new list_scales fp32
 *   [capacity_slots]; the same SMI_IVF_LIST_ALIGN and the same smi_ivf_slots_bound.  Pad slots have zero codes, scale 0 and
 *   id -1.  Slots from list_offsets[K] on are not written, except list_ids, which is -1 there.
 * smi_ivf_i8_build: smi_ivf_build's bucketing (labels outside [0, K) leave the row out), then one wave per slot encodes the
 *   row list_ids[slot] names.
 * smi_ivf_i8_search: encodes the first nq rows of qn into the workspace, then inverts the probe table, scans and merges as
 *   smi_ivf_search does.  idx / score: smi_ivf_search's layout, total order (score descending, ties to the lower ORIGINAL row
 *   number, across lists as inside them) and (-1, -inf) fill.  Reads nothing back, allocates nothing.
 * workspace: device memory, 16-byte aligned, smi_ivf_i8_build_workspace_bytes / smi_ivf_i8_search_workspace_bytes bytes.
 * Refused before any launch: what smi_ivf_build / smi_ivf_search refuse, with the same codes, and d > SMI_IVF_I8_MAX_DIM
 *   (SMI_ERR_UNSUPPORTED: the int32 sum could overflow).  For these shapes the sizing functions return 0.  The unit-size rule
 *   is smi_ivf_search's. */
#define SMI_IVF_I8_MAX_DIM 131072
int smi_ivf_i8_encode(const void* xn_f16, int64_t n, int32_t d, void* codes, float* scales, void* stream);
int64_t smi_ivf_i8_build_workspace_bytes(int64_t n, int64_t K, int32_t d);
int smi_ivf_i8_build(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, int64_t K, void* list_codes,
                     float* list_scales, int32_t* list_ids, int64_t capacity_slots, int32_t* list_offsets,
                     int32_t* list_sizes, void* workspace, int64_t workspace_bytes, void* stream);
int64_t smi_ivf_i8_search_workspace_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d);
int smi_ivf_i8_search(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                      const void* list_codes, const float* list_scales, const int32_t* list_ids,
                      const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* Product quantiser and IVF index with product-quantised rows (restated in tests/ivf_pq_ref.py).
 * d = M * dsub: M sub-quantisers over dsub in {8, 16, 32, 64} dimensions each, always 256 codewords, so a code is one byte
 * and a row M bytes (128 / 64 / 32 / 16 at d = 1024).  codebooks: fp16 [M][256][dsub], 16-byte aligned; codes: uint8 [n][M].
 *
 * Encoding of subvector x (the fp16 x[m dsub .. (m + 1) dsub) of a row) against codeword c (fp16 [dsub]), all in fp32:
 *   n2 = ((0 + c_0 c_0) + c_1 c_1) + ... ascending;  bias = -0.5f * n2 (exact);
 *   key = fmaf(x_{dsub-1}, c_{dsub-1}, ... fmaf(x_0, c_0, bias)), one chain ascending in j;
 *   code_m = the c with the largest key, ties to the lower code: the Euclidean nearest codeword.  A product of two fp16 is
 *   exact in fp32, so every step is one rounding of an exact sum.  Non-finite input is outside the contract.
 * smi_pq_encode: codes of the first n rows of xn (fp16 [>= n, d]).  smi_pq_train (every round) and smi_ivf_pq_build call
 *   the same device function: a row has the same codes wherever it is encoded.
 * smi_pq_decode: rows fp16 [n, d] (16-byte aligned), row r = the concatenation of the M codewords codes[r] names.
 * smi_pq_train: Lloyd rounds on the first n rows of xn.  init = device int32 [256], row numbers in [0, n) (trusted):
 *   codeword c of every sub-quantiser starts as that subvector of row init[c].  A round encodes all rows, forms
 *   S[m][c][j] = sum over the members of x_j * 2^24 as int64 (exact in any order; needs n * max|x| * 2^24 < 2^63, always
 *   true for rows of smi_xsim_normalize) and count[m][c], then c_j = fp16_rn(fdiv_rn((float)S, (float)count) * 2^-24), the
 *   int64 -> fp32 conversion, the division and the fp16 conversion to nearest even; a codeword with no member keeps its
 *   value.  n_iter >= 0 rounds (0: the start), all enqueued on the stream, no read-back, integer atomics only: one init
 *   gives one result bit for bit.
 * Storage of the index: smi_ivf_build's layout with list_codes uint8 [capacity_slots, M] in place of list_rows; the same
 *   SMI_IVF_LIST_ALIGN and smi_ivf_slots_bound.  A pad slot has id -1 and all codes 0.  Slots from list_offsets[K] on are
 *   not written, except list_ids, which is -1 there.
 * smi_ivf_pq_build: smi_ivf_build's bucketing, then one wave per slot encodes the row list_ids[slot] names.
 * smi_ivf_pq_search: inverts the probe table, scans and merges as smi_ivf_search does; the scan decodes every tile's codes
 *   into the flat scan's fp16 LDS image once per tile and K slice.  Score: the fp32 accumulation, in MFMA K steps of 32
 *   ascending, of the fp16 query row against the fp16 decoded row -- the bits smi_ivf_search returns for that query against
 *   smi_pq_decode of the row, whatever the list, slot, unit size, company or run.  idx / score: smi_ivf_search's layout,
 *   total order and (-1, -inf) fill.  Reads nothing back, allocates nothing.
 * workspace: device memory, 16-byte aligned, of the size the matching *_workspace_bytes function returns.
 * Refused before any launch: what smi_ivf_build / smi_ivf_search refuse, with the same codes; dsub outside {8, 16, 32, 64}
 *   or not dividing d (SMI_ERR_UNSUPPORTED); null or misaligned codebooks, n_iter < 0 (SMI_ERR_INVALID_ARG).  For these
 *   shapes the sizing functions return 0. */
int smi_pq_encode(const void* xn_f16, int64_t n, int32_t d, int32_t dsub, const void* codebooks_f16, void* codes,
                  void* stream);
int smi_pq_decode(const void* codes, int64_t n, int32_t d, int32_t dsub, const void* codebooks_f16, void* rows_f16,
                  void* stream);
int64_t smi_pq_train_workspace_bytes(int64_t n, int32_t d, int32_t dsub);
int smi_pq_train(const void* xn_f16, int64_t n, int32_t d, int32_t dsub, const int32_t* init_rows, int32_t n_iter,
                 void* codebooks_f16, void* workspace, int64_t workspace_bytes, void* stream);
int64_t smi_ivf_pq_build_workspace_bytes(int64_t n, int64_t K, int32_t d, int32_t dsub);
int smi_ivf_pq_build(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, int64_t K, int32_t dsub,
                     const void* codebooks_f16, void* list_codes, int32_t* list_ids, int64_t capacity_slots,
                     int32_t* list_offsets, int32_t* list_sizes, void* workspace, int64_t workspace_bytes, void* stream);
int64_t smi_ivf_pq_search_workspace_bytes(int64_t nq, int64_t K, int32_t nprobe, int32_t k, int32_t d, int32_t dsub);
int smi_ivf_pq_search(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, int32_t nprobe,
                      const void* list_codes, int32_t dsub, const void* codebooks_f16, const int32_t* list_ids,
                      const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx, float* score, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* Residual encoding against the list centroid for the IVF-PQ index (restated in
 * tests/ivf_pq_residual_ref.py): FAISS's `by_residual`.  A row is product-quantised as its difference from the centroid of
 * its list, so the codewords describe only what the coarse quantiser has not already said.
 *
 * centroids: the fp16 normalised centroid table [K, d], 16-byte aligned.  Residual of row i with label l in [0, K):
 *   r_i[j] = fp16_rn(fp32_rn((float)x_i[j] - (float)c[l][j])), two roundings to nearest even.  A label outside [0, K) addresses
 *   nothing: the residual is the row itself.  A residual is fp16, a multiple of 2^-24 with |r| <= 2 for normalised operands,
 *   so the exact int64 training sums of smi_pq_train and their range condition carry over.
 * Codes, codebooks, decode: those of the plain quantiser applied to r instead of x -- the same key chain, ties, finalise
 *   rounding and start (codeword c = that subvector of the RESIDUAL of row init[c]).  A row's codes depend on its label.
 * smi_pq_residuals: out fp16 [n, d] (16-byte aligned) = the residuals of the first n rows of xn, labels int32 [n].  The other
 *   entries form the same element inside their kernels and keep no n x d temporary; this one is what they are tested against.
 * smi_pq_encode_residual / smi_pq_train_residual / smi_ivf_pq_build_residual: smi_pq_encode / smi_pq_train /
 *   smi_ivf_pq_build on the residuals; labels int32 [n] (of the build: the labels it buckets by).  Storage, byte for byte, and
 *   workspaces are the plain index's: size them with smi_pq_train_workspace_bytes / smi_ivf_pq_build_workspace_bytes.
 * smi_ivf_pq_search_residual: smi_ivf_pq_search with coarse = device fp32 [nq, nprobe], the score of query q against the
 *   centroid of the list probes[q][p] names.  score = fl32(acc + coarse[q][p]), acc = smi_ivf_pq_search's score against the
 *   decoded residual row: one fp32 add is the whole difference.  Total order, (-1, -inf) fill and merge are unchanged; nothing
 *   is added to an empty entry; a probe entry outside [0, K) names no list and its coarse entry is not read.  Non-finite
 *   coarse is outside the contract.  Workspace: smi_ivf_pq_search_workspace_bytes.
 * Refused before any launch: what the plain entries refuse, with the same codes; null labels / coarse, null or misaligned
 *   centroids / out, K < 1 (SMI_ERR_INVALID_ARG); K above 2^31 - 256 (SMI_ERR_UNSUPPORTED). */
int smi_pq_residuals(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, const void* centroids_f16, int64_t K,
                     void* out_f16, void* stream);
int smi_pq_encode_residual(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, const void* centroids_f16,
                           int64_t K, int32_t dsub, const void* codebooks_f16, void* codes, void* stream);
int smi_pq_train_residual(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, const void* centroids_f16,
                          int64_t K, int32_t dsub, const int32_t* init_rows, int32_t n_iter, void* codebooks_f16,
                          void* workspace, int64_t workspace_bytes, void* stream);
int smi_ivf_pq_build_residual(const void* xn_f16, const int32_t* labels, int64_t n, int32_t d, int64_t K,
                              const void* centroids_f16, int32_t dsub, const void* codebooks_f16, void* list_codes,
                              int32_t* list_ids, int64_t capacity_slots, int32_t* list_offsets, int32_t* list_sizes,
                              void* workspace, int64_t workspace_bytes, void* stream);
int smi_ivf_pq_search_residual(const void* qn_f16, int64_t nq, int32_t d, const int32_t* probes, const float* coarse,
                               int32_t nprobe, const void* list_codes, int32_t dsub, const void* codebooks_f16,
                               const int32_t* list_ids, const int32_t* list_offsets, int64_t K, int32_t k, int32_t* idx,
                               float* score, void* workspace, int64_t workspace_bytes, void* stream);

/* Gram / cross-moment matrix of fp16 rows in fp64 (restated in tests/transforms_ref.py): what a PCA
 * diagonalises and what an OPQ Procrustes step decomposes (sonar_amd/transforms.py), contracted over the rows of a corpus.
 *
 * smi_gram: out[i][j] = sum over r < n of x[r][i] * y[r][j].  x contiguous fp16 [>= n, d1], y contiguous fp16 [>= n, d2] or
 *   NULL (y = x, d2 == d1), out device fp64 [d1, d2], overwritten.  Nothing is read back or allocated.
 * Numerics: the rows are cut into chunks of SMI_GRAM_CHUNK_ROWS consecutive rows.  Inside a chunk every product is exact (a
 *   product of two fp16 values is exact in fp32) and the sums are the fp32 accumulation of v_mfma_f32_16x16x32_f16 over the
 *   chunk's 32-row steps in ascending order.  A chunk's result is widened to fp64; the chunks of a span (a run of consecutive
 *   chunks whose length is a function of n alone) are added in ascending order and then the spans in ascending order.  The
 *   bits of out depend on (x, y, n) and the constant only: not on the CU count, the grid, the run, or the rows beyond n in
 *   the allocation.  No atomics.  Inf and NaN propagate; nothing is read at or beyond row n.  With y == NULL only the tiles on
 *   or above the diagonal are computed and an element below it is a copy of its mirror image: out is bitwise symmetric.
 *   Integer-valued operands whose chunk sums stay below 2^24 give the exact integer result.
 * workspace: device memory, 16-byte aligned, smi_gram_ws_bytes(n, d1, d2) bytes (one fp64 128 x 128 partial per span and tile;
 *   at most 32 spans).  The symmetric form fills only the T (T + 1) / 2 tile slots of the upper triangle, T = ceil(d / 128), and
 *   is content with smi_gram_ws_bytes(n, d, d) / T^2 * T (T + 1) / 2 bytes (an exact division).
 * Refused before any launch: null x, out or workspace, n < 1, y == NULL with d1 != d2, a small or misaligned workspace
 *   (SMI_ERR_INVALID_ARG); d1 or d2 below 64, not a multiple of 64 or above 8192, n above 2^31 - 256 (SMI_ERR_UNSUPPORTED).
 *   For these shapes smi_gram_ws_bytes returns 0. */
#define SMI_GRAM_CHUNK_ROWS 2048
int64_t smi_gram_ws_bytes(int64_t n, int32_t d1, int32_t d2);
int smi_gram(const void* x_f16, const void* y_f16, int64_t n, int32_t d1, int32_t d2, double* out, void* workspace,
             int64_t workspace_bytes, void* stream);

/* Embedding heads: BLASER / MuTox ---------------------------------------------
 * A small MLP over (features of) sentence embeddings.  Replaces
 *   BlaserModel.forward = F.normalize -> featurize_input -> mlp   sonar/models/blaser/model.py:82-125
 *   MutoxClassifier.forward = model_all (+ sigmoid)               sonar/models/mutox/model.py:18-24,
 *                                                                 sonar/models/mutox/factory.py:15-38
 * Hidden layers need in % 64 == 0 and out % 128 == 0 (MFMA GEMM tiles); the output layer has 1..8 units. */
typedef struct smi_mlp_head smi_mlp_head; /* opaque */
typedef struct smi_mlp_head_config {
  int32_t input_dim;  /* feature width: 6*d (COMET), 4*d (QE), d (MuTox) */
  int32_t n_layers;   /* Linear layers including the output layer, 1..8 */
  int32_t hidden_act; /* 0 ReLU, 1 tanh */
  int32_t out_act;    /* 0 none, 1 tanh (BLASER output_act), 2 sigmoid (MuTox output_prob) */
} smi_mlp_head_config;
typedef struct smi_mlp_head_layer {
  smi_tensor w; /* [out_dim, in_dim], nn.Linear layout */
  smi_tensor b; /* [out_dim] */
  int32_t out_dim;
  int32_t reserved;
} smi_mlp_head_layer;
int smi_mlp_head_create(const smi_mlp_head_config* cfg, const smi_mlp_head_layer* layers, smi_mlp_head** out);
void smi_mlp_head_destroy(smi_mlp_head* head);
/* features: form 0 f16(src); 1 QE [src, mt, src*mt, |mt-src|]; 2 COMET [ref, mt, src*mt, ref*mt,
 * |mt-src|, |mt-ref|] (model.py:95-125), inputs L2-normalised first when norm_emb (model.py:89-93).
 * src/mt/ref: device [rows, d] of `dtype`; out: device f16 [(rows+127)/128*128, blocks*d], pad rows zeroed. */
int smi_head_featurize(int32_t form, const void* src, const void* mt, const void* ref, int32_t dtype, int32_t rows,
                       int32_t d, int32_t norm_emb, void* out_f16, void* stream);
/* x: device f16 [(rows+127)/128*128, input_dim]; out: device fp32 [rows, out_dim];
 * out_act -1 = the configured one, else 0 / 1 / 2 as above. */
int smi_mlp_head_forward(smi_mlp_head* head, const void* x_f16, int32_t rows, int32_t out_act, float* out,
                         void* stream);

/* Training of MLP heads over frozen embeddings ----------------------------------
 * The recipe of examples/finetune_sonar_as_toxicity_classifier.ipynb part 4 (a head on the frozen encoder, AdamW,
 * gradient clipping) for the MLP that smi_mlp_head runs: dims [input_dim, hidden..., out], the same divisibility rules.
 * Semantics of torch.nn / torch.optim.AdamW (one parameter group: weights and biases decay alike).  Storage: masters,
 * moments and gradients fp32; an fp16 shadow (RNE) of the hidden weights feeds the same GEMM calls as
 * smi_mlp_head_forward; activations fp16; dz bf16; the backward products gW = dz^T A and dA = dz W take bf16 operands
 * with fp32 accumulation.  No atomics: every reduction has one fixed order, a run is reproducible bit for bit.
 * Dropout masks are a pure function: with site 0 = the input and l = after hidden layer l, row = the position in the batch
 * and step counted from 1, key = (step*16 + site) * 2^40 + row*width + col, z = mix(seed + 0x9E3779B97F4A7C15 * (key+1))
 * (mix = the splitmix64 finaliser of the sampler), u = (z >> 40) * 2^-24, kept iff u >= p; kept values are scaled by
 * 1/(1-p) in fp32 and rounded to fp16.  The key is taken modulo 2^64: the masks repeat after 2^20 steps. */
typedef struct smi_head_trainer smi_head_trainer; /* opaque */
typedef struct smi_head_trainer_config {
  int32_t input_dim;  /* % 64 == 0 */
  int32_t n_layers;   /* Linear layers including the output layer, 1..8 */
  int32_t hidden_act; /* 0 ReLU, 1 tanh */
  int32_t loss;       /* 0 ce (int32 labels, out >= 2, mean over rows), 1 bce with logits, 2 mse (fp32 targets
                         [n, out], mean over all elements) */
  int32_t max_batch;  /* batch capacity in rows */
  int32_t reserved;
  float p_in;         /* dropout on the input, [0, 1) */
  float p_hidden;     /* dropout after every hidden activation, [0, 1) */
  uint64_t seed;      /* of the dropout masks */
  float beta1, beta2, eps, weight_decay;
} smi_head_trainer_config;
/* layers: the initial weights, as for smi_mlp_head_create (fp32 or fp16, host or device). */
int smi_head_trainer_create(const smi_head_trainer_config* cfg, const smi_mlp_head_layer* layers,
                            smi_head_trainer** out);
void smi_head_trainer_destroy(smi_head_trainer* t);
/* One optimizer step on batch row r = dataset row (perm ? perm[offset + r] : offset + r), r < rows.
 *   x: device [n, input_dim] of x_dtype (SMI_F32 / SMI_F16); targets: device int32 [n] (ce) or fp32 [n, out];
 *   perm: device int64 or NULL.  lr: this step's learning rate (the schedule lives on the host); max_grad_norm <= 0 =
 *   no clipping, else the gradients are scaled by min(1, c / (||g|| + 1e-6)).
 *   The step's loss is recorded on the device (smi_head_trainer_losses).  loss_out == NULL: the step is only enqueued,
 *   nothing is read back and the caller guarantees labels in range -- provided the loss record has room: it holds 4096
 *   steps at creation, smi_head_trainer_reserve sizes it for a run up front, and a step past its end grows it, which
 *   waits for the device (and cannot be captured); loss_out != NULL: the batch's labels are read back
 *   and checked BEFORE anything is launched, and the call returns after the step with its loss.
 * Refused before any launch: a null handle or pointer, rows < 1, rows > max_batch, a label outside 0..out-1. */
int smi_head_trainer_step(smi_head_trainer* t, const void* x, int32_t x_dtype, const void* targets,
                          const int64_t* perm, int64_t offset, int32_t rows, float lr, float max_grad_norm,
                          float* loss_out, void* stream);
/* The same forward and backward pass with the masks of the NEXT step, no update: grads_out (host, fp32) receives the flat
 * gradient vector in the order W0, b0, W1, b1, ... (nn.Linear layouts). */
int smi_head_trainer_gradients(smi_head_trainer* t, const void* x, int32_t x_dtype, const void* targets,
                               const int64_t* perm, int64_t offset, int32_t rows, float* loss_out, float* grads_out,
                               void* stream);
/* Room in the loss record for `more_steps` further steps (allocates and waits for the device; call before the run). */
int smi_head_trainer_reserve(smi_head_trainer* t, int64_t more_steps);
/* losses of steps first .. first+count-1 (0-based) -> out (host); waits for the device. */
int smi_head_trainer_losses(smi_head_trainer* t, int64_t first, int64_t count, float* out);
/* fp32 masters of one layer -> host w_out [out, in], b_out [out]; waits for the device. */
int smi_head_trainer_export(smi_head_trainer* t, int32_t layer, float* w_out, float* b_out);
/* Inference on the current weights, the calls of smi_mlp_head_forward (no dropout): x device f16
 * [(rows+127)/128*128, input_dim], out device fp32 [rows, out]; out_act 0 none, 1 tanh, 2 sigmoid; rows <= max_batch. */
int smi_head_trainer_forward(smi_head_trainer* t, const void* x_f16, int32_t rows, int32_t out_act, float* out,
                             void* stream);
/* Test entries.  smi_head_bwd_gemm: the backward MFMA kernel alone, operands fp16 or bf16 (SMI_F16 / SMI_BF16), fp32 out:
 *   mode 0: out[M, N] = sum_r P[r, M] Q[r, N];  mode 1: out[R, N] = sum_m P[R, m] Q[m, N];  R, M % 128 == 0, N % 64 == 0.
 * smi_head_adamw: gradient-norm reduction, clip scale and one AdamW step (1-based `step`) on device vectors of n
 *   elements; norm_scale_out (host, may be NULL) receives {||g||, clip scale}. */
int smi_head_bwd_gemm(int32_t mode, const void* P, int32_t p_dtype, const void* Q, int32_t q_dtype, int32_t R,
                      int32_t M, int32_t N, float* out_f32, void* stream);
int smi_head_adamw(float* p, const float* g, float* m, float* v, void* shadow_f16, int64_t n, int64_t step, float lr,
                   float beta1, float beta2, float eps, float weight_decay, float max_grad_norm, float* norm_scale_out,
                   void* stream);

/* LASER2 BiLSTM text encoder -------------------------------------------------
 * Replaces LaserLstmEncoder.forward(seqs, seq_lens)   sonar/nn/laser_lstm_encoder.py:60-116
 * for the configurations of Laser2Config              sonar/models/laser2_text/config.py:12-38
 * (card sonar/cards/laser2_text_encoder.yaml: arch laser2 = 50004 / pad 1 / 320 / 512 / 5 layers / bidirectional / 0.0).
 * fp16 operands with fp32 accumulation; fp32 cell state, gates and pooling.  Any embed_dim / hidden_size / num_layers, uni- or
 * bidirectional: widths are zero-padded inside the engine, which is exact (a padded unit's c and h stay 0). */
typedef struct smi_laser2 smi_laser2; /* opaque */
typedef struct smi_laser2_config {
  int64_t vocab_size;    /* vocabulary_size: 50004 */
  int32_t pad_idx;       /* 1: its embedding row is used as stored; its positions pool as -inf (:105-110) */
  int32_t embed_dim;     /* model_dim: 320 */
  int32_t hidden_size;   /* 512 */
  int32_t num_layers;    /* 5 */
  int32_t bidirectional; /* 1 */
  float padding_value;   /* 0.0: pad_packed_sequence's value at positions >= a row's length (:83-85) */
} smi_laser2_config;
/* One direction of one nn.LSTM layer: lstm.{weight,bias}_{ih,hh}_l{k}[_reverse], PyTorch gate order i, f, g, o. */
typedef struct smi_laser2_layer {
  smi_tensor weight_ih; /* [4*hidden, in]: in = embed_dim (layer 0), hidden_size * (1 + bidirectional) after */
  smi_tensor weight_hh; /* [4*hidden, hidden] */
  smi_tensor bias_ih;   /* [4*hidden] */
  smi_tensor bias_hh;   /* [4*hidden] */
} smi_laser2_layer;
/* embed: embed_tokens.weight [vocab, embed_dim]; layers: [num_layers][1 + bidirectional] (forward, then reverse);
 * max_tokens_hint: workspace to reserve (sum of the lengths of a batch; it grows on demand). */
int smi_laser2_create(const smi_laser2_config* cfg, const smi_tensor* embed, const smi_laser2_layer* layers,
                      int64_t max_tokens_hint, smi_laser2** out);
void smi_laser2_destroy(smi_laser2* h);
/* ids: device int64 [n, s]; seq_lens: HOST int32 [n], each in [1, s], max == s (the reference asserts it, :86);
 * out: device fp32 [n, hidden_size * (1 + bidirectional)], forward units first, in the caller's row order (:114-116).
 * Positions whose token is pad_idx pool as -inf whatever seq_lens says; a row with non-pad tokens at or beyond its length
 * also pools padding_value (:83-114).  Out-of-vocabulary ids are not read: they raise a flag that smi_laser2_status reports. */
int smi_laser2_forward(smi_laser2* h, const int64_t* ids, const int32_t* seq_lens, int32_t n, int32_t s, float* out,
                       void* stream);
/* Synchronises `stream`; SMI_ERR_INVALID_ARG if a batch since the last call held ids outside [0, vocab_size) (the
 * reference's nn.Embedding raises IndexError there); clears the flag. */
int smi_laser2_status(smi_laser2* h, void* stream);
int64_t smi_laser2_device_bytes(const smi_laser2* h);

/* Host input path ------------------------------------------------------------
 * Replaces the fairseq2n C++ DataPipeline stages between the tokenizer and the model,
 * sonar/inference_pipelines/text.py:226-247 (`.map(truncate)`, `.dynamic_bucket(...)`,
 * `Collater(pad_value)`), fused with the NLLB id assembly of the token encoder
 * ([prefix] piece+1 ... [suffix]).  Pure host code (threads), writes into the caller's
 * (pinned) staging buffer.  SentencePiece segmentation itself is done by the caller with the
 * sentencepiece library's multi-threaded batch encode, as `pieces` (flat int32) + `piece_offsets`. */
int smi_host_token_lengths(const int64_t* piece_offsets, int64_t n, int32_t n_prefix, int32_t n_suffix,
                           int32_t max_seq_len, int32_t* out_lens, int64_t* n_truncated);
int smi_host_dynamic_bucket(const int32_t* lens, int64_t n, int64_t threshold, int32_t max_num,
                            int32_t min_num, int64_t* bounds, int64_t* n_buckets, int64_t* n_open);
int smi_host_collate_nllb(const int32_t* pieces, const int64_t* piece_offsets, const int32_t* lens,
                          int64_t first, int64_t n, const int64_t* prefix, int32_t n_prefix,
                          const int64_t* suffix, int32_t n_suffix, int32_t piece_shift, int64_t pad_value,
                          int64_t* out_ids, int32_t row_stride, int32_t num_threads);

/* WAV decoding on the host (the reference: fairseq2n AudioDecoder over libsndfile,
 * sonar/inference_pipelines/speech.py:292-308).  RIFF/WAVE with PCM 8/16/24/32-bit or IEEE float
 * 32/64-bit samples (incl. WAVE_FORMAT_EXTENSIBLE).  `bytes` is the file image.  smi_host_wav_decode
 * writes float32 [frames, channels] (channel-last, integer PCM scaled by 2^-(bits-1)). */
int smi_host_wav_info(const uint8_t* bytes, int64_t nbytes, int32_t* channels, int32_t* sample_rate, int64_t* frames);
int smi_host_wav_decode(const uint8_t* bytes, int64_t nbytes, float* out, int64_t frames, int32_t channels);
/* The same pair for any covered container, sniffed from the file image: RIFF/WAVE as above, or a native FLAC stream
 * (RFC 9639: every block-size / sample-size code, constant / verbatim / fixed / LPC subframes, Rice and Rice2
 * residuals, wasted bits, left-side / side-right / mid-side stereo, 4-32 bits per sample, header CRC-8 and frame
 * CRC-16 verified; an ID3v2 tag in front is skipped).  Ogg encapsulation returns SMI_ERR_UNSUPPORTED. */
int smi_host_audio_info(const uint8_t* bytes, int64_t nbytes, int32_t* channels, int32_t* sample_rate, int64_t* frames);
int smi_host_audio_decode(const uint8_t* bytes, int64_t nbytes, float* out, int64_t frames, int32_t channels);

/* Building blocks (exported for the parity tests and microbenchmarks) ------ */
/* TILE-MAJOR operand layout (SMI_GEMM_IN_TM / SMI_GEMM_OUT_TM, `tile_major` arguments): a K-major
 * fp16 matrix A[rows][k] (rows % 256 == 0, k % 32 == 0) stored as 16-KiB blocks, block
 * (r/256, c/32) at element offset ((r/256)*(k/32) + c/32) * 8192, and inside a block element
 * (rr = r%256, cc = c%32) at rr*32 + (((cc/8) ^ s(rr)) << 3) + cc%8 with s(rr) = q ^ ((q&1)<<1),
 * q = (rr>>2)&3 (i.e. 0,3,2,1 for q = 0..3: the bank swizzle of the 16x16x32 fragment reads) -- the LDS image of the
 * 256x256 tile engine, so one K slice of a tile is one linear 16 KiB read.  The encoder keeps
 * every GEMM operand (weights, LayerNorm / attention / FFN-inner outputs) in this layout. */
#define SMI_GEMM_IN_TM (1 << 12)  /* x and w are tile-major (m, n % 256 == 0) */
#define SMI_GEMM_OUT_TM (1 << 13) /* f16 output tile-major, as the next GEMM's x (needs IN_TM, ldo == n); with epilogues 8 / 9: the
                                   * f16 residual stream that is read-modified-written is tile-major */
/* dst <- tile-major(src) (inverse == 0) or dst <- row-major(src) (inverse != 0); f16, device. */
int smi_pack_tile_major(const void* src_f16, void* dst_f16, int32_t rows, int32_t k, int32_t inverse,
                        void* stream);
/* out = epilogue(X[m,k] . W[n,k]^T + bias[n]); epi & 0xff: 0 f16 out, 1 f16 ReLU out,
 * 2 fp32 residual accumulate (out += ...), 3 fp32 store, 4 fp32 residual += 0.5 * (...),
 * 5 f16 SiLU out, 6 f16 GLU out (n/2 wide), 7 f16 tanh out, 8 f16 residual accumulate
 * (out_f16 = f16(float(out_f16) + ...), one rounding), 9 the same with 0.5 * (...) (bias may be NULL);
 * (epi >> 8) & 0xf selects the tile engine: 0 auto, 1 128x128, 2 256x256 (needs m,n % 256 == 0);
 * layout flags SMI_GEMM_IN_TM (epilogues 0, 2, 3, 4, 6, 8, 9) and SMI_GEMM_IN_TM|SMI_GEMM_OUT_TM (0, 1, 5, 8, 9; 6 with ldo == n/2, a bias
 * and enough 256x256 tiles for the 4-wave engine -- SMI_ERR_UNSUPPORTED otherwise).
 * m%128==0, n%128==0, k%64==0. */
int smi_gemm_tn(int32_t epi, const void* x_f16, const void* w_f16, const float* bias, void* out,
                int32_t m, int32_t n, int32_t k, int32_t ldo, void* stream);
/* Split-K form of the same product: parts[z][m][n] (slab_dtype SMI_F32 or SMI_F16, row-major, z < ksplit) = X[:, Kz] . W[:, Kz]^T
 * (+ bias in part 0); the consumer sums the slabs (the decode step's and the small-batch encoder's N = model_dim
 * projections).  fp16 slabs saturate at +-65504.  in_tm: x and w tile-major. */
int smi_gemm_tn_splitk(const void* x_f16, const void* w_f16, const float* bias, void* parts, int32_t m, int32_t n, int32_t k,
                       int32_t ksplit, int32_t in_tm, int32_t slab_dtype, void* stream);
/* Which GEMM engine smi_gemm_tn (ksplit == 0) or smi_gemm_tn_splitk (ksplit >= 1; of epi_sel only SMI_GEMM_IN_TM is read, ldo is
 * ignored) would run for a request, without launching anything: the library's single routing function, steered by the same
 * tuning switches as a launch.  fold_kind: 0 none, 1 LayerNorm-fold producer, 2 producer that leaves the rows' partial sums,
 * 3 consumer with the exact mean term, 4 consumer with centred weights (fold_nparts partial sums per row); stats_kind: 0 none,
 * 1 tile statistics with scale > 0, 2 tile statistics otherwise.  num_cus 0: the current device's (256 without a device); any other
 * value needs no device.  engine SMI_GEMM_ENGINE_NONE: the launch is refused (SMI_ERR_UNSUPPORTED).  Like a launch, the query sees the
 * calling thread's grid cap (a chained decoder call caps its logits GEMM): grid_x is what a launch from THIS thread would get. */
enum {
  SMI_GEMM_ENGINE_NONE = 0,
  SMI_GEMM_ENGINE_RING = 1,         /* 128x128 tiles, ring = 0 (two stages, two workgroups per CU) or 4 stages */
  SMI_GEMM_ENGINE_LONE64 = 2,       /* 64x64 lone units */
  SMI_GEMM_ENGINE_LONE16 = 3,       /* k-sliced 64x64 units, unit = 128-column K blocks per unit */
  SMI_GEMM_ENGINE_PP256 = 4,        /* 8-wave 256x256 ping-pong engine */
  SMI_GEMM_ENGINE_V2 = 5,           /* 4-wave 256x256 engine, flag = LayerNorm-fold consumer */
  SMI_GEMM_ENGINE_V2_RESID = 6,     /* ... its tile-major residual stream, flag = leaves partial sums */
  SMI_GEMM_ENGINE_V2_STATS = 7,     /* ... its logits projection with tile statistics */
  SMI_GEMM_ENGINE_V2_LONE128 = 8,   /* ... its lone units of unit = 128 / 160 / 192 rows, flag = split-K slabs */
  SMI_GEMM_ENGINE_V2_LONE160 = 9,
  SMI_GEMM_ENGINE_V2_LONE192 = 10,
  SMI_GEMM_ENGINE_COUNT = 11
};
#define SMI_GEMM_ENGINE_NAMES \
  { "none", "ring", "lone64", "lone16", "pp256", "v2", "v2_resid", "v2_stats", "v2_lone128", "v2_lone160", "v2_lone192" }
typedef struct smi_gemm_route_info {
  int32_t engine;         /* SMI_GEMM_ENGINE_* */
  int32_t epi, layout;    /* the kernel's epilogue and LAYOUT (0 row-major, 1 tile-major in, 2 and out, 3 tile-major residual stream) */
  int32_t ring, unit, flag;
  int32_t grid_x, grid_y, lds_bytes, ksplit, raster;
  int32_t reserved;
  int64_t part_stride;    /* bytes between split-K slabs */
} smi_gemm_route_info;
int smi_gemm_route(int32_t epi_sel, int32_t m, int32_t n, int32_t k, int32_t ldo, int32_t has_bias, int32_t fold_kind,
                   int32_t fold_nparts, int32_t stats_kind, int32_t ksplit, int32_t slab_dtype, int32_t num_cus,
                   smi_gemm_route_info* out);
/* The number of K parts (<= max_parts) the decode-time projections give smi_gemm_tn_splitk for an [m, k] x [n, k] product;
 * num_cus as above.  Negative: an smi_status. */
int smi_gemm_splitk_parts(int32_t m, int32_t n, int32_t k, int32_t max_parts, int32_t num_cus);
/* The decoder's logits projection with its fused softmax statistics (exported for tests; TiedProjection + the beam search's
 * log_softmax, sonar/models/sonar_text/factory.py:300-315, sonar/inference_pipelines/text.py:305-346): x, w and the f16 output
 * tile-major, no bias (m, n % 256 == 0, k % 64 == 0), scale > 0; per (256-column tile t, row r), over the columns c < valid_n of
 * the tile: tile_max[t*m + r] = max_c scale*v, tile_sum[t*m + r] = sum_c exp(scale*v - tile_max), v = the ROUNDED f16 logit. */
int smi_gemm_tn_tile_stats(const void* x_f16_tm, const void* w_f16_tm, void* out_f16_tm, int32_t m, int32_t n, int32_t k,
                           float scale, int32_t valid_n, float* tile_max, float* tile_sum, void* stream);
/* dst[i] = (dst_dtype) src[i] for n elements of DEVICE memory (dtypes: smi_dtype incl. SMI_BF16; fp32 -> bf16 rounds to
 * nearest even).  The bf16 side of the pipelines' `dtype=` argument: `model.to(device, dtype)` / the embeddings returned by
 * TextToEmbeddingModelPipeline.predict (sonar/inference_pipelines/text.py:161-162, 262-268). */
int smi_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, void* stream);
/* out = f16(LN(x) * w + b); tile_major != 0: out in the tile-major layout ((rows+255)/256*256 rows allocated) */
int smi_layernorm(const float* x, const float* w, const float* b, float eps, void* out_f16,
                  int32_t rows, int32_t d, int32_t tile_major, void* stream);
/* The LayerNorm fold (exported for tests): an fp16 model's encoders launch no LayerNorm in front of a projection.  With
 * h = LN(x) = (x - mean) * rstd * g + b,   h . W^T + bias = rstd * (x . Wf^T - mean * c1) + c2,   Wf = W (.) g,
 * c1[n] = sum_k Wf[n][k], c2[n] = sum_k b[k] W[n][k] + bias[n]: the projection multiplies the tile-major fp16 residual stream x
 * ITSELF by the pre-scaled weights and applies the rows' statistics in its epilogue; the residual GEMM that wrote x leaves
 * them as per-row partial sums.
 * smi_ln_fold_prep: w f16 [n][k], g / b fp32 [k], bias fp32 [n] or NULL, all row-major -> wf f16 [n][k], c1 / c2 fp32 [n].
 * centered == 0: wf = f16(f32(w * g)), the fp32 product rounded to fp16, c1 = the row sums of the ROUNDED wf.  centered != 0: wf = f16(w * g - rowmean(w * g)), which
 * moves the mean term into the product (the epilogue is rstd * acc + c2); c1 = the row sums of wf, the rounding residue. */
int smi_ln_fold_prep(const void* w_f16, const float* g, const float* b, const float* bias_or_null, void* wf_f16, float* c1,
                     float* c2, int32_t n, int32_t k, int32_t centered, void* stream);
/* part[0][r] = (sum, sum of squares) of row r < m of the tile-major f16 stream x [rows % 256 == 0][d] (d % 32 == 0),
 * part[1 .. nparts-1][r] = (0, 0); part: [nparts][m] pairs of floats.  The statistics of a stream no GEMM has produced. */
int smi_row_stats_tm(const void* x_f16_tm, float* part, int32_t m, int32_t d, int32_t nparts, void* stream);
/* smi_gemm_tn with a LayerNorm fold (epi, operands, shapes and ldo as there; m, n % 256 == 0, x and w tile-major).
 * PRODUCER (part_out given): epilogues 8 / 9 on a tile-major stream; part_out[n/256][m] pairs <- (sum, sum of squares) of the
 * ROUNDED new values of each row over the 256 columns of each tile.  CONSUMER (part_in given): x = the stream, w = wf,
 * bias = c2, part_in[nparts][m] pairs whose sum over the parts is the row's (sum, sum of squares), 1 <= nparts <= 4, c1 given;
 * out = act(rstd * (x . wf^T - mean * c1) + c2), or act(rstd * x . wf^T + c2) with centered != 0, mean = sum / k,
 * rstd = 1 / sqrt(sumsq / k - mean^2 + eps).  Tile-major outputs: epilogues 0, 1 (both variants), 5 and -- on the 4-wave engine --
 * 6 (centred only); row-major outputs: 0 and 6, centred only.  part_out and part_in both NULL: the plain launch of the
 * residual epilogue; both given: SMI_ERR_INVALID_ARG.  What no kernel computes is refused with SMI_ERR_UNSUPPORTED before
 * anything is launched (smi_gemm_route answers the same question). */
int smi_gemm_tn_ln_fold(int32_t epi, const void* x_f16_tm, const void* w_f16_tm, const float* bias, void* out, int32_t m,
                        int32_t n, int32_t k, int32_t ldo, float* part_out, const float* part_in, const float* c1,
                        int32_t nparts, float eps, int32_t centered, void* stream);
/* qkv: f16 [t, 3*d] packed rows; cu_seqlens: device int32 [n+1]; ctx: f16 [t, d];
 * tile_major bit 0: ctx written tile-major, bit 1: qkv read tile-major (k = 3*d)
 * ((t+255)/256*256 rows allocated for a tile-major buffer) */
int smi_attention(const void* qkv_f16, const int32_t* cu_seqlens, void* ctx_f16, int32_t n,
                  int32_t max_len, int32_t d, int32_t heads, int32_t tile_major, void* stream);

/* The conformer's relative-position self-attention (exported for tests; fairseq2 RelativePositionSDPA as configured by
 * sonar/models/sonar_speech/factory.py via the w2v-BERT encoder: Shaw-style scores with the learned u / v biases):
 * scores[i][j] = ((q_i + u) . k_j + (q_i + v) . rp[rp_zero + i - j]) / 8 over the frames j of the clip, softmax, times V.
 * qkv: f16 [t, 3*d] packed rows (q | k | v); cu_seqlens: device int32 [n+1]; rp: f16 [rp_rows, d], the projected relative-position
 * table, row rp_zero = distance 0 (rows outside the table are clamped); u_bias / v_bias: fp32 [d]; ctx: f16 [t, d].
 * tile_major bit 0: ctx written tile-major, bit 1: qkv read tile-major (k = 3*d) ((t+255)/256*256 rows allocated for a
 * tile-major buffer).  head_dim = 64. */
int smi_relpos_attention(const void* qkv_f16, const int32_t* cu_seqlens, const void* rp_f16, int32_t rp_zero, int32_t rp_rows,
                         const float* u_bias, const float* v_bias, void* ctx_f16, int32_t n, int32_t max_len, int32_t d,
                         int32_t heads, int32_t tile_major, void* stream);

/* The row kernels of the speech encoder and the text decoder, one call each (exported for the kernel-level parity tests,
 * tests/test_gpu_row_kernels.py).  All pointers are device memory; cu: int32 [n+1] row offsets of the packed clips.  Widths: d in
 * {256, 512, 768, 1024, 2048} for the LayerNorms, d % 256 == 0 for the conv, head_dim = 64 for the attentions;
 * anything else is SMI_ERR_UNSUPPORTED.  Rows that no clip owns are neither read nor written. */
/* Frame stacking + LayerNorm: out[cu[i] + j][0 .. 2nb) = f16(LN(fbank[i][2j][:] | fbank[i][2j+1][:]) * w + b) for j < cu[i+1] - cu[i],
 * columns 2nb .. ldo-1 zero; fbank fp32 [n][t][nb], w / b fp32 [2nb], out f16 [rows][ldo]; 2nb <= ldo <= 192, max_len >= the longest
 * stacked clip. */
int smi_stack_ln(const float* fbank, int32_t n, int32_t t, int32_t nb, const int32_t* cu, int32_t max_len, const float* w,
                 const float* b, float eps, void* out_f16, int32_t ldo, void* stream);
/* x <- LN(x) * w1 + b1 in place (x_dtype SMI_F32 or SMI_F16); h = f16(w2 ? LN(x) * w2 + b2 : x), or nothing with h NULL.  With an
 * fp16 stream the second LayerNorm sees the rounded values the stream holds.  layout bit 0: h tile-major, bit 1: x tile-major
 * (fp16 stream, d % 512 == 0; (rows+255)/256*256 rows allocated for a tile-major buffer). */
int smi_ln2(void* x, int32_t x_dtype, const float* w1, const float* b1, const float* w2_or_null, const float* b2_or_null, float eps,
            void* h_f16_or_null, int32_t rows, int32_t d, int32_t layout, void* stream);
/* The conformer's depthwise convolution + BatchNorm (folded to scale / shift) + SiLU over packed clips:
 * y[t][c] = f16(silu(scale[c] * sum_k w16[c][k] * x[t + k - (ktaps-1)/2][c] + shift[c])), frames outside the clip are zero.
 * PRECISION CONTRACT: the taps w (fp32 [d][ktaps]) are rounded to fp16 (w16) whatever the model dtype, like every GEMM weight of the
 * engine; the products w16 * x are exact and accumulate in fp32.  x, y: f16 [rows][d]; ktaps 7 or 31; d % 256 == 0;
 * layout bit 0: y tile-major, bit 1: x tile-major. */
int smi_dwconv_bn_silu(const void* x_f16, const int32_t* cu, const float* w, const float* scale, const float* shift, void* y_f16,
                       int32_t n, int32_t max_len, int32_t d, int32_t ktaps, int32_t layout, void* stream);
/* The attention pooler: one query per clip and head over the clip's frames, scores / 8.  q: f16 [n][d]; kv: f16 [rows][2d] (k | v);
 * ctx: f16 [n][d]; a clip of length 0 yields zeros. */
int smi_pool_attention(const void* q_f16, const void* kv_f16, const int32_t* cu, void* ctx_f16, int32_t n, int32_t d, int32_t heads,
                       void* stream);
/* x <- x + sum_z parts[z] (+ c[row / group]) in fp32, in that order, ONE rounding for an fp16 stream; h = f16(LN(x) * w + b) of the
 * stored row.  parts: nparts slabs of x's shape, part_stride ELEMENTS apart (parts_dtype SMI_F32 or SMI_F16), or NULL with
 * nparts == 0; c: fp32 [ceil(rows / group)][d] or NULL; prefetch: prefetch_bytes of device memory that surplus workgroups pull into
 * the cache (no effect on x or h), or NULL. */
int smi_sum_layernorm(void* x, int32_t x_dtype, const void* parts_or_null, int32_t parts_dtype, int32_t nparts, int64_t part_stride,
                      const float* c_or_null, int32_t group, const float* w, const float* b, float eps, void* h_f16, int32_t rows,
                      int32_t d, int32_t h_tile_major, const void* prefetch_or_null, int64_t prefetch_bytes, void* stream);
/* Single-query attention of the decode step at position pos.  kv: f16 [pos+1][rows_pad][3d] (q | k | v slabs, one per position);
 * anc: int32 [rows][anc_stride], anc[r][j] = the row of slab j that holds hypothesis r's position j < pos (anc_stride >= pos);
 * the query is q of slab pos, row r; key / value j < pos are row anc[r][j] of slab j, key / value pos row r of slab pos;
 * scores / 8; ctx: f16 [rows][d]. */
int smi_dec_attention(const void* kv_f16, const int32_t* anc, int32_t anc_stride, void* ctx_f16, int32_t rows, int32_t rows_pad,
                      int32_t d, int32_t heads, int32_t pos, void* stream);
/* Causal self-attention of the teacher-forced rows: nseq sequences of seq rows each (cu = [0, seq, 2 seq, ...]), query i of a
 * sequence sees its keys 0..i; qkv: f16 [nseq*seq][3d]; ctx: f16 [nseq*seq][d], both row-major. */
int smi_causal_attention(const void* qkv_f16, const int32_t* cu, void* ctx_f16, int32_t nseq, int32_t seq, int32_t d, int32_t heads,
                         void* stream);

/* The beam search's state kernels on caller-owned device arrays, one call each (exported for the kernel-level tests,
 * tests/test_gpu_beam_kernels.py; the launchers are those of smi_text_decoder_generate).  Every pointer is device memory.
 *
 * SPECIAL IDS.  The selection reads tile 0 (ids 0..255) and the k2 tiles of largest raw maximum.  That holds every candidate only
 * when the ids the masks touch -- PAD, EOS (blocked before min_seq_len), UNK (penalised) -- live in tile 0: a masked id that is the
 * maximum of a later tile would take a slot from a tile that holds a real candidate.  So pad_idx, eos_idx and unk_idx must be below
 * 256 (-1 = none, where an entry allows it); smi_text_decoder_create, smi_vocab_select and smi_vocab_select_banned refuse anything
 * else with SMI_ERR_UNSUPPORTED before the device is asked for.
 *
 * A per-sentence prompt table (tok NULL = none, the scalar arguments hold): sentence s has prompt tok[s][0 .. len[s]), len[s] >= 1,
 * its cap max_len_s = min(len[s] + gen_cap, model_max) and min_len_s = min(len[s] + min_gen, max_len_s).  At the step that chooses
 * token step_nr it is forced to tok[s][step_nr] while step_nr < len[s], forced to EOS at step_nr == max_len_s - 1, free before that
 * (EOS blocked while step_nr < min_len_s), and past its cap it does nothing.  The caller keeps len[s] <= stride and the prompt ids
 * inside the vocabulary: the table is device memory and is not read on the host. */
typedef struct smi_prompt_table {
  const int32_t* tok; /* [n][stride], left-aligned */
  const int32_t* len; /* [n] */
  int32_t stride, gen_cap, min_gen, model_max;
} smi_prompt_table;

/* The selection of one step.  logits: fp32 [rows][ldl] row-major, or (logits_f16_tm) fp16 tile-major with K = ldl in a buffer of
 * (rows + 255) / 256 * 256 rows; ldl a multiple of 256 >= vocab, at most 2048 tiles.  tile_max / tile_sum: fp32 [ldl / 256][stat_rows], per 256-column tile
 * of logits * inv_temp the maximum and the sum of exp(v - maximum) (columns >= vocab excluded).  Outputs: pmax / psum [rows], the
 * row's softmax normaliser (pmax = the row maximum, bit for bit); pval / pidx [rows][16], the first k2 entries = the row's best
 * candidates (value desc, token asc), value = logits * inv_temp (- unk_penalty for unk_idx) in fp32, where pad_idx, columns >= vocab,
 * -inf and -- block_eos -- eos_idx are no candidates; (-inf, INT32_MAX) fills a shorter list.  k2 = 0 writes pmax / psum only.  With
 * a table, row r belongs to sentence r / group: block_eos is its sentence's at step_nr (the argument is not read), and a row whose
 * sentence is not free there gets pmax / psum only. */
typedef struct smi_vocab_select_args {
  const void* logits;
  int32_t ldl, logits_f16_tm, rows, vocab;
  const float* tile_max;
  const float* tile_sum;
  int32_t stat_rows; /* >= rows */
  int32_t k2;        /* 0..16 */
  float inv_temp;    /* > 0 */
  int32_t pad_idx, eos_idx, unk_idx; /* -1 = none; below 256 and below vocab */
  float unk_penalty;
  int32_t block_eos;
  float* pmax;
  float* psum;
  float* pval;
  int32_t* pidx;
  smi_prompt_table table;
  int32_t group, step_nr; /* read with a table: group >= 1, step_nr >= 1 */
} smi_vocab_select_args;
int smi_vocab_select(const smi_vocab_select_args* args, void* stream);

/* The state of a search over n sentences x beam rows (row r = sentence r / beam), stride int32 per row of history.
 *   tok / cum [n*beam]: the token fed at the current position and the cumulative log-probability of each row;
 *   nactive / done / fin_count [n], ndone [1]: live rows (rows >= nactive[s] of a sentence are never read), finished flag,
 *     finished hypotheses, number of finished sentences;
 *   parent / new_tok / new_cum [n*beam]: what a step decides, consumed by the reorder;
 *   fin_tok [n*beam][stride], fin_len / fin_score [n*beam]: finished hypotheses in the order they finished (generated tokens + EOS);
 *   margins [n][2] or NULL: smallest gap between neighbours of a step's sorted candidate list up to the first one not consumed,
 *     and (written by the output, for >= 2 hypotheses) best minus second finished score;
 *   anc[2] / hist[2] [n*beam][stride]: ancestry (row of position j's slab) and tokens; position pos reads buffer pos & 1 and the
 *     reorder writes the other one. */
typedef struct smi_beam_state {
  int32_t* tok;
  float* cum;
  int32_t* nactive;
  int32_t* done;
  int32_t* ndone;
  int32_t* parent;
  int32_t* new_tok;
  float* new_cum;
  int32_t* fin_tok;
  int32_t* fin_len;
  float* fin_score;
  int32_t* fin_count;
  float* margins;
  int32_t* anc[2];
  int32_t* hist[2];
  int32_t n, beam, stride; /* beam 1..8 */
} smi_beam_state;

/* tok = hist[0][r][0] = first_tok (or first_toks[(r / beam) * first_stride] when given), cum = 0, anc[0][r][0] = r, nactive = 1,
 * done = fin_count = ndone = 0, margins = +inf. */
int smi_beam_init(const smi_beam_state* st, int32_t first_tok, const int32_t* first_toks_or_null, int32_t first_stride, void* stream);

/* One beam step at position pos (it chooses token step_nr = pos + 1) from what smi_vocab_select left.  Per sentence:
 *   done: parent = the row itself, new_tok = tok, new_cum = cum (the rows are inert), nothing else is written;
 *   forced prompt token (step_nr < prompt_len): every live row takes forced_tok, new_cum = cum + logit * inv_temp - lse;
 *   forced EOS (step_nr == max_len - 1): the live rows finish in order (score desc, row asc) until `beam` have, the sentence is done;
 *   free: the candidates cum + pval - lse of the live rows' lists, ordered score desc, row asc, token asc (-inf is none).  An EOS among
 *     the first `beam` of them finishes its row (in that order; the `beam`-th finished hypothesis ends the sentence at once, inert
 *     rows as above); otherwise the first `beam` non-EOS candidates of the first 2 beam continue, nactive = their number, and a
 *     spare slot keeps parent = itself, new_tok = tok, new_cum = -inf.
 * lse = pmax + log(psum) (fast log); fin_score = score / (step_nr ^ len_penalty) with normalize, else the score.
 * k2 must be 2 * beam; stride >= pos + 2; eos_idx (and forced_tok on a forced step) inside [0, vocab).  With a table, prompt_len /
 * forced_tok / max_len are the sentence's own and the scalars are not read. */
typedef struct smi_beam_step_args {
  const void* logits;
  int32_t ldl, logits_f16_tm, vocab;
  const float* pmax;
  const float* psum;
  const float* pval;
  const int32_t* pidx;
  int32_t k2, pos, prompt_len, forced_tok, max_len;
  float inv_temp, len_penalty;
  int32_t normalize, eos_idx;
  smi_prompt_table table;
} smi_beam_step_args;
int smi_beam_step(const smi_beam_state* st, const smi_beam_step_args* args, void* stream);

/* The reorder after the step at pos, from buffer c = pos & 1 to the other: anc'[r][j] = anc[parent[r]][j] (j < pos), anc'[r][pos] =
 * parent[r]; hist'[r][j] = hist[parent[r]][j] (j <= pos), hist'[r][pos + 1] = new_tok[r]; tok = new_tok, cum = new_cum.  Positions
 * beyond pos + 1 of the destination are not written.  stride >= pos + 2; parent must hold row numbers (a step wrote them). */
int smi_beam_reorder(const smi_beam_state* st, int32_t pos, void* stream);

/* The finished hypotheses of each sentence, best first (stable: equal scores keep the order they finished in): out_tok
 * [n*beam][out_stride] (-1 beyond the length; fin_len <= out_stride), out_len / out_score [n*beam]; a slot past fin_count is -1 /
 * length 0 / score -inf.  margins[s][1] is written when the sentence has >= 2 hypotheses. */
int smi_beam_output(const smi_beam_state* st, int32_t out_stride, int32_t* out_tok, int32_t* out_len, float* out_score, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SONAR_MI355_H */
