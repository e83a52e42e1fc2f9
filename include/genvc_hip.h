/*
 * genvc_hip.h -- C ABI of libgenvc_hip.so: the MI355X (gfx950) implementation of GenVC's
 * autoregressive codec-token generation hot path.
 *
 * The reference (caizexin/GenVC) is pure Python and has no FFI layer of its own; the seam this
 * library sits behind is the duck-typed object API that inference/inference_utils.py consumes
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it replaces
 * (paths relative to the reference repo).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C symbols, no C++ types or exceptions across the boundary;
 *   - every function returns 0 on success or a negative GVC_ERR_* code; the message of the
 *     last failure on the calling thread is available from gvc_last_error();
 *   - every launch is asynchronous on the caller's stream (a hipStream_t passed as void*);
 *     no hidden synchronisation or allocation after *_create / *_bind_*;
 *   - tensor arguments are raw DEVICE pointers borrowed from the caller (fp32 unless stated,
 *     row-major, contiguous); index arrays are DEVICE int32; the library frees only what it
 *     allocated in *_create;
 *   - a context is bound to the device that was current at *_create and must not be used
 *     from two host threads at once; contexts are independent of each other.
 *
 * Environment switches read by the library (eleven; everything else that used to be a run-time knob is a constant now, and the
 * experiments that lost are gone from the kernels: profiles/r06_removed_experiments.patch).  All default to the shipped configuration.
 *   GVC_PERSIST=0            never use the one-launch steps (one stream and 2..16 rows then take the launch-per-phase paths)
 *   GVC_PERSIST_ROWS=0       2..16 rows keep the launch-per-phase rows path (the one-stream one-launch step stays on)
 *   GVC_PERSIST_XCD=0        one-stream step: device-wide hand-off of the MLP's hidden units instead of the XCD-local layout
 *                            (for partition modes in which a 256-workgroup grid is not dealt 8 x 32 over the XCDs; the topology
 *                            probe switches it off by itself when it sees such a deal)
 *   GVC_DEFER_DECODE=0       one-stream generation on the one-launch step: the eager order [sample, decode] instead of deferring the
 *                            decode of a call's last token to the next call that continues the slot (read at gvc_gpt_create; for A/B
 *                            runs and the tests that compare the two orders)
 *   GVC_PERSIST_TEST_GRID=n  test hook: launch the one-launch steps with n < 256 workgroups (every hand-off then times out)
 *   GVC_PERSIST_STAMPS=1     in-kernel wall-clock stamps of the one-launch steps (scripts/stamps_persist.py, scripts/stamps_rows.py).  The
 *                            one-stream step stamps in a kernel variant of its own, chosen when the context prepares that step and
 *                            instantiated for d_model 1024 only: at other widths the switch leaves the one-stream step as it is
 *   GVC_DEBUG_STAMPS=1       in-kernel stamps of the launch-per-phase decode kernels (scripts/stamps.py)
 *   GVC_ROWS_DECODE_MIN=n    smallest batch that decodes on the MFMA rows path when the one-launch rows step does not serve it
 *                            (default 5; 0: never -- the 8-stream GEMV groups; tests use it to reach both paths)
 *   GVC_GRAPHS=0             ContentVec and Perceiver: eager launches instead of one hipGraph per shape
 *   GVC_VOCODER_GRAPH=0|2    HiFi-GAN: eager launches / only the conv chain as a graph (default 1: the whole call)
 *   GVC_VOCODER_SMALL_CONV=0|2  HiFi-GAN: every conv on the tiled GEMM / only the ResBlocks on k_conv_lds (the paths other shapes take)
 * Outside the library: GENVC_HIP_LIB (genvc_amd/_lib.py: another build of the library, for A/B runs), GVC_BENCH_* (bench.py dry runs).
 */
#ifndef GENVC_HIP_H
#define GENVC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVC_OK 0
#define GVC_ERR_ARG (-1)          /* bad argument / shape */
#define GVC_ERR_HIP (-2)          /* a HIP runtime call failed */
#define GVC_ERR_STATE (-3)        /* weights missing, cache overflow, wrong call order */
#define GVC_ERR_UNSUPPORTED (-4)  /* dimension not supported by the kernels */
#define GVC_ERR_TIMEOUT (-5)      /* a hand-off of a one-launch step timed out (not all 256 workgroups resident): the previous decode / generate /
                                     cached-prefill call produced garbage; the context has switched to the launch-per-phase paths and stays usable --
                                     reset the affected slots and repeat the call (gvc_gpt_health).  Distinct from GVC_ERR_STATE (a full KV cache,
                                     missing weights), which repeating does not cure */

typedef void* gvc_stream;         /* hipStream_t */

int gvc_version(void);
const char* gvc_last_error(void);

/* ------------------------------------------------------------------------------------------
 * GPT: prefill, KV-cached decode step, head, latent re-pass.
 * Replaces layers/gpt.py:GPT.{init_gpt_for_inference,compute_embeddings(prefix store),forward
 * (return_latent=True)} (gpt.py:197-218, 375-508, 572-592), layers/gpt_inference.py:
 * GPT2InferenceModel.forward (:55-124) and the HF GPT2Model block stack it drives
 * (gpt.py:42-84, gpt_inference.py:97-110).
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_gpt gvc_gpt;

typedef struct gvc_gpt_dims {
    int32_t n_layer;      /* gpt_layers */
    int32_t d_model;      /* gpt_n_model_channels; multiple of 256 */
    int32_t n_head;       /* gpt_n_heads; head_dim = d_model / n_head must be 64, 128 or 256 */
    int32_t vocab;        /* gpt_num_audio_tokens (1026) */
    int32_t max_mel_pos;  /* rows of mel_pos_embedding (608) */
    int32_t max_text_pos; /* rows of text_pos_embedding (404) */
    int32_t n_text;       /* gpt_number_text_tokens (258) */
    int32_t max_seq;      /* KV-cache positions per slot (>= 1083, gpt.py:198) */
    int32_t max_slots;    /* concurrent streams whose KV cache is resident */
    int32_t max_rows;     /* capacity (rows) of one prefill / latent re-pass call, all slots together */
    int32_t weight_dtype; /* 0: fp32 (reference numerics). 1: the c_attn/c_proj/c_fc/mlp c_proj/mel_head matrices are
                             rounded to bf16 at bind time; the decode step and the skinny MFMA path stream bf16 copies (half the HBM bytes),
                             every product and accumulation stays fp32; KV cache and activations stay fp32.
                             2: as 1, and the KV cache holds bf16 too (k / v rounded to nearest even where they enter the cache,
                             widened to fp32 where the attention kernels use them; half the cache bytes).
                             3: as 2, and the one-launch rows step (2..16 rows that continue cached sequences: batched decode steps, cached
                             chunk prefills; csrc/persist_rows_b16.h) rounds the four activations that cross its hand-offs -- x into LN1, the
                             attention output, x' into LN2, the gelu output -- to bf16 where they are published and multiplies on bf16 MFMAs with
                             fp32 accumulation (LayerNorm gain folded into the packed bf16 weights); residual stream, softmax, statistics and q stay
                             fp32.  The other paths of such a context (one stream, full prefills, 17+ streams) compute as mode 2.  Not bit-exact
                             against any reference by construction: oracle rounding points `dims["act_bf16"]`.
                             4 ("bf16_mfma"): as 3, and every other pass over MORE THAN ONE row -- full prefills, cached chunk prefills, the
                             latent re-pass, verification rows of assisted decoding, 17+ streams, and 2..16 rows whenever the one-launch rows
                             step is switched off or has timed out -- runs its four projections per layer on bf16 matrix cores
                             (v_mfma_f32_16x16x32_bf16, csrc/gemm_b16.hip) with the rounding points of the rows step, so they are the same on
                             every multi-row path: x~ = bf16(x) into c_attn / c_fc with the LayerNorm statistics taken over x~ in fp32 and the
                             gain folded into bf16(W g); the attention output and gelu_new(.) rounded to bf16 where they are stored;
                             residual stream, q, softmax, k / v (bf16 into the cache as in 2), every accumulation and the head stay fp32.  One
                             row (the one-stream decode step, the fused skinny path) computes as mode 2, as in mode 3.  Costs a second bf16 copy of
                             the four block matrices in MFMA fragment order: 12 d^2 x 2 bytes per layer (755 MB at d = 1024, L = 30), packed
                             outside the data path (first call after a bind, or gvc_gpt_warmup).  Needs d_model % 256 == 0, d_model <= 2048.
                             Oracle: gpt_blocks(act_bf16, kv_bf16), gpt_prefill(act_bf16_prefill) */
} gvc_gpt_dims;

int gvc_gpt_create(const gvc_gpt_dims* dims, gvc_gpt** out);
int gvc_gpt_destroy(gvc_gpt* ctx);

/* One-time repack of a tensor named as in the reference GPT state dict, e.g.
 * "gpt.h.3.attn.c_attn.weight" (HF Conv1D [in,out] -> row-per-output layout), "mel_head.weight",
 * "mel_embedding.weight", "final_norm.bias".  `src` is a device pointer with `numel` floats.
 * Unknown names (text_head.*, attn.bias buffers, conditioning_perceiver.*) return GVC_OK and are
 * ignored, mirroring load_state_dict(strict=False) at inference/model_init.py:22. */
int gvc_gpt_bind_weight(gvc_gpt* ctx, const char* name, const float* src, int64_t numel, gvc_stream s);
/* number of GPT tensors still unbound (0 = ready) */
int gvc_gpt_missing_weights(gvc_gpt* ctx);

/* Build the prefix embeddings of GPT.compute_embeddings (gpt.py:572-581):
 * prefix[b] = [cond_latents[b] (n_cond rows) | text_embedding(<s> codes </s>) + text_pos[0..Tc+1]].
 * codes: int32 [B,Tc] content codes; out: [B, n_cond+Tc+2, d]. */
int gvc_gpt_prefix_embeddings(gvc_gpt* ctx, const float* cond_latents, int32_t n_cond,
                              const int32_t* codes, int32_t B, int32_t Tc, int32_t start_text,
                              int32_t stop_text, float* out, gvc_stream s);

/* Prefill (gpt_inference.py:81-91): rows = [prefix_emb[b] (P rows) | mel_embedding[start_tok] +
 * mel_pos[0]]; fills the KV cache of slots[b] (positions 0..P), sets its length to P+1 and its next
 * mel position to 1; writes the last row's latent = final_norm(ln_f(h)) [B,d] and logits [B,vocab].
 * logits_out / latent_out may be NULL: the results then stay in the context's staging buffers, which is
 * where gvc_gpt_generate reads the first step's logits from. */
int gvc_gpt_prefill(gvc_gpt* ctx, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P,
                    int32_t start_tok, float* logits_out, float* latent_out, gvc_stream s);
/* Prefix caching: the same call when the first n_cached rows of prefix_emb (the 32 conditioning latents of the reference
 * speaker, identical for every segment of an utterance: inference_utils.py:43-66 rebuilds them per segment) are ALREADY in
 * the slots' KV cache from an earlier gvc_gpt_prefill[_cached] with the same leading rows.  Only rows n_cached..P are
 * computed and appended; results are bit-identical to the full prefill while the uncached rows fit the skinny path (<= 128
 * rows per call) and equal to rounding on the tiled path (its split-K depends on the row count).  The caller vouches for
 * the cache contents. */
int gvc_gpt_prefill_cached(gvc_gpt* ctx, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P,
                           int32_t n_cached, int32_t start_tok, float* logits_out, float* latent_out, gvc_stream s);
/* The conditioning rows alone: K/V of cond_latents[b] (n_cond rows, [B, n_cond, d]) into the caches of slots[b], length n_cond; no text
 * rows, no start token, no outputs.  For a caller that knows the target speaker before the first source segment arrives (a streaming
 * session; the reference rebuilds these rows inside every segment's prefill, inference_utils.py:43-66): every segment, the first one too,
 * then calls gvc_gpt_prefill_cached with n_cached = n_cond and its first audio chunk no longer waits for the 32 conditioning rows. */
int gvc_gpt_prefill_cond(gvc_gpt* ctx, const int32_t* slots, int32_t B, const float* cond_latents, int32_t n_cond, gvc_stream s);

/* One KV-cached decode step for B streams (gpt_inference.py:92-112):
 * x = mel_embedding[tok_in[b]] + mel_pos[pos(slot)], 30 blocks against the cache, double
 * LayerNorm, mel_head.  Appends K/V, advances the slot's length and mel position.  For callers that sample themselves: the
 * logits go to the caller only (gvc_gpt_generate continues a slot from its last prefill / generate, not from here). */
int gvc_gpt_decode_step(gvc_gpt* ctx, const int32_t* slots, int32_t B, const int32_t* tok_in,
                        float* logits_out, float* latent_out, gvc_stream s);

/* Reset a slot (length 0, mel position 0) so that decode steps can also build a context from
 * nothing (used by tests). */
int gvc_gpt_reset_slots(gvc_gpt* ctx, const int32_t* slots, int32_t B, gvc_stream s);

/* KV fan-out: pair i copies slot src_slots[i] to slot dst_slots[i] (device arrays of n entries, n <= max_slots): positions
 * [0, length of the source) of every (layer, k|v, head) run of the cache in 16-byte accesses (fp32 and bf16 caches alike), the slot's
 * length and mel position, and the logits / latent its last prefill or generate call parked.  Afterwards the destination continues
 * exactly as the source would: N candidates of one item cost one prefill (GPT.generate(num_return_sequences=N)).  One launch over a
 * fixed grid, no allocation.  A destination must not be the source or destination of another pair; a pair with a slot outside
 * [0, max_slots) or with src == dst copies nothing. */
int gvc_gpt_kv_fanout(gvc_gpt* ctx, const int32_t* src_slots, const int32_t* dst_slots, int32_t n, gvc_stream s);

/* Log-probability of generated sequences under the RAW model distribution (an extension: the reference has no such score):
 * logprob_out[r] = sum over t < length_out[r] of log_softmax(mel_head(latents[r][t]))[tokens[r][t]], where length_out[r] runs up to and
 * including the first stop_tok of row r, or is n without one.  latents [R][n][d] (contiguous) are the generation loop's
 * final_norm(ln_f(h)) rows (latents_out of gvc_gpt_generate*), so mel_head of row t is the logits row token t was chosen from -- before
 * any repetition penalty, logits processor or warper.  With bf16 weight storage (weight_dtype >= 1) the bound mel_head is held rounded to
 * bf16 in both its copies, so the score uses the very weights the loop drew from; the loop's GEMV and this GEMM sum in different orders,
 * so the logits agree to fp32 rounding, not bit for bit (in every mode).  tokens int32 [R][tokens_stride >= n].  token_logprobs_out (nullable) [R][n]:
 * the per-token terms, 0 from length_out[r] on.  The fp32 head GEMM on the bound mel_head (into the context's scratch, in chunks of whole
 * sequences) followed by a row kernel (max, log-sum-exp with the accurate expf / logf, the sum in double in a fixed order).  No
 * allocation, no synchronisation; not part of any captured step graph. */
int gvc_gpt_sequence_logprobs(gvc_gpt* ctx, const int32_t* tokens, int32_t tokens_stride, const float* latents, int32_t R, int32_t n,
                              int32_t stop_tok, double* logprob_out, int32_t* length_out, float* token_logprobs_out, gvc_stream s);

/* Teacher-forced latent re-pass, GPT.forward(..., cond_latents=, return_latent=True)
 * (gpt.py:375-508, call site inference_utils.py:71-76): rows = [prefix_emb (P) | start, codes(n),
 * stop x4]; out[b] = final_norm(ln_f(h)) of the first n mel rows -> [B,n,d].  Uses scratch slot
 * `slots[b]` for K/V (its previous content is overwritten).  gen_codes: int32 [B,n]. */
int gvc_gpt_latents(gvc_gpt* ctx, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P,
                    const int32_t* gen_codes, int32_t n, int32_t start_tok, int32_t stop_tok,
                    float* out, gvc_stream s);

/* Trace pass: the attention weights, hidden states and content alignment of a generated sequence, by one teacher-forced pass over
 * rows = [prefix_emb (P) | start, codes 0 .. n-2] of B items (T = P + n rows per item, embedded as gvc_gpt_latents embeds them; row
 * P + i is the query of generation step i, the one that produced code i).  A full pass without a cache reproduces the per-step rows
 * of HF's cached loop (output_attentions / output_hidden_states of transformers' generate with eager attention) to fp32 rounding.
 * Always the launch-per-phase layer loop, with taps between its phases; fp32 contexts only (GVC_ERR_UNSUPPORTED otherwise).
 *
 * lengths int32 [B] (device) and lengths_host (the same values, host: the argument check reads them without a synchronisation):
 * item b's generated length, its stop code counted, in [1, n].  Steps i >= lengths[b] of a finished item fed HF's model a pad
 * token; their rows mean nothing and are written as zeros here (a deviation from HF, which returns them).
 *
 * Outputs (device, each nullable, at least one set; every element is written, no memset needed):
 *   probs  fp32 [L][B][H][T][T]: (l, b, h, t, k) = softmax weight of query row t on key k in layer l; exactly 0 for k > t; rows
 *          t >= P + lengths[b] all zeros.
 *   hidden fp32 [L+1][B][T][D]: plane 0 the embedded rows, plane l (0 < l < L) the residual after layer l, plane L ln_f of the last
 *          residual -- HF GPT-2's hidden_states (not final_norm(ln_f(.)), which is `latents`); rows t >= P + lengths[b] zeros.
 *   align  fp32 [B][n][n_content]: the mean over the heads of the chosen layers (layer_mask bit l; 0 = all layers) of the weight step
 *          i's query (row P + i) puts on the key rows content_off .. content_off + n_content - 1 of the prefix.  For a prefix of
 *          gvc_gpt_prefix_embeddings = [cond (n_cond) | start text | Tc content codes | stop text] the content rows are
 *          content_off = n_cond + 1, n_content = Tc: the conditioning rows and the text start / stop rows are not content.  Summed in
 *          a fixed order (heads inside a layer, layers in order), no atomics: the same input gives the same bits.  Computed layer by
 *          layer from probs' plane, or with probs null from `scratch` fp32 [B][H][T][T] (required then).
 * Uses slots[b] as K/V scratch and leaves the slots as gvc_gpt_latents leaves them (length 0).
 * GVC_ERR_ARG: B > max_slots, B * T > max_rows, T >= max_seq, n > max_mel_pos - 5, a length outside [1, n], content rows outside the
 * prefix, a layer mask naming a layer the model does not have, no output set. */
typedef struct gvc_trace_options {
    int32_t start_tok, stop_tok;          /* start / stop audio token (the stop token embeds nothing here: n - 1 codes are read) */
    int32_t content_off, n_content;       /* align: the content key rows of the prefix */
    uint64_t layer_mask;                  /* align: bit l = layer l counts; 0 = every layer */
    float* probs;
    float* hidden;
    float* align;
    float* scratch;
} gvc_trace_options;
int gvc_gpt_trace(gvc_gpt* ctx, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P, const int32_t* gen_codes, int32_t n,
                  const int32_t* lengths, const int32_t* lengths_host, const gvc_trace_options* opt, gvc_stream s);

/* The evaluation pass, GPT.forward's default call (gpt.py:375-537; the reference trainer's eval step): a padded batch through the
 * block stack with ALL its text and code rows, then both heads, the losses and the top-k accuracy.  The integer preparation
 * (gpt.py:404-474, 514-518: padding, start / stop tokens, targets, masks) is the caller's (genvc_amd.layers.gpt.forward_eval_prepare).
 *
 * gvc_gpt_forward_rows: rows of item b = [cond[b] (n_cond) | text_emb[text_ids[b][i]] + text_pos[i] (Lt) | mel_emb[code_ids[b][i]] +
 * mel_pos[i] (Lm)] (gpt.py:476-480, get_logits :275-280); causal attention combined with the key-padding mask key_mask uint8
 * [B][n_cond + Lt + Lm] (nonzero = attend, device, nullable = no mask: gpt.py:446-474 -- the mask a return_latent call does not
 * pass).  A masked key has weight exactly 0 for every query row; padded query rows are still computed.  latents_out [B][Lt + Lm][d] =
 * final_norm(ln_f(h)) of the rows behind the conditioning ones (get_logits :300-301).  Uses slots[b] as K/V scratch, as gvc_gpt_latents.
 * GVC_ERR_ARG: B > max_slots, B * (n_cond + Lt + Lm) > max_rows, Lt / Lm beyond the position tables, n_cond + Lt + Lm > max_seq.
 * GVC_ERR_UNSUPPORTED: a context with weight_dtype != 0 (evaluation is a reference-numerics job).
 *
 * gvc_gpt_head_xent: logits_out [R][V] = head(latents [R][d]) (head 0: text_head, V = n_text, needs text_head.* bound, else
 * GVC_ERR_STATE; head 1: mel_head, V = vocab), then per row r with target t = targets[r] (int32, -1 = ignored):
 *   row_terms[r] = (lse - x[t],  lse - mean_c x[c],  #{c : x[c] > x[t]} < top_k)        fp32 [R][3], zeros for ignored rows
 * and, summed over the rows in a fixed order in double (no atomics: the same input gives the same bits),
 *   sums[0] = ((1 - ls) sum nll + ls sum smoothing) / count   = F.cross_entropy(ignore_index=-1, label_smoothing=ls) (gpt.py:526-531)
 *   sums[1] = hits, sums[2] = count (hits / count = MulticlassAccuracy(top_k, average="micro", ignore_index=-1), gpt.py:166-172, 533),
 *   sums[3] = sum nll / count.                                                          double [4], device */
int gvc_gpt_forward_rows(gvc_gpt* ctx, const int32_t* slots, int32_t B, const float* cond, int32_t n_cond, const int32_t* text_ids,
                         int32_t Lt, const int32_t* code_ids, int32_t Lm, const uint8_t* key_mask, float* latents_out, gvc_stream s);
int gvc_gpt_head_xent(gvc_gpt* ctx, const float* latents, int32_t R, int32_t head, const int32_t* targets, float label_smoothing,
                      int32_t top_k, float* logits_out, float* row_terms, double* sums, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Sampling.  Replaces the per-step body of NewGenerationMixin.sample_stream
 * (layers/stream_generator.py:834-874): RepetitionPenalty -> Temperature -> TopK -> TopP ->
 * softmax -> draw, finished rows emit the pad token.
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_sample_params {
    float repetition_penalty;   /* 2.0 */
    float temperature;          /* 0.85 */
    float top_p;                /* 0.85; >= 1 disables */
    int32_t top_k;              /* 15; <= 0 disables; 1 = greedy (argmax of penalised logits) */
    int32_t eos_token;          /* stop_audio_token 1025 (also the pad) */
    int32_t vocab;              /* 1026 */
    uint64_t seed;              /* counter-based RNG key (torch.multinomial is not reproducible) */
} gvc_sample_params;

/* ids: int32 [B, ids_stride] row b holds the input_ids of the reference loop (fake prefix ids
 * 1..1,1024 followed by the generated tokens); ids_len[b] = current length (updated +1);
 * finished[b] in/out (1 once eos was emitted); step = RNG counter.  tok_out[b] receives the token. */
int gvc_sample(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
               int32_t* finished, const gvc_sample_params* p, int32_t step, int32_t* tok_out,
               gvc_stream s);

/* Per-row sampling settings and RNG key (no reference counterpart: the reference decodes one stream per call).  A row that
 * belongs to stream `rng_row` of a job keyed `seed` draws rng_uniform(seed, rng_step0 + i, rng_row) at step i of a call, so its
 * tokens do not depend on which other rows share the call or where in the batch it sits.  The layout is fixed: 32 bytes,
 * seed at offset 16. */
typedef struct gvc_row_sampling {
    float repetition_penalty, temperature, top_p;   /* as gvc_sample_params; temperature > 0 */
    int32_t top_k;                                  /* as gvc_sample_params; <= vocab */
    uint64_t seed;                                  /* RNG key of the row's stream */
    int32_t rng_row;                                /* the row's index inside ITS job (0 for a lone stream) */
    int32_t rng_step0;                              /* tokens this stream has already drawn (its RNG counter at step 0 of this call) */
} gvc_row_sampling;

/* gvc_sample with per-row settings and keys.  rows: HOST array of B (<= 64) entries, free for reuse when the call returns;
 * common supplies eos_token and vocab only (its other fields are ignored).  Row b draws rng_uniform(rows[b].seed,
 * rows[b].rng_step0 + step, rows[b].rng_row).  A row with top_k == 1 gets the argmax token gvc_sample gives it at top_k = 1. */
int gvc_sample_rows(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                    const gvc_sample_params* common, const gvc_row_sampling* rows, int32_t step, int32_t* tok_out,
                    gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Fused generation loop: prefill state -> n_steps x (sample, decode step) replayed from one
 * captured hipGraph with all step state on the device (no host sync per token; the reference
 * syncs at stream_generator.py:877).  Replaces GPT.generate / GPT.get_generator (gpt.py:594-621).
 *
 * Call after gvc_gpt_prefill[_cached] on the same slots (its logits / latent are parked per slot, as are those of the last
 * gvc_gpt_generate call: consecutive calls may batch different sets of slots).  Per step i in [0,n_steps): samples token i from
 * the current logits, stores it at tokens_out[b*tok_stride + i0 + i] and the latent that predicted
 * it at latents_out[(b*lat_stride + i0 + i)*d], then runs the decode step that consumes it.
 * ids / ids_len / finished as in gvc_sample (the caller initialises them from compute_embeddings).
 * max_keys = cached positions of the longest of these streams once the call has run (prefix + 1 + steps so far + n_steps);
 * the library picks the kernel variant for that context length and returns GVC_ERR_STATE when it would overflow the KV
 * cache (max_seq).  0 = unknown: ids_stride (which must then cover the whole run of the stream) is taken as the bound.
 * On a full MI355X (256 CUs) the decode step of ONE stream is ONE launch (csrc/persist_kernel.h; fp32, bf16 weights, bf16 weights
 * + bf16 KV cache; d_model 1024 or 512 for the bf16 modes) and the step of 2..16 streams runs its whole block stack in ONE launch
 * (csrc/persist_rows.h; d_model 1024, 4 heads of 256, an even layer count); other shapes and batch sizes take the
 * launch-per-phase paths.  A hand-off of a one-launch step that times out (not all of its 256 workgroups resident: another
 * process or stream holds CUs) is reported ONCE -- by gvc_gpt_health, else by the next call -- as GVC_ERR_TIMEOUT, and the context
 * continues on the launch-per-phase paths (see gvc_gpt_health).  Eight consecutive steps are captured per graph.
 * ------------------------------------------------------------------------------------------ */
int gvc_gpt_generate(gvc_gpt* ctx, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride,
                     int32_t* ids_len, int32_t* finished, const gvc_sample_params* p, int32_t i0,
                     int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out,
                     int32_t lat_stride, gvc_stream s);

/* gvc_gpt_generate with per-row settings and RNG keys (see gvc_row_sampling): rows is a HOST array of B (<= 64) entries, copied
 * into the call's device state by the call's first launch (a kernel argument: the caller may reuse the array as soon as the call
 * returns; no allocation and no synchronisation per call).  common supplies eos_token and vocab only.  Tokens and latents land
 * at column i0 + i as in gvc_gpt_generate; only the RNG counter is per row (rng_step0 + i).  The same captured step graphs serve
 * both calls: the greedy sampler when every row has top_k == 1, the sampling one otherwise (gvc_gpt_warmup with top_k 1 / not 1).
 * With rows[b] = {p's settings, p->seed, b, i0} for every b the result is bit-identical to gvc_gpt_generate(p, i0). */
int gvc_gpt_generate_rows(gvc_gpt* ctx, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                          int32_t* finished, const gvc_sample_params* common, const gvc_row_sampling* rows, int32_t i0,
                          int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out,
                          int32_t lat_stride, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Deterministic beam search (HF generate(num_beams=K, do_sample=False); reference layers/gpt.py:594-609 hands num_beams /
 * length_penalty to HF generate, trainers/hifigan_trainer.py:457-500 forwards them, layers/gpt_inference.py:84-89 widens the
 * prefix to B x K rows and :126-136 reorders the KV cache by beam).  Here the KV cache is not reordered: a beam is a slot, and a
 * reorder is a permutation of the slot table plus at most K-1 span copies per item.
 *
 * Per step and item b (one workgroup): s = log_softmax(logits) in fp32 over the vocab of each of its K beam rows; repetition
 * penalty on the log-probs over the ids of the beam's input_ids row (s < 0 ? s * p : s / p, each id once); s += running score;
 * top-2K of the K x vocab candidates (descending); walk them in rank order: an eos candidate at rank < K becomes a finished
 * hypothesis with score / len ** length_penalty, kept in a set of at most K (BeamHypotheses.add), an eos candidate at rank >= K is
 * skipped, the first K other candidates become the next beams.  The item is done once its set is full and its worst kept score is
 * >= best / len ** length_penalty.  length_mode 0 ("4.33", transformers 4.33 = the reference's pin): len = n0 + t for both, best =
 * the best candidate of the step; 1 ("generated", transformers >= 4.50): len = t + 1 for both, best = the best next beam; t =
 * tokens generated before the step.  A done item keeps its beams: tokens = eos, parents = identity, no copies.
 * early_stopping (bits 8..15 of length_mode, so the struct keeps its size and a caller that sets the mode alone gets False): 0 False,
 * the test above; 1 True, the item is done as soon as its set is full (BeamHypotheses.is_done of 4.33; in the installed _beam_search a
 * full set takes no further hypothesis); 2 "never", the test above with len replaced by the longest possible length when
 * length_penalty > 0 -- n0 + max_new in mode 0 (4.33's max_length), max_new in mode 1 (max_length - decoder_prompt_len) -- and
 * unchanged otherwise.  The hypotheses' own normalisation is not affected.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t B, K;                   /* items, beams per item: 2 <= K <= 16, K * vocab <= 16 * 1026 */
    int32_t vocab, eos;
    int32_t n0;                     /* prompt length = positions of the fake ids (compute_embeddings) = KV positions after the prefill */
    int32_t ids_stride;             /* >= n0 + max_new */
    int32_t max_new;                /* hypothesis capacity in tokens (max_gen_mel_tokens) */
    int32_t length_mode;            /* bits 0..7: 0 "4.33", 1 "generated"; bits 8..15: early_stopping 0 False, 1 True, 2 "never" */
    float length_penalty, repetition_penalty;
    int32_t* ids;                   /* [2][B*K][ids_stride] input_ids rows, double-buffered: step t reads buffer t & 1 (positions
                                       [0, n0 + t)) and writes buffer (t + 1) & 1 gathered by parent, plus the new token at n0 + t */
    float* scores;                  /* [B*K] running sums of the beams (start: 0 for beam 0, -1e9 for the others) */
    int32_t* tokens;                /* [B*K] out: token of each next beam (the input of the next decode step) */
    int32_t* parents;               /* [B*K] out: beam (0..K-1 within the item) each next beam continues */
    int32_t* done;                  /* [B] item done (0 / 1) */
    float* hyp_score;               /* [B][K] finished hypotheses: normalised score */
    int32_t* hyp_len;               /* [B][K] ... generated tokens, eos excluded */
    int32_t* hyp_tok;               /* [B][K][max_new] ... the tokens */
    int32_t* hyp_count;             /* [B] hypotheses kept (start 0) */
    float* hyp_worst;               /* [B] worst kept score (start 1e9) */
    int32_t* copies;                /* [B][K][3] (src slot, dst slot, first position) of the KV spans the reorder needs */
    int32_t* n_copies;              /* [B] copies of the last step (<= K - 1) */
} gvc_beam_state;

/* One select step on caller-given logits [B*K][vocab] (device), state st (device arrays), slots [B*K] (device, in/out: the KV slot of
 * each beam row; rewritten by the slot permutation: a parent's slot goes to its first child, further children take the slots of
 * childless parents, each such take is a copies entry) at step t (t tokens generated before).  The KV cache itself is not touched.
 * For tests and for callers that decode themselves. */
int gvc_beam_select(const gvc_beam_state* st, const float* logits, int32_t* slots, int32_t t, gvc_stream s);

/* n_steps beam steps [select -> KV span copies -> decode step over B*K rows], replayed from captured graphs (eight steps per graph,
 * as gvc_gpt_generate) with all state on the device.  The caller has prefilled item b into slots[b*K] (gvc_gpt_prefill) and
 * initialised st (i0 == 0); slots[b*K+1 .. b*K+K-1] are free slots the first step fans the prefix out to (the item is prefilled
 * once).  Step i of the call is step t = i0 + i of the search; slots is rewritten to the beams' slots at return; consecutive calls
 * continue the search.  max_keys as in gvc_gpt_generate (n0 + i0 + n_steps).  Status codes as gvc_gpt_generate: a hand-off
 * time-out is reported by gvc_gpt_health / the next call as GVC_ERR_TIMEOUT and the search must be repeated from its prefill. */
int gvc_gpt_beam_generate(gvc_gpt* ctx, int32_t* slots, const gvc_beam_state* st, int32_t i0, int32_t n_steps, int32_t max_keys,
                          gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Length and repetition logits processors (HF generate kwargs; the reference hands them to HF generate, layers/gpt.py:594-621).
 * One set per call, for every row.  Applied after the repetition penalty, in the order HF's _get_logits_processor builds them:
 *   no_repeat_ngram_size -> min_length -> min_new_tokens -> exponential_decay_length_penalty -> suppress_tokens ->
 *   begin_suppress_tokens -> [sampling only: temperature -> top_k -> top_p] -> min_p (sampling only).
 * Lengths are those of the row's input_ids (fake prompt included): len = the row's length before the step, plen = its prompt
 * length.  no_repeat_ngram_size n: every window of n ids of the whole row whose first n-1 ids equal the row's last n-1 ids bans its
 * last id (nothing while len < n).  min_length: eos -inf while len < min_length.  min_new_tokens: eos -inf while len - plen <
 * min_new_tokens.  Decay (start, factor): once len > plen + start, s_eos += |s_eos| * (factor ** (len - plen - start) - 1) (a
 * banned eos stays -inf; HF would make it NaN).  suppress: those ids -inf at every step; begin_suppress: at the step with
 * len == plen.  min_p: after top-p, ids with exp(s - max) < min_p are dropped (the top one always stays).  With beams the
 * processors act on each beam's penalised log-probs before the running score is added, and plen = the state's n0.
 * An all-zero struct is "every processor off": every kernel then computes exactly what it computes without one.
 * ------------------------------------------------------------------------------------------ */
#define GVC_PROC_MAX_NGRAM 8            /* no_repeat_ngram_size cap: the ban scans the row once per step, n-1 compares per window */
#define GVC_PROC_VOCAB_WORDS 33         /* bitmap words: vocab <= 1056 */
typedef struct gvc_logits_processors {
    int32_t no_repeat_ngram_size;       /* 0 off; 1..GVC_PROC_MAX_NGRAM */
    int32_t min_length;                 /* 0 off */
    int32_t min_new_tokens;             /* 0 off */
    int32_t decay_start;                /* exponential_decay_length_penalty start (new tokens) */
    float decay_factor;                 /* exponential_decay_length_penalty factor: 0 off, else > 0 */
    float min_p;                        /* 0 off, else in (0, 1]; ignored by the greedy (top_k == 1) sampler and by beams */
    int32_t prompt_len;                 /* plen of every row when prompt_lens is null */
    int32_t n_suppress;                 /* ids set in suppress (0: skip the bitmap) */
    int32_t n_begin_suppress;           /* ids set in begin_suppress */
    int32_t reserved;                   /* 0 */
    const int32_t* prompt_lens;         /* nullable DEVICE [B]: plen per row (rows / rolling decodes); must outlive the call's work */
    uint32_t suppress[GVC_PROC_VOCAB_WORDS];        /* bit x of word x / 32: id x suppressed */
    uint32_t begin_suppress[GVC_PROC_VOCAB_WORDS];
} gvc_logits_processors;

/* gvc_sample / gvc_sample_rows with processors: rows (nullable HOST array of B entries) as gvc_sample_rows, null = p's settings for
 * every row; proc (HOST) is staged on the stream for this call.  top_k == 1 rows go to the argmax kernel as in gvc_sample. */
int gvc_sample_proc(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                    const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* proc, int32_t step,
                    int32_t* tok_out, gvc_stream s);
/* gvc_gpt_generate (rows null) or gvc_gpt_generate_rows (rows set) with processors.  proc (HOST, nullable) travels by value in the
 * call's first launch into the device-resident call state, as rows do: the same captured step graphs, no allocation and no
 * synchronisation per call.  proc null: exactly gvc_gpt_generate / gvc_gpt_generate_rows. */
int gvc_gpt_generate_proc(gvc_gpt* ctx, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                          int32_t* finished, const gvc_sample_params* p, const gvc_row_sampling* rows,
                          const gvc_logits_processors* proc, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out,
                          int32_t tok_stride, float* latents_out, int32_t lat_stride, gvc_stream s);
/* gvc_beam_select / gvc_gpt_beam_generate with processors (proc HOST, nullable: null = the calls without it).  min_p and
 * prompt_len / prompt_lens are ignored (beams are deterministic; the prompt is st->n0). */
int gvc_beam_select_proc(const gvc_beam_state* st, const gvc_logits_processors* proc, const float* logits, int32_t* slots, int32_t t,
                         gvc_stream s);
int gvc_gpt_beam_generate_proc(gvc_gpt* ctx, int32_t* slots, const gvc_beam_state* st, const gvc_logits_processors* proc, int32_t i0,
                               int32_t n_steps, int32_t max_keys, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Group (diverse) beam search (HF generate(num_beams=K, num_beam_groups=G, diversity_penalty=lambda, do_sample=False); the reference
 * hands every kwarg to HF generate, layers/gpt.py:594-609, and its pinned dispatcher routes the mode, layers/stream_generator.py:308-317,
 * 512-556).  The semantics are transformers 4.33's group_beam_search, HammingDiversityLogitsProcessor and BeamSearchScorer with
 * num_beam_groups, restated from the published source.  The K beams of an item are G groups of S = K / G: rows
 * b*K + g*S + i belong to group g.  The running score starts at 0 for the first beam of every group and at -1e9 for the others.  Per
 * step the groups run in order inside one launch; for the S rows of group g: s = log_softmax(logits); for g > 0, s[x] -= lambda * f[x],
 * f[x] = how often token x was chosen at this step by the rows of groups 0..g-1 of the item (a done group: eos S times; eos is
 * penalised like any x); then the repetition penalty, the processors and the running score as in the plain search; top-2S of the group's
 * S x vocab candidates, walked as the plain search walks 2K with K replaced by S: the kept set (capacity S), its count, its worst score
 * and the done flag are the (item, group)'s; parents are beams of the same group.  A done group keeps its beams (tokens = eos, parents
 * = identity, no copies); the item (st->done) is done when all its groups are.  The state is a gvc_beam_state whose hypothesis store
 * [B][K] reads [B][G][S]; st->hyp_count / st->hyp_worst are written for G == 1 only (then every output equals the plain search's).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t G;                      /* groups per item: 1 <= G <= K, K % G == 0 */
    float diversity_penalty;        /* lambda: finite, >= 0 */
    int32_t* done;                  /* [B][G] group done (0 / 1; start 0) */
    int32_t* hyp_count;             /* [B][G] hypotheses kept by the group (start 0) */
    float* hyp_worst;               /* [B][G] worst kept score of the group (start 1e9) */
} gvc_beam_groups;

/* gvc_beam_select / gvc_beam_select_proc for a group search (proc HOST, nullable).  st->parents are beams within the item (0..K-1, inside
 * the row's group); the slot permutation runs per group, so a step makes at most K - G copies per item.  At t == 0 the copies of a G > 1
 * search start at n0 (the caller has fanned the prefix out to every slot); G == 1 computes gvc_beam_select bit for bit. */
int gvc_group_beam_select(const gvc_beam_state* st, const gvc_beam_groups* grp, const gvc_logits_processors* proc, const float* logits,
                          int32_t* slots, int32_t t, gvc_stream s);
/* gvc_gpt_beam_generate / gvc_gpt_beam_generate_proc for a group search (proc HOST, nullable): [group select -> KV span copies -> decode
 * step over B*K rows] from captured graphs of their own kind.  The caller has prefilled item b into slots[b*K]; with G > 1 the call
 * with i0 == 0 first fans that slot out to the item's other K-1 slots (as gvc_gpt_kv_fanout), so every group starts from a whole prefix.
 * K % G != 0, G > K, K > 16 and a lambda that is not finite or below 0 are GVC_ERR_ARG.  Status codes as gvc_gpt_beam_generate. */
int gvc_gpt_group_beam_generate(gvc_gpt* ctx, int32_t* slots, const gvc_beam_state* st, const gvc_beam_groups* grp,
                                const gvc_logits_processors* proc, int32_t i0, int32_t n_steps, int32_t max_keys, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Contrastive search (HF generate(top_k=K > 1, do_sample=False, penalty_alpha=a > 0); reference layers/gpt.py:594-609 hands every kwarg
 * to HF generate, whose pinned 4.33 selects this mode by that test, layers/stream_generator.py:264-270 restates it and :366-385 routes it
 * to contrastive_search without a logits warper).  The semantics are transformers 4.33's contrastive_search + _ranking_fast:
 *   prefill: ctx = ln_f of EVERY prompt row (hidden_states[-1], not the final_norm latent); logits = the last row's.
 *   step t (t tokens generated before it), item b: s = processors(ids row, logits) (repetition penalty on the raw logits, then the
 *   gvc_logits_processors in HF's order; no warper: temperature, top_p, min_p ... have no effect); p = softmax(s) in fp32; the top-K
 *   (p_k, x_k) descending; the K candidates run one decode step each from the item's KV (rows b*K + k of a B*K-row step, at the cache and
 *   mel positions greedy step t uses); h_k = ln_f of candidate k's residual; pen_k = max_j cos(ctx_j, h_k) over the n0 + t context rows;
 *   score_k = (1 - a) p_k - a pen_k; k* = the first argmax.  Token = x_{k*}, or eos (= pad) once the item has finished; ctx gains h_{k*},
 *   the item's KV keeps candidate k*'s row, the next logits are candidate k*'s.  finished |= token == eos.
 * A candidate is a KV slot (the item's K slots hold identical K/V between steps): after the ranking the slot of k* is copied to the
 * other K-1 slots for the one new position (k_kv_copy_span, as beams reorder).  DESIGN.md 4.10.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t B, K;                   /* items, candidates per item: 2 <= K <= 16, B * K <= the context's slots */
    int32_t vocab, eos;
    int32_t n0;                     /* prompt length = positions of the fake ids (compute_embeddings) = KV positions after the prefill */
    int32_t ids_stride;             /* >= n0 + max_new */
    int32_t max_new;                /* tokens_out / latents_out capacity per item */
    float penalty_alpha;            /* a: finite, > 0 (a > 1 is accepted, as HF accepts it) */
    float repetition_penalty;       /* > 0; 1 = off */
    int32_t reserved;               /* 0 */
    int32_t* ids;                   /* [B][ids_stride] input_ids rows: the n0 fake ids at the start; step t writes column n0 + t */
    int32_t* finished;              /* [B] 0 / 1 (start 0) */
    int32_t* tokens_out;            /* [B][max_new]: token of step t at column t */
    float* latents_out;             /* nullable [B][max_new][d]: step t's final_norm latent of the chosen candidate (what predicts the next
                                       token, as gvc_gpt_generate's latents) */
    const float* hidden0;           /* [B][n0][d] ln_f of the prompt rows (gvc_gpt_prefill_hidden); read by the call with i0 == 0 */
} gvc_contrastive_state;

/* gvc_gpt_prefill(logits_out = NULL) that also writes hidden_out [B][P+1][d] = ln_f of every row it computed (the P prefix rows and the
 * start token): the context rows of a contrastive search.  The logits and latent are parked per slot as gvc_gpt_prefill parks them. */
int gvc_gpt_prefill_hidden(gvc_gpt* ctx, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P, int32_t start_tok,
                           float* hidden_out, gvc_stream s);
/* n_steps contrastive steps [recall -> decode step over B*K rows -> hidden rows -> similarity -> select -> KV span copies], replayed from
 * captured graphs (eight steps per graph) with all state on the device.  The caller has prefilled item b into slots[b*K]
 * (gvc_gpt_prefill_hidden, its hidden rows in st->hidden0) and initialised st (i0 == 0: ids rows, finished = 0); slots[b*K+1 ..
 * b*K+K-1] are free slots the call with i0 == 0 fans the prefix out to.  slots are not permuted.  Step i of the call is step t = i0 + i;
 * consecutive calls continue the search (the context rows live in the context between them).  max_keys as in gvc_gpt_beam_generate.
 * proc (HOST, nullable; min_p and prompt_len ignored: the prompt is st->n0) travels by value into the device-resident call state.
 * Status codes as gvc_gpt_beam_generate. */
int gvc_gpt_contrastive_generate(gvc_gpt* ctx, const int32_t* slots, const gvc_contrastive_state* st, int32_t i0, int32_t n_steps,
                                 int32_t max_keys, gvc_stream s);
int gvc_gpt_contrastive_generate_proc(gvc_gpt* ctx, const int32_t* slots, const gvc_contrastive_state* st, const gvc_logits_processors* proc,
                                      int32_t i0, int32_t n_steps, int32_t max_keys, gvc_stream s);
/* gvc_gpt_warmup for gvc_gpt_contrastive_generate over B items of K candidates: the context-row buffers and the step graphs of every
 * context class up to max_keys cached positions (and everything gvc_gpt_warmup(B*K) prepares).  Afterwards such calls neither allocate
 * nor synchronise */
int gvc_gpt_warmup_contrastive(gvc_gpt* ctx, int32_t B, int32_t K, int32_t max_keys);

/* Per-row processor sets: row b uses sets[set_of_row[b]], or no processors at all when the index is -1 (such a row computes exactly
 * what it computes in the call without processors).  sets (n_sets entries, 1 <= n_sets <= B <= 64) and set_of_row (B entries, each in
 * [-1, n_sets)) are HOST arrays, free again when the call returns; GVC_ERR_ARG otherwise, and every set is checked as proc is.  A set's
 * prompt length rule is proc's: prompt_lens[b] (device, indexed by the row's place in the call) when set, else prompt_len.  rows
 * (nullable HOST) as in gvc_sample_proc / gvc_gpt_generate_proc.
 * gvc_gpt_generate_proc_sets stages each set some row uses into the device-resident call state in launches of its own (four sets per
 * launch) ahead of the call's first launch, which carries the indices: the same captured step graphs, no allocation and no
 * synchronisation per call.  Not on the beam path. */
int gvc_sample_proc_sets(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                         const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets, int32_t n_sets,
                         const int32_t* set_of_row, int32_t step, int32_t* tok_out, gvc_stream s);
int gvc_gpt_generate_proc_sets(gvc_gpt* ctx, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                               int32_t* finished, const gvc_sample_params* p, const gvc_row_sampling* rows,
                               const gvc_logits_processors* sets, int32_t n_sets, const int32_t* set_of_row, int32_t i0, int32_t n_steps,
                               int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride,
                               gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Entropy-aware sampling warpers (HF typical_p, epsilon_cutoff, eta_cutoff), applied by the sampling kernel after min_p and before
 * the draw, in that order, each to the scores the previous step left (masked ids are -inf; p = softmax over the survivors):
 *   typical_p m: logp = log_softmax(s), H = -sum p logp, key = |-logp - H|.  T = the smallest key whose ids with key <= T hold mass
 *                >= m (the largest key if none does); every id with key <= T stays, ties included.  May drop the argmax.
 *   epsilon_cutoff e: ids with p < e are dropped, except those whose score equals the largest surviving score.
 *   eta_cutoff e: H = the survivors' entropy; the epsilon rule with min(e, sqrt(e) * exp(-H)).
 * 0 is "off" for each; on values lie in (0, 1) (HF: typical_p >= 1 and cutoffs outside (0, 1) are off, typical_p <= 0 raises: the
 * caller maps those).  An all-zero struct computes exactly what the call without it computes.  The argmax sampler (top_k == 1 rows,
 * every greedy call) and beams never read them: one candidate is left, and every warper keeps one.
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_logits_warpers {
    float typical_p;                    /* 0 off, else in (0, 1) */
    float epsilon_cutoff;               /* 0 off, else in (0, 1) */
    float eta_cutoff;                   /* 0 off, else in (0, 1) */
    int32_t reserved;                   /* 0 */
} gvc_logits_warpers;

/* Processor sets with warpers: row b uses sets[set_of_row[b]] and warps[set_of_row[b]], neither when the index is -1.  sets (nullable:
 * no processors for any row), warps (nullable: no warpers) and set_of_row (nullable: every row uses entry 0) are HOST arrays as in
 * gvc_sample_proc_sets, n_sets entries each (1 <= n_sets <= B <= 64); a bad value is GVC_ERR_ARG.  With warps null these are
 * gvc_sample_proc_sets / gvc_gpt_generate_proc_sets (sets null too: the calls without processors).  gvc_gpt_generate_warp stages the
 * warpers into the device-resident call state in one launch of its own ahead of the call's first launch: the same captured step
 * graphs, no allocation and no synchronisation per call.  Not on the beam path. */
int gvc_sample_warp(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                    const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                    const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, int32_t step, int32_t* tok_out,
                    gvc_stream s);
int gvc_gpt_generate_warp(gvc_gpt* ctx, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                          int32_t* finished, const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                          const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, int32_t i0, int32_t n_steps,
                          int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride,
                          gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Classifier-free guidance (HF guidance_scale; transformers generation/logits_process.py,
 * UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__):
 *     scores = log_softmax(scores, dim=-1)
 *     unconditional_logits = log_softmax(logits[:, -1], dim=-1)
 *     scores_processed = guidance_scale * (scores - unconditional_logits) + unconditional_logits
 * HF puts this processor first in the list (generation/utils.py, _get_logits_processor), so every other processor, the warpers and
 * the draw see scores_processed in the place of the raw logits.  The model's prompt is an embedded prefix, so the unconditional
 * pass is a second prefilled KV slot per item (another conditioning, e.g. the source speaker) that is fed the item's tokens.
 *
 * gvc_cfg_guide: out[b][v] from logits_cond[b] and logits_uncond[b] ([B][vocab] device rows, vocab <= 2048), fp32, in the operation
 * order above; the row maximum comes off before exp, so finite inputs of any range give finite outputs.
 * gvc_gpt_generate_cfg: gvc_gpt_generate_warp over B items (2B <= max_slots, 2B <= 64).  slots[b] is item b's conditional slot,
 * uncond_slots[b] its unconditional one (device arrays; both prefilled).  One step = [guide; sample over B rows on the guided
 * scores with ids / processors / keys of the conditional rows; token b to both rows; one decode step over the 2B rows -- the
 * one-launch rows step for 2..16 rows where it applies, never the one-stream step].  latents_out are the conditional rows'.
 * The next-step logits and latents of all 2B slots are parked between calls, so a generation split into calls (i0 > 0) continues
 * exactly; pending deferred tokens of the slots are flushed first.  scale must be finite (scale == 1 computes log_softmax(cond):
 * callers that want the unguided path call gvc_gpt_generate_warp).  The graphs are captured on first use or by gvc_gpt_warmup_cfg,
 * after which a call of that shape neither allocates nor synchronises.
 * ------------------------------------------------------------------------------------------ */
int gvc_cfg_guide(const float* logits_cond, const float* logits_uncond, int32_t B, int32_t vocab, float scale, float* out, gvc_stream s);
int gvc_gpt_generate_cfg(gvc_gpt* ctx, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                         int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                         const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                         int32_t n_sets, const int32_t* set_of_row, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out,
                         int32_t tok_stride, float* latents_out, int32_t lat_stride, gvc_stream s);
/* ------------------------------------------------------------------------------------------
 * Per-step scores and logits (HF return_dict_in_generate with output_scores / output_logits; transformers
 * generation/utils.py, GenerationMixin._sample and compute_transition_scores).
 *
 * gvc_gpt_generate_scores: gvc_gpt_generate_warp (uncond_slots null; scale is then ignored) or gvc_gpt_generate_cfg (uncond_slots set)
 * that also stores what each step decoded from.  scores_out / logits_out: device buffers [B][out_stride][vocab] fp32, either may be
 * null; step i of the call lands at [b][i0 + i], as in tokens_out, and i0 + n_steps <= out_stride.
 *   scores_out  the row logits_processor(input_ids, logits) returns in HF: behind the guidance, the repetition penalty and the
 *               processors.  do_sample != 0: also behind Temperature and every warper (TopK, TopP, MinP, Typical, Epsilon, Eta), dropped
 *               entries -inf, kept ones at their temperature-scaled score, not renormalised; top_k == 1 gives TopK's row at k = 1
 *               (ties with the maximum kept).  do_sample == 0 (greedy search, top_k == 1): the full processed row, no temperature.
 *   logits_out  the raw head output of the step; under guidance the conditional row.
 * Rows that have stopped keep decoding the stop token and keep storing rows.  do_sample decides nothing else: the tokens, ids and
 * latents are those of the call without the buffers, bit for bit, and the same captured step graphs serve both.
 *
 * gvc_transition_scores: out[r][t] = scores[r][t][tokens[r][t]] (normalize 0) or log_softmax(scores[r][t])[tokens[r][t]] (normalize 1:
 * the maximum comes off before exp, -inf entries add nothing, the sum runs in a fixed order).  scores: row r starts row_stride floats
 * after row r - 1 and holds n dense [V] rows (row_stride >= n * V: a scores_out buffer's out_stride * vocab); tokens int32 [R][n] and
 * out fp32 [R][n] are dense.  A token outside [0, V) gives NaN.
 * ------------------------------------------------------------------------------------------ */
int gvc_gpt_generate_scores(gvc_gpt* ctx, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                            int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                            const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                            int32_t n_sets, const int32_t* set_of_row, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out,
                            int32_t tok_stride, float* latents_out, int32_t lat_stride, float* scores_out, float* logits_out,
                            int32_t out_stride, int32_t do_sample, gvc_stream s);
int gvc_transition_scores(const float* scores, int64_t row_stride, const int32_t* tokens, int32_t R, int32_t n, int32_t V,
                          int32_t normalize, float* out, gvc_stream s);
/* ------------------------------------------------------------------------------------------
 * Sequence bias, bad words, forced EOS and renormalised scores (HF sequence_bias, bad_words_ids, forced_eos_token_id,
 * renormalize_logits; transformers generation/logits_process.py: SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor,
 * ForcedEOSTokenLogitsProcessor, LogitNormalization), on the sampler kernels.  One call-wide struct; HF's order
 * (generation/utils.py, _get_logits_processor) is
 *   guidance -> SEQUENCE BIAS -> repetition penalty -> no_repeat_ngram -> BAD WORDS -> min_length -> min_new_tokens -> FORCED EOS ->
 *   exponential decay -> suppress -> begin_suppress -> [sampling: temperature, top_k, top_p, min_p, typical, epsilon, eta] ->
 *   LOGIT NORMALIZATION.
 * Entry e is the id sequence ids[e][0 .. len[e]) with the value bias[e]; it HITS a row when its first len - 1 ids equal the row's
 * last len - 1 input ids (the fake prompt ids count; len == 1 always hits; an entry longer than the row never hits).
 *   sequence bias  entries [0, n_bias), length-1 entries first, then the caller's order: x = logit + (0 + bias of every hit entry
 *                  that ends in this id, added in entry order), one fp32 add per term, ahead of the repetition penalty.
 *   bad words      entries [n_bias, n_bias + n_ban): the last id of every hit entry is -inf (their bias field is not read).
 *   forced EOS     force_eos_at = N > 0: at the step where the row holds N - 1 new tokens (len - prompt_len == N - 1) every score is
 *                  -inf and the stop token's is 0.0, whatever the bans above say; the decay, suppress, the temperature and the
 *                  warpers then run as ever.  N is the call's max_new_tokens.
 *   renormalize    the scores_out row of a step is log_softmax of the row stored without it: the maximum comes off before exp, -inf
 *                  entries stay -inf and add nothing, the sum runs in a fixed order.  Read only where a scores row is stored.  THE
 *                  TOKENS ARE THOSE OF THE CALL WITHOUT IT, BIT FOR BIT: the draw and the argmax read the un-normalised row (in HF
 *                  the draw reads the normalised one; the two distributions differ by rounding only).
 * Ids lie in [0, vocab) -- HF's list form of sequence_bias refuses id 0 and its dict form does not; 0 is accepted here in both, the
 * one deviation.  Values are finite or -inf.  The all-zero struct is "off" and computes exactly what the call without it computes.
 * ------------------------------------------------------------------------------------------ */
#define GVC_BIAS_MAX_SEQS 32
#define GVC_BIAS_MAX_LEN 8
typedef struct gvc_logits_bias {
    int32_t n_bias;                     /* entries [0, n_bias): sequence_bias, length-1 entries first, then dict order */
    int32_t n_ban;                      /* entries [n_bias, n_bias + n_ban): bad words; n_bias + n_ban <= GVC_BIAS_MAX_SEQS */
    int32_t force_eos_at;               /* 0 off, else max_new_tokens: the stop token is forced at len - prompt_len == force_eos_at - 1 */
    int32_t renormalize;                /* 0 / 1; read only where a scores row is stored */
    int32_t prompt_len;                 /* prompt length of every row (read with force_eos_at) */
    int32_t reserved[3];                /* 0 */
    int32_t len[GVC_BIAS_MAX_SEQS];     /* 1..GVC_BIAS_MAX_LEN */
    float bias[GVC_BIAS_MAX_SEQS];      /* finite or -inf */
    int32_t ids[GVC_BIAS_MAX_SEQS][GVC_BIAS_MAX_LEN];
} gvc_logits_bias;

/* gvc_sample_bias: gvc_sample_warp with the struct above (HOST, nullable: null is gvc_sample_warp; sets / warps / set_of_row all null
 * then mean no processors, n_sets is ignored).  gvc_gpt_generate_bias: gvc_gpt_generate_scores with it; bias null is exactly
 * gvc_gpt_generate_scores.  The struct travels into the device-resident call state in one staging launch of its own (1.3 KB of kernel
 * argument) ahead of the call's first launch: the same captured step graphs, no allocation and no synchronisation per call.
 * GVC_ERR_ARG: counts outside the caps, a len outside 1..8, an id outside the vocabulary, a NaN or +inf bias, force_eos_at or
 * prompt_len < 0, renormalize other than 0 / 1, reserved != 0.  Not on the beam or contrastive paths. */
int gvc_sample_bias(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                    const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                    const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, int32_t step,
                    int32_t* tok_out, gvc_stream s);
int gvc_gpt_generate_bias(gvc_gpt* ctx, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                          int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                          const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                          int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, int32_t i0, int32_t n_steps,
                          int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride,
                          float* scores_out, float* logits_out, int32_t out_stride, int32_t do_sample, gvc_stream s);
/* ------------------------------------------------------------------------------------------
 * Repetition-aware sampling (RAS; VALL-E 2, and the default decoder of CosyVoice with window 10 and ratio 0.1), on the full sampling
 * kernel.  Per row and step, after the chain above has picked its token x exactly as without RAS:
 *   n_gen = len - prompt_len (the fake prompt ids never count), w = min(window, n_gen), c = how many of the row's last w generated
 *   ids equal x.  When c >= min_count, x is not the stop token, the row is not finished and its ids buffer is not full, x is thrown
 *   away and drawn again from the row as the chain left it AHEAD OF TRUNCATION: every finite score behind the sequence bias, the
 *   repetition penalty, the processors and Temperature (-inf entries -- suppressed ids, a banned EOS, bad words -- stay impossible),
 *   with the arithmetic of the first draw: weights expf(s - max) in fp32 widened to double, running mass in double in vocabulary
 *   order, first index whose mass reaches u2 * total, else the last finite index.  The redraw may return x again.
 *   u2 = rng_uniform(seed ^ GVC_RAS_SALT, step, row) with the seed, step and row of the first draw (the row's own key when keyed).
 * Otherwise x stands and the step is that of the call without RAS, bit for bit.  The caller turns a ratio into integers:
 * min_count = max(1, ceil(ratio * window - 1e-9)); the device compares integers only.  top_k == 1 is served ("greedy with an
 * escape"): x is the argmax and the redraw runs at the call's temperature; such a call runs on the full kernel, never on the argmax
 * kernel.  Per-step scores and logits (gvc_gpt_generate_scores) are those of the first draw: RAS changes the token only.
 * A null table, a -1 index or window == 0 computes exactly what the call without it computes.
 * ------------------------------------------------------------------------------------------ */
#define GVC_RAS_MAX_WINDOW 64
#define GVC_RAS_SALT 0x5241535F52454452ull          /* "RAS_REDR" */
typedef struct gvc_logits_ras {
    int32_t window;                     /* 0 off, else 1..GVC_RAS_MAX_WINDOW */
    int32_t min_count;                  /* >= 1 where the window is on */
    int32_t prompt_len;                 /* prompt length of the rows of this entry (fake ids included), as gvc_logits_processors' */
    int32_t reserved;                   /* 0 */
} gvc_logits_ras;

/* gvc_sample_ras: gvc_sample_bias with a RAS table; gvc_gpt_generate_ras: gvc_gpt_generate_bias with one.  ras (HOST, nullable: null
 * is exactly the call without it): n_sets entries (1 <= n_sets <= B <= 64, as for sets and warps) indexed like warps -- row b uses ras[set_of_row[b]], none for
 * -1, entry 0 for every row when set_of_row is null.  ras_redraws (DEVICE, nullable): int32 [B], the step that redraws row b adds 1
 * to entry b; the caller zeroes it.  The table travels into the device-resident call state in one staging launch of its own (1 KB of
 * kernel argument) ahead of the call's first launch, so nothing is allocated or synchronised per call; the step graphs are the
 * sampling ones whatever top_k is (gvc_gpt_warmup with a top_k other than 1 prepares them).  GVC_ERR_ARG: a window outside
 * [0, 64], min_count < 1 with the window on, prompt_len < 0, reserved != 0, n_sets outside [1, B].  Not on the beam, contrastive,
 * assisted or lookup paths. */
int gvc_sample_ras(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                   const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                   const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias,
                   const gvc_logits_ras* ras, int32_t* ras_redraws, int32_t step, int32_t* tok_out, gvc_stream s);
int gvc_gpt_generate_ras(gvc_gpt* ctx, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                         int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                         const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                         int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, const gvc_logits_ras* ras,
                         int32_t* ras_redraws, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride,
                         float* latents_out, int32_t lat_stride, float* scores_out, float* logits_out, int32_t out_stride,
                         int32_t do_sample, gvc_stream s);
/* ------------------------------------------------------------------------------------------
 * Presence, frequency and windowed repetition penalties (the OpenAI / vLLM definition of the first two), on both sampler kernels.
 * Counts of a row at a step:
 *   n_gen = len - prompt_len (the fake prompt ids never count, as for RAS);
 *   w = n_gen when window == 0, else min(window, n_gen);
 *   c_i = how often id i occurs among the row's last w generated ids, ids[len - w .. len); ids outside [0, vocab) are ignored.
 * For every i with c_i > 0: score_i -= frequency * c_i + presence, in fp32 with this operation order and no fused multiply-add:
 *   t = fl(fl(frequency * float(c_i)) + presence), score_i = fl(score_i - t).
 * Place in the chain: directly behind RepetitionPenalty -- behind SequenceBias, ahead of the n-gram, length and suppress processors,
 * the EOS decay and Temperature.  Under guidance they act on the guided row with the conditional row's ids, as the repetition
 * penalty does.  Per-step scores (gvc_gpt_generate_scores) carry them: they are processors; logits stay raw.
 * window > 0 also narrows the row's multiplicative repetition_penalty to the ids with c_i > 0 (the fake prompt ids are no longer
 * penalised): the windowed repetition penalty, usable alone (presence = frequency = 0).  With window == 0 the repetition penalty is
 * untouched: every id of input_ids, once.  The stop code is never in a row's history, so c_eos = 0.  A RAS redraw (gvc_logits_ras)
 * draws from the row that carries the penalties.  The counts are integers built with integer LDS atomics: the same bits on every
 * run, whatever the history length.
 * A null table, a -1 index or an entry with presence == frequency == 0 and window == 0 computes exactly what the call without it
 * computes, through the same barriers.
 * ------------------------------------------------------------------------------------------ */
#define GVC_PENALTY_MAX 2.0f            /* |presence|, |frequency| <= 2: the OpenAI range */
typedef struct gvc_logits_penalties {
    float presence;                     /* p in [-2, 2]; 0 off */
    float frequency;                    /* f in [-2, 2]; 0 off */
    int32_t window;                     /* 0: every generated id of the row; W > 0: the last W of them (and the repetition penalty too) */
    int32_t prompt_len;                 /* prompt length of the rows of this entry (fake ids included), as gvc_logits_ras' */
} gvc_logits_penalties;

/* gvc_sample_pen: gvc_sample_ras with a penalties table; gvc_gpt_generate_pen: gvc_gpt_generate_ras with one.  pen (HOST, nullable:
 * null is exactly the call without it): n_sets entries (1 <= n_sets <= B <= 64) indexed like warps / ras -- row b uses
 * pen[set_of_row[b]], none for -1, entry 0 for every row when set_of_row is null.  The table travels into the device-resident call
 * state in one staging launch of its own (1 KB of kernel argument) ahead of the call's first launch, so nothing is allocated or
 * synchronised per call.  The kernels and step graphs are those of the call without the table (the argmax kernel at top_k == 1
 * unless the call also has a RAS table), so gvc_gpt_warmup and its relatives prepare such calls as they stand.  GVC_ERR_ARG: a
 * non-finite presence / frequency or one outside [-2, 2], window < 0, prompt_len < 0, n_sets outside [1, B].  Not on the beam,
 * contrastive, assisted or lookup paths. */
int gvc_sample_pen(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                   const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                   const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias,
                   const gvc_logits_ras* ras, int32_t* ras_redraws, const gvc_logits_penalties* pen, int32_t step, int32_t* tok_out,
                   gvc_stream s);
int gvc_gpt_generate_pen(gvc_gpt* ctx, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                         int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                         const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                         int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, const gvc_logits_ras* ras,
                         int32_t* ras_redraws, const gvc_logits_penalties* pen, int32_t i0, int32_t n_steps, int32_t max_keys,
                         int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride, float* scores_out,
                         float* logits_out, int32_t out_stride, int32_t do_sample, gvc_stream s);
/* ------------------------------------------------------------------------------------------
 * Green-list watermark of the generated codes (Kirchenbauer et al.; transformers' WatermarkLogitsProcessor and WatermarkDetector with
 * context_width 1), on both sampler kernels, and its detector.
 * The table (DEVICE memory, uint32): `words` = ceil(vocab / 32) words per row; id i is green when bit (i & 31) of word (i >> 5) of
 * its row is set.  scheme 0 (lefthash): vocab rows, and the row of a step is that of prev = ids[len - 1], the last id of the row's
 * input_ids (the fake prompt's last id at the first step); a prev outside [0, vocab) leaves the step unmarked.  scheme 1 (selfhash):
 * one row, the ids that are green after themselves.  The caller builds the table (genvc_amd.engine.watermark_table: transformers'
 * recipe with a CPU generator) and keeps it alive and unchanged until every launch that reads it has finished.
 * Place in the chain: behind every processor and every warper, ahead of LogitNormalization (bias.renormalize), as transformers
 * appends it.  Sampling (top_k != 1): score_i = fl(score_i + bias) (one fp32 add) for every id i that survives the warpers and is
 * green; under selfhash only for those whose score is at least the 40th largest of the row ahead of truncation (transformers biases
 * the green ids among the 40 highest scores; ties at that boundary keep more than 40).  The draw takes its weights from the biased
 * survivors, relative to their maximum; per-step scores carry the bias, logits stay raw.  top_k == 1: the token is the argmax of
 * fl(fl(score_i / temperature) + bias * green_i) -- greedy search with the mark (pass temperature 1, as greedy search has none); the
 * stored scores of a greedy search are the biased row.  Scheme 1 at top_k == 1 computes the same without the 40-largest condition
 * and is not transformers' selfhash: the Python layer refuses it.  The speculative warp kernel never sees a table.
 * A null entries pointer, a -1 index or an entry with a null table computes exactly what the call without it computes, through the
 * same barriers.
 * What the C entries do NOT refuse (genvc_amd's Python layer does, by name): scheme 1 beside a typical_p warper -- typical decoding
 * can drop the highest scores, so the 40-highest threshold above is then not transformers' --, scheme 1 at top_k == 1, and a RAS
 * table beside a mark -- a redraw draws from the UNBIASED untruncated row relative to its unbiased maximum.
 * ------------------------------------------------------------------------------------------ */
#define GVC_WM_LEFTHASH 0
#define GVC_WM_SELFHASH 1
#define GVC_WM_SELFHASH_TOP 40          /* selfhash: only the green ids among this many highest scores are biased */
typedef struct gvc_logits_watermark {
    const uint32_t* table;              /* device: [vocab][words] (lefthash) or [words] (selfhash); null: off */
    float bias;                         /* finite; added to the green survivors */
    int32_t scheme;                     /* GVC_WM_LEFTHASH or GVC_WM_SELFHASH */
    int32_t words;                      /* ceil(vocab / 32) */
    int32_t reserved;                   /* 0 */
} gvc_logits_watermark;

/* gvc_sample_wm: gvc_sample_pen with a watermark table; gvc_gpt_generate_wm: gvc_gpt_generate_pen with one.  wm (HOST, nullable: null
 * is exactly the call without it): n_sets entries (1 <= n_sets <= B <= 64) indexed like warps / ras / pen -- row b uses
 * wm[set_of_row[b]], none for -1, entry 0 for every row when set_of_row is null.  The entries travel by value into the device-resident
 * call state in one staging launch ahead of the call's first launch; the kernels and step graphs are those of the call without them.
 * GVC_ERR_ARG (entries with a table): a non-finite bias, a scheme outside {0, 1}, words != ceil(vocab / 32), reserved != 0; n_sets
 * outside [1, B].  Not on
 * the beam, contrastive, assisted or lookup paths. */
int gvc_sample_wm(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                  const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                  const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias,
                  const gvc_logits_ras* ras, int32_t* ras_redraws, const gvc_logits_penalties* pen, const gvc_logits_watermark* wm,
                  int32_t step, int32_t* tok_out, gvc_stream s);
int gvc_gpt_generate_wm(gvc_gpt* ctx, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                        int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                        const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                        int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, const gvc_logits_ras* ras,
                        int32_t* ras_redraws, const gvc_logits_penalties* pen, const gvc_logits_watermark* wm, int32_t i0,
                        int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out,
                        int32_t lat_stride, float* scores_out, float* logits_out, int32_t out_stride, int32_t do_sample, gvc_stream s);
/* The detector's counts.  codes int32 [B][n] (row stride n), lens [B] (nullable: every row has n codes; else 0 <= lens[b] <= n), all
 * device memory; table / scheme / words as in gvc_logits_watermark, the table not null, vocab the table's.  One workgroup per row.
 * lefthash: position t in [1, len) is scored with the bit (codes[t-1], codes[t]); position 0 is unscored.  selfhash: position t in
 * [0, len) is scored with the self-green bit of codes[t].  A position whose id (or previous id, lefthash) lies outside [0, vocab) is
 * unscored.  ignore_repeated 1: an n-gram -- the pair (codes[t-1], codes[t]), or codes[t] alone under selfhash -- counts at its first
 * scored occurrence only; later ones are unscored.  counts int32 [B][2]: scored positions and green ones; flags uint8 [B][n]: 1 green,
 * 0 scored and not green, 2 unscored (every position at or past len included).  Integer arithmetic only: the same bits on every run.
 * GVC_ERR_ARG: a null pointer, B < 1, n < 1 or n > 8192 (the repeated-n-gram scan is quadratic in n), a scheme outside {0, 1}, words != ceil(vocab / 32), ignore_repeated not 0 / 1. */
int gvc_wm_score(const int32_t* codes, const int32_t* lens, int32_t B, int32_t n, const uint32_t* table, int32_t scheme, int32_t words,
                 int32_t vocab, int32_t ignore_repeated, int32_t* counts, uint8_t* flags, gvc_stream s);
/* gvc_gpt_warmup for gvc_gpt_generate_cfg over B items with this top_k: the guided step graphs of every context class up to max_keys
 * cached positions (and everything gvc_gpt_warmup(2B) prepares).  Afterwards such calls neither allocate nor synchronise */
int gvc_gpt_warmup_cfg(gvc_gpt* ctx, int32_t B, int32_t max_keys, int32_t top_k);

/* ------------------------------------------------------------------------------------------
 * Assisted (speculative) greedy decoding (HF generate(assistant_model=...), transformers generation/utils.py _assisted_decoding
 * with do_sample=False): a small draft context proposes k tokens per stream, the target scores [pending token, d_1..d_k] in ONE
 * multi-row pass, the longest prefix of drafts that equals the target's own greedy choices is accepted together with one target
 * token, and both KV caches roll back.  The emitted tokens are those of the plain greedy call.
 *
 * gvc_gpt_verify: appends T rows to each of the B slots (B * T <= 128, B * T <= max_rows): row t of stream b enters as
 * mel_embedding[toks[b][t]] + mel_pos[mel_pos(slot) + t] at cache position len(slot) + t, attends causally over [0, len + t], writes
 * its K/V, and its final_norm(ln_f(h)) / mel_head land in latent_out[b][t] / logits_out[b][t]; length and mel position advance by T.
 * d_model 1024 with B * T <= 16 runs the block stack in one launch (csrc/persist_rows.h), otherwise the skinny MFMA rows path.  More
 * than 128 rows is GVC_ERR_ARG.  A pending deferred token of a slot is decoded first.  A slot whose length + T would pass max_seq - 1
 * is computed at the last positions that fit and a mel position past the table reads its last row: nothing is indexed out of
 * bounds, the slot does not advance, its outputs are invalid and the next call reports GVC_ERR_STATE as after a full decode step.
 * gvc_gpt_truncate: length and mel position of slot b go down by drop[b] (DEVICE int32 [B], negative counts as 0), not below 0;
 * no synchronisation.  K/V behind the new length is overwritten by later rows.
 * ------------------------------------------------------------------------------------------ */
int gvc_gpt_verify(gvc_gpt* ctx, const int32_t* slots, int32_t B, const int32_t* toks, int32_t T, float* logits_out, float* latent_out,
                   gvc_stream s);
int gvc_gpt_truncate(gvc_gpt* ctx, const int32_t* slots, int32_t B, const int32_t* drop, gvc_stream s);

/* State of an assisted generation: DEVICE arrays owned by the caller.  ids / ids_len / finished as in gvc_sample; ids_stride must
 * hold prompt + max_new + 16 ids.  emitted[b]: tokens row b has emitted; toks / lats receive token j of row b at column j (the
 * caller fills toks with the stop token first).  pending[b]: the row's last emitted token, which is in neither KV cache yet and
 * opens the next round.  rounds / drafted / accepted (nullable): counters, bumped once per round and live row.
 * The rest is workspace of gvc_gpt_generate_assisted (unused by gvc_spec_accept): v_toks [B][16], v_logits [B][16][vocab],
 * v_latents [B][16][d], d_ids_len / d_finished [B]. */
typedef struct gvc_spec_state {
    int32_t B, ids_stride, max_new, tok_stride, lat_stride, d;
    int32_t* ids;
    int32_t* ids_len;
    int32_t* finished;
    int32_t* emitted;
    int32_t* pending;
    int32_t* toks;
    float* lats;                        /* nullable */
    int32_t* drop_target;               /* [B] rows the target / the assistant drop after this round */
    int32_t* drop_assistant;
    int32_t* rounds;
    int32_t* drafted;
    int32_t* accepted;
    int32_t* v_toks;
    float* v_logits;
    float* v_latents;
    int32_t* d_ids_len;
    int32_t* d_finished;
} gvc_spec_state;

/* The accept step, one workgroup per stream.  logits [B][k + 1][vocab] and latents [B][k + 1][d] are the target's rows for the inputs
 * [pending, d_1..d_k]; drafts [B][draft_stride] holds d_1..d_k (0 <= k <= 15; k = 0: the opening step of a generation, one row per
 * stream and no draft).  `appended`: rows both caches gained this round (k + 1; 0 for the opening step).  A live row with r =
 * max_new - emitted tokens to go compares k' = min(k, r - 1) drafts (HF clamps the draft length the same way): for i = 0..k' in
 * order, draft i - 1 goes into the ids row, the greedy chain of gvc_sample at top_k = 1 (repetition penalty, the processors `proc`
 * at length ids_len + i, temperature, argmax with the lower index winning a tie) runs on logits row i, the token is emitted with
 * latent row i, and the row goes on while i < k' and the token equals draft i and is not the stop token.  Then ids_len and emitted
 * grow by the m emitted tokens, pending is the last of them, finished is set at the stop token or when emitted reaches max_new,
 * both drops are appended - m (0 for the opening step), and rounds += 1, drafted += k', accepted += the agreeing drafts (not for
 * the opening step).  A finished row emits nothing and drops `appended`.  p: eos_token, vocab (<= 2048), repetition_penalty and
 * temperature are read.  proc: nullable HOST struct, free when the call returns. */
int gvc_spec_accept(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                    const int32_t* drafts, int32_t draft_stride, const gvc_sample_params* p, const gvc_logits_processors* proc,
                    gvc_stream s);

/* n_rounds rounds of assisted greedy decoding over st->B streams (B * (k + 1) <= 128, 1 <= k <= 15) with no host synchronisation
 * inside or between them.  target / assistant: two contexts with the same vocabulary whose slots[b] / assistant_slots[b] (device
 * arrays) hold the same stream, both prefilled.  first != 0 opens the generation: token 0 of every row is the target's greedy
 * choice from the logits its prefill parked (gvc_spec_accept with k = 0) and becomes the pending token.  One round:
 *   1. the assistant decodes the pending token, then k x [greedy sample -> decode step] with the call's settings on its own
 *      logits; the last of those decodes consumes d_k, so that a round in which every draft is accepted leaves the assistant
 *      complete (k + 1 decode steps per round; both caches then hold the same k + 1 new positions and roll back by the same count);
 *   2. gvc_gpt_verify of [pending, d_1..d_k] on the target: exactly one block-stack pass per round;
 *   3. gvc_spec_accept;  4. gvc_gpt_truncate on both contexts.
 * Rows accept different counts: all loop state is per row on the device.  The caller reads st->finished between calls.  max_keys /
 * assistant_max_keys: cached positions the longest stream can reach inside this call, rolled-back rows included (GVC_ERR_STATE
 * when that passes max_seq - 1: refused before anything runs).  The rounds are launched directly, not captured.  Pending deferred
 * tokens of the slots are decoded first; the slots end the call with nothing deferred and their parked logits stale. */
int gvc_gpt_generate_assisted(gvc_gpt* target, gvc_gpt* assistant, const int32_t* slots, const int32_t* assistant_slots,
                              const gvc_spec_state* st, const gvc_sample_params* p, const gvc_logits_processors* proc, int32_t first,
                              int32_t n_rounds, int32_t k, int32_t max_keys, int32_t assistant_max_keys, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Speculative SAMPLING for assisted decoding (Leviathan et al. 2023; transformers generation/utils.py _speculative_sampling).  The
 * draft draws d_{i+1} from q_i, its own warped row; the target's verification row i is warped into p_i -- "warped" is what gvc_sample
 * draws from: repetition penalty over the ids the row has at that position (accepted drafts included), the processors `proc` (min_p
 * included) at length ids_len + i, Temperature, TopK, TopP, MinP; kept entries weigh expf(s - max) in fp32, sums and CDFs are double
 * in vocabulary order, a probability is weight / total.  For one stream with e tokens emitted and k' = min(k, max_new - e - 1), for
 * i = 0, 1, ..: draft x = d_{i+1} is accepted iff (double)u_acc(e + i) * q_i(x) <= p_i(x) (no division: q_i(x) == 0 accepts) and is
 * emitted with latent row i; the stop token ends the row.  At the first rejection one token is drawn from max(p_i - q_i, 0) by the
 * sampler's inverse-CDF rule (first kept index whose running mass reaches u * total, else the last kept index) with u = u_res(e + i)
 * -- from p_i with the same u when the residual is empty (p_i == q_i); behind k' accepted drafts one token is drawn from p_k' with
 * u_res(e + k').  The opening step (k = 0) draws token 0 from p_0 with u_res(0).  Bookkeeping is gvc_spec_accept's, field for field.
 * RNG counters are keyed by position, so a result does not depend on how rounds are grouped into calls; row b deciding token t uses
 *     u_draft(t) = rng_uniform(seed, t, 3b)     u_acc(t) = rng_uniform(seed, t, 3b + 1)     u_res(t) = rng_uniform(seed, t, 3b + 2)
 * and a position drafted behind a rejection reuses its uniforms when it is drafted again (they were never looked at).
 * Each emitted token is distributed as a plain sampled token of the target under the same warpers; the tokens themselves are NOT those
 * of gvc_gpt_generate with the same seed.
 * ------------------------------------------------------------------------------------------ */
/* Device workspaces of a sampled assisted generation, owned by the caller: q_scores / p_scores fp32 [B][16][vocab] (used as
 * [B][k + 1][vocab]: row j of q is the warped row d_j was drawn from, row 0 unused; row i of p is p_i), rows [B] the draft sampler's
 * keyed rows (written at the start of every round: the call's settings, seed, rng_row = 3b, rng_step0 = emitted[b]). */
typedef struct gvc_spec_sampling {
    float* q_scores;
    float* p_scores;
    gvc_row_sampling* rows;
} gvc_spec_sampling;

/* The accept step of speculative sampling alone, warping included; needs no context.  Arguments as gvc_spec_accept, plus q_scores
 * [B][k + 1][vocab] (read; null allowed for k = 0) and p_scores [B][k + 1][vocab] (written: the warped target rows up to k').  d_1..d_k'
 * are written behind the live rows' ids first, then one workgroup per verification row warps it and one per stream applies the rule;
 * only the rows up to the first rejection are read.  p: every field is read (top_k == 1 is served too: one-hot rows).  A null
 * workspace, top_k > vocab or temperature <= 0 is GVC_ERR_ARG before anything is launched. */
int gvc_spec_accept_sample(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                           const int32_t* drafts, int32_t draft_stride, const float* q_scores, float* p_scores,
                           const gvc_sample_params* p, const gvc_logits_processors* proc, gvc_stream s);

/* gvc_gpt_generate_assisted with speculative sampling: the same contract (first, n_rounds, k, both max_keys, no host synchronisation
 * inside, rounds launched directly), the sampling settings taken from p (top_k != 1; top_k == 1 is gvc_gpt_generate_assisted).  The
 * draft's steps run gvc_sample's full kernel on the keyed rows `ss->rows` and store their warped rows in ss->q_scores; step 3 of a
 * round is gvc_spec_accept_sample.  ss: HOST struct of device pointers, free when the call returns. */
int gvc_gpt_generate_assisted_sample(gvc_gpt* target, gvc_gpt* assistant, const int32_t* slots, const int32_t* assistant_slots,
                                     const gvc_spec_state* st, const gvc_spec_sampling* ss, const gvc_sample_params* p,
                                     const gvc_logits_processors* proc, int32_t first, int32_t n_rounds, int32_t k, int32_t max_keys,
                                     int32_t assistant_max_keys, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Prompt-lookup assisted decoding (HF generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=N), transformers
 * generation/candidate_generator.py PromptLookupCandidateGenerator): the drafts of a round come from the row's own history instead of
 * a draft model.  For a live row with history h = ids[from .. ids_len) (the generated codes; the last entry is the pending token), for
 * n = min(N, len(h) - 1) down to 1: the lowest index i with h[i .. i + n) == h[len - n ..) and i + n < len (the suffix's own position
 * never counts, so the continuation is not empty); the first n with a hit wins, and the drafts are h[i + n .. min(i + n + k, len)) -- they
 * may overlap the suffix.  `from` is the prompt length: the placeholder ids of the prefix and the start token are no codes and are never
 * searched (HF would match inside them).
 *
 * gvc_spec_lookup: the kernel alone, one workgroup per stream, no context needed.  Reads st->ids / ids_stride / ids_len / finished /
 * pending; writes st->v_toks as [B][k + 1]: column 0 the pending token (the call is the round's begin), columns 1..draft_len[b] the
 * drafts, the remaining columns the pending token again (a valid id that is never compared); draft_len DEVICE int32 [B] gets the
 * count, 0..k, and 0 for a finished row.  q_scores (nullable) fp32 [B][k + 1][vocab]: row j = 1..k of a live stream becomes the
 * one-hot row of v_toks[b][j] in the form gvc_spec_accept_sample reads, a warped scores row -- 0 at the token and -inf at every other
 * id, i.e. probability exactly 1 at the token and 0 elsewhere.  GVC_ERR_ARG for k outside [1, 15], max_ngram outside [1, 8], negative
 * `from`, a null array, or ids_stride - from above 2048 (the history is staged in LDS); nothing is launched then.
 *
 * gvc_spec_accept_len / gvc_spec_accept_sample_len: gvc_spec_accept / gvc_spec_accept_sample with a draft count per row, draft_len
 * DEVICE int32 [B] (nullable): k' = min(k, max_new - emitted - 1, draft_len[b]), and drafted += k'.  Null is the entry without it,
 * bit for bit.
 *
 * gvc_gpt_generate_lookup: gvc_gpt_generate_assisted without an assistant; the same contract for `first`, no host synchronisation
 * inside or between rounds, the checks of gvc_gpt_verify, GVC_ERR_STATE before anything runs when max_keys would pass max_seq - 1, and
 * pending deferred tokens decoded first.  One round: gvc_spec_lookup -> gvc_gpt_verify of [pending, d_1..d_k] -> gvc_spec_accept_len
 * (ss null) or gvc_spec_accept_sample_len (ss given; p->top_k != 1) -> gvc_gpt_truncate of the target by drop_target.  Every stream
 * pays the full (k + 1)-row pass, whatever its draft_len.  Sampled, this is speculative sampling with q = one-hot: draft x at position
 * e + i is accepted iff u_acc(e + i) <= p_i(x), the residual is p_i with x removed, u_draft is not consumed, and u_acc / u_res stay
 * keyed by position as above.  ss->rows is not used and may be null.  draft_len: DEVICE int32 [B] workspace owned by the caller.
 * ------------------------------------------------------------------------------------------ */
int gvc_spec_lookup(const gvc_spec_state* st, int32_t k, int32_t max_ngram, int32_t from, int32_t* draft_len, float* q_scores,
                    int32_t vocab, gvc_stream s);
int gvc_spec_accept_len(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                        const int32_t* drafts, int32_t draft_stride, const int32_t* draft_len, const gvc_sample_params* p,
                        const gvc_logits_processors* proc, gvc_stream s);
int gvc_spec_accept_sample_len(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                               const int32_t* drafts, int32_t draft_stride, const int32_t* draft_len, const float* q_scores,
                               float* p_scores, const gvc_sample_params* p, const gvc_logits_processors* proc, gvc_stream s);
int gvc_gpt_generate_lookup(gvc_gpt* target, const int32_t* slots, const gvc_spec_state* st, const gvc_spec_sampling* ss,
                            const gvc_sample_params* p, const gvc_logits_processors* proc, int32_t first, int32_t n_rounds, int32_t k,
                            int32_t max_ngram, int32_t from, int32_t* draft_len, int32_t max_keys, gvc_stream s);

/* Which decode step the last gvc_gpt_generate call replayed (diagnostic): 0 none yet, 1 launch-per-phase with split-key attention,
 * 2 launch-per-phase with the fused short-context attention launch, 3 the one-launch step (one stream), 4 the MFMA rows path
 * (launch per phase: 17+ streams, or shapes the one-launch rows step does not serve), 5 the one-launch rows step (2..16 streams,
 * csrc/persist_rows.h).  gvc_gpt_verify and the rounds of gvc_gpt_generate_assisted report 5 or 4 for their verification pass (on the
 * assistant: the variant of its draft steps). */
int gvc_gpt_decode_variant(gvc_gpt* ctx);
/* Diagnostic: how many one-launch rows steps (csrc/persist_rows.h: 2..16 rows that continue cached sequences -- batched decode
 * steps, the uncached rows of a streaming chunk's prefill) this context has issued; a step captured into the generation loop's
 * graph counts once.  Tests use it to prove which path served a call. */
long long gvc_gpt_rows_step_launches(gvc_gpt* ctx);
/* bf16 matrix-core strip GEMMs issued so far by the multi-row passes of a weight_dtype-4 context (four per layer and pass; a captured
 * graph counts once per capture); 0 in every other mode. */
long long gvc_gpt_bf16_gemm_launches(gvc_gpt* ctx);
/* Diagnostic: how many one-stream one-launch decode steps (csrc/persist_kernel.h) have RUN in this context -- generation loops,
 * gvc_gpt_decode_step, flushes of deferred decodes.  A launch that left at its run flag (the first step of a deferring call with
 * nothing pending, a flush row with nothing pending) is not counted: a prefill followed by 24 generated tokens counts 23, and 24
 * under GVC_DEFER_DECODE=0.  Synchronises the device; -1 on an error. */
long long gvc_gpt_one_stream_steps(gvc_gpt* ctx);
/* Health of the work a caller has just synchronised (no reference counterpart: the reference has no in-kernel hand-offs).  The
 * one-launch steps need all 256 workgroups co-resident; when another process or stream holds CUs a hand-off times out (~0.2 s,
 * bounded spins), the step's outputs are garbage and a device-visible word records it.  This call -- and, failing that, the next
 * library call -- then returns GVC_ERR_TIMEOUT ONCE, having switched the context to the launch-per-phase paths (captured graphs
 * dropped, hand-off buffers re-initialised): the context stays usable, the caller resets the affected slots and repeats the work.
 * Also reports a full KV cache / mel position table (see gvc_gpt_reset_slots).  GVC_OK otherwise. */
int gvc_gpt_health(gvc_gpt* ctx);
/* Warm-up (reference: the user's own warm-up conversions, /root/reference/infer.py:27-30; SURVEY.md 8(b)(iii): no hidden
 * synchronisation or allocation after create).  Does, for a generation over B streams that reaches max_keys cached positions
 * (0: up to max_seq) with this top_k, everything the first data-path call of that shape would otherwise do itself: the one-launch
 * steps' hand-off buffers, packed weight copy, XCD-topology probe and LDS opt-in, and the capture of the step graphs (eight steps /
 * one step).  Synchronous; call it after the weights are bound, once per (B, context class, greedy or sampled) a deployment uses.
 * Afterwards gvc_gpt_generate / gvc_gpt_decode_step / gvc_gpt_prefill_cached calls of that shape do no hipMalloc, no
 * hipDeviceSynchronize and no graph capture. */
int gvc_gpt_warmup(gvc_gpt* ctx, int32_t B, int32_t max_keys, int32_t top_k);
/* The same for EVERY context class a generation over B streams passes through while its longest stream grows from min_keys to max_keys
 * cached positions (the library keys its step graphs by classes of the context length -- fused / split-key attention, 1 / 2 / 4 key chunks
 * of the rows steps -- whose thresholds are its own business: callers name the range, not the classes). */
int gvc_gpt_warmup_range(gvc_gpt* ctx, int32_t B, int32_t min_keys, int32_t max_keys, int32_t top_k);
/* gvc_gpt_warmup for gvc_gpt_beam_generate over B items of K beams: the beam step graphs of every context class up to max_keys cached
 * positions (and everything gvc_gpt_warmup(B*K) prepares).  Afterwards such calls neither allocate nor synchronise */
int gvc_gpt_warmup_beam(gvc_gpt* ctx, int32_t B, int32_t K, int32_t max_keys);
/* ... for gvc_gpt_group_beam_generate over B items of K beams in G groups (the group step graphs do not depend on G beyond its checks) */
int gvc_gpt_warmup_group_beam(gvc_gpt* ctx, int32_t B, int32_t K, int32_t G, int32_t max_keys);
/* Diagnostic: allocations / device-wide synchronisations / graph captures this context has done INSIDE data-path calls (first use
 * of a path that gvc_gpt_warmup had not prepared; a rebind after the weight pack was built; the fallback after a hand-off
 * time-out).  gvc_gpt_warmup's own work does not count.  Tests assert it stays put across warmed-up calls. */
long long gvc_gpt_lazy_inits(gvc_gpt* ctx);
/* Re-arm the one-launch steps after a hand-off time-out has switched the context to the launch-per-phase paths (gvc_gpt_health): to be called
 * when the caller knows the GPU is its own again (no reference counterpart).  Reports pending errors like gvc_gpt_health; synchronises the
 * device, drops the captured step graphs and resets the hand-off state.  A later time-out falls back again. */
int gvc_gpt_rearm(gvc_gpt* ctx);

/* Measurement hook used by bench.py (not a reference interface): launches ONLY one kernel class of the
 * decode step (0 c_attn GEMV, 1 attention, 2 attn c_proj GEMV, 3 mlp c_fc GEMV, 4 mlp c_proj GEMV, 5 head
 * GEMV) for every layer, n_steps times back to back on the stream between two hipEvents, and returns the
 * mean microseconds per launch (same-stream launch boundary included) and the number of launches.
 * which = 6: the whole decode step (sampler excluded); which = 16 + X: the whole step WITHOUT class X, so that
 * (whole - without) / launches_per_step is the IN-SITU cost of class X (behind its real predecessor, as rocprofv3
 * sees it); both return microseconds per step.  which = 7: the one-launch decode step (csrc/persist_kernel.h), microseconds per
 * launch.  0..6 and 16+ always time the launch-per-phase step (the fallback of bf16 / multi-stream / partial-GPU contexts).
 * Synchronises the stream; leaves the slots' caches in an undefined state (reset or prefill afterwards). */
int gvc_gpt_time_kernel(gvc_gpt* ctx, int32_t which, const int32_t* slots, int32_t B, const int32_t* tok_in,
                        int32_t n_steps, float* avg_us, int32_t* n_launches, gvc_stream s);

/* Measurement / test hook for the fp32 MFMA GEMMs under the prefill (not a reference interface): C[M][N] = A[M][K] W[N][K]^T
 * (+ bias[N], nullable), all row-major device buffers, through one kernel: variant 0 the 64x64x32 tiled kernel, 1 the strip
 * kernel (operands converted to the fragment-major layout first; K split up to sk_max), 2 the skinny kernel (M <= 128), 3 the bf16
 * matrix-core strip kernel (csrc/gemm_b16.hip: both operands rounded to bf16, nearest even, by the probe; K split up to sk_max; needs
 * K % 32 == 0 and N % 64 == 0).  With
 * iters > 0 the GEMM is then launched iters more times between two hipEvents and *avg_us is the mean microseconds per GEMM
 * (split-K epilogue included).  Synchronises the stream. */
int gvc_gemm_probe(int32_t variant, const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                   int32_t sk_max, int32_t iters, float* avg_us, gvc_stream s);

/* Test hook for every operand mode and epilogue of the fp32 GEMM kernels (csrc/gemm.h; not a reference interface): one launch of one
 * kernel class on CALLER-OWNED device buffers, described by the fields a product caller sets in GemmArgs / GemmEpi / LnFuse, so that a
 * test can surround every buffer with guard regions.  No conversion, no allocation, no timing; synchronises the stream.
 * kind: GVC_GEMM_TILED      launch_gemm_cap(batch, work_cap): row-major operands, implicit conv, batches, split-K chosen by the shape;
 *       GVC_GEMM_SKINNY     launch_gemm_skinny(sk): FM16 operands (A padded to 16 rows), M <= 128; sk > 1 leaves raw planes in work;
 *       GVC_GEMM_SKINNY_LN  launch_gemm_skinny_ln: A = LayerNorm(x_in + pbias + sum part) built in the prologue (the ln_* fields);
 *       GVC_GEMM_STRIP      launch_gemm_strip(sk = sk_max, raw_partials); the chosen split comes back in sk_used;
 *       GVC_GEMM_STRIP_GEOM the strip kernel with mtw M tiles per workgroup and K split sk (refused when the pair cannot run);
 *       GVC_GEMM_LN_ROWS / _LN_ROWS_B16  launch_ln_sum_rows(_b16): rows = M, d = K, x_in / x_out / part / ln_sk / pbias / ln_w / ln_b,
 *                           output a = C (a_fm16 = c_fm16; b16: C holds bf16 in the FB16 layout and stats gets (mean, rstd) per row);
 *       GVC_GEMM_TO_FM16 / _TO_FM16_BF16  C = the FM16 copy of the row-major [N][K] matrix A (bf16: of its upper 16 bits). */
enum { GVC_GEMM_TILED = 0, GVC_GEMM_SKINNY = 1, GVC_GEMM_SKINNY_LN = 2, GVC_GEMM_STRIP = 3, GVC_GEMM_STRIP_GEOM = 4, GVC_GEMM_LN_ROWS = 5,
       GVC_GEMM_LN_ROWS_B16 = 6, GVC_GEMM_TO_FM16 = 7, GVC_GEMM_TO_FM16_BF16 = 8 };
typedef struct gvc_gemm_case {
    int32_t kind, M, N, K;
    const void* A; const void* W; float* C; float* work;
    int64_t a_batch_stride, a_batch_stride2, w_batch_stride, c_batch_stride, c_batch_stride2, work_cap;
    int32_t lda, ldw, ldc, w_bf16, batch, batch_inner, conv_cin, conv_tap_stride, a_act;
    float a_slope;
    const float* att_part;
    int32_t att_nc, att_heads, att_hd;
    int32_t sk, raw_partials, mtw, sk_used;        /* sk_used: written by the call */
    /* GemmEpi */
    const float* bias; const float* resid; const float* resid2;
    int64_t bias_batch_stride, resid_batch_stride, resid_batch_stride2;
    int32_t act, ldr, resid_fm16, geglu, c_fm16, qkv, d, n_head, head_dim, max_seq, T, kv_bf16;
    float out_scale; int32_t reserved;
    void* kcache; void* vcache; const int32_t* slots; const int32_t* base_len;
    /* LnFuse / the row kernels */
    const float* x_in; float* x_out; const float* part; const float* pbias; const float* ln_w; const float* ln_b; float* stats;
    int32_t ln_sk, ln_rows;
} gvc_gemm_case;
int gvc_gemm_probe_ex(gvc_gemm_case* c, gvc_stream s);

/* Test hook for every attention kernel (csrc/gpt_kernels.h, csrc/attn64.h; not a reference interface), after the pattern of
 * gvc_gemm_probe_ex: one launch of one kernel class on CALLER-OWNED device buffers, described by the fields a product caller sets (AttnArgs,
 * AttnProjArgs, the arguments of k_attn64_mfma), so that a test can surround every buffer with guard regions and poison what the call must
 * not read.  No allocation, no conversion, no timing; synchronises the stream.  The kernels trust their arguments as they trust the
 * product's: the caller owns every bound (strides, slot numbers, key counts against the cache it passes).
 * kind: GVC_ATTN_ROWS         launch_attention_hd(head_dim, n_head, args, chunks, rows, direct, wide, kv_bf16): k_attention, one workgroup per
 *                             (chunk, head, row).  direct: chunks = 1, out [rows][out_stride] row-major or FM16; otherwise out holds the chunk
 *                             partials [rows][n_head][chunks][head_dim + 4] = (o unnormalised, m, l, two floats nobody writes);
 *       GVC_ATTN_TILE         launch_attention_tile(head_dim, n_head, args, batch, max_keys, kv_bf16): `taken` comes back 1 when the chooser took
 *                             the call (0: it left it to k_attention and nothing was launched) and `ran` names the kernel its rule selects
 *                             (GVC_ATTN_RAN_SHORT: k_attention_tile_short, max_keys <= 128; GVC_ATTN_RAN_TILED: k_attention_tile).  `ran` is
 *                             DERIVED, not observed: the probe restates the launchers' threshold (gpt_kernels.h launch_attention_tile,
 *                             forward_eval.hip launch_attention_tile_masked) and must be kept equal to it when that rule changes;
 *       GVC_ATTN_TILE_MASKED  launch_attention_tile_masked(head_dim, n_head, args, batch, max_keys): key_mask [batch][mask_stride], fp32 cache,
 *                             no base_len; `taken` and `ran` as above (every shape is taken);
 *       GVC_ATTN_FUSED_PROJ   k_attn_proj<256, kv_bf16> on grid (d / 16, n_head): q [d], kbase / vbase [slot][n_head][max_seq][256], slots[0],
 *                             seq_len[slot] + 1 keys, Wp [d][d], out = part2 [n_head][d].  Refused (GVC_ERR_ARG) unless head_dim == 256,
 *                             d == n_head * 256, d a multiple of 16, d <= 1024 and seq_len[slots[0]] + 1 <= 128 (the kernel has no place for more
 *                             keys and would ignore them silently; the probe reads the two integers back to check);
 *       GVC_ATTN_64           k_attn64_mfma<mask, nw> (nw 4 or 16) on grid (ceil(Tq / 16), n_head, batch): q / kbase / vbase fp32 matrices with
 *                             row stride ld and batch stride bs, out [batch * out_rows][E] row-major or FM16, fmask int32 [batch][Tk]
 *                             (nonzero = excluded; read only with mask != 0). */
enum { GVC_ATTN_ROWS = 0, GVC_ATTN_TILE = 1, GVC_ATTN_TILE_MASKED = 2, GVC_ATTN_FUSED_PROJ = 3, GVC_ATTN_64 = 4 };
enum { GVC_ATTN_RAN_NONE = 0, GVC_ATTN_RAN_SHORT = 1, GVC_ATTN_RAN_TILED = 2 };
typedef struct gvc_attn_case {
    int32_t kind, head_dim, n_head, kv_bf16;
    /* AttnArgs */
    const float* q; const void* kbase; const void* vbase;
    int64_t k_batch_stride, k_head_stride;
    int32_t q_stride, k_row_stride, T, causal, n_keys, out_stride, out_fm16, mask_stride;
    float scale; int32_t reserved;
    const int32_t* slots; const int32_t* base_len; float* out; const uint8_t* key_mask;
    /* the launchers' own arguments; taken / ran: written by the call */
    int32_t chunks, rows, direct, wide, batch, max_keys, taken, ran;
    /* AttnProjArgs (with q, kbase, vbase, slots, n_head, scale, out) */
    const int32_t* seq_len; const float* Wp;
    int32_t max_seq, d;
    /* k_attn64_mfma (with q, kbase, vbase, out, n_head, batch, scale, out_fm16) */
    int32_t nw, mask;
    const int32_t* fmask;
    int64_t ld, bs;
    int32_t Tq, Tk, out_rows, E;
} gvc_attn_case;
int gvc_attn_probe(gvc_attn_case* c, gvc_stream s);

/* Element index of (row m, column k) of an [M][K] bf16 matrix in the fragment-major layout of the bf16 matrix-core GEMMs
 * (csrc/gemm_b16.h: fb16_index; M % 16 == 0, K % 32 == 0): each (16 rows x 32 k) block is 64 fragments of 8 consecutive k, fragment
 * (m % 16) + 16 * ((k % 32) / 8) -- the lane of v_mfma_f32_16x16x32_bf16 that holds them.  Host arithmetic only. */
int64_t gvc_fb16_index(int32_t m, int32_t k, int32_t K);

/* ------------------------------------------------------------------------------------------
 * Perceiver resampler.  Replaces layers/perceiver_encoder.py:PerceiverResampler.forward (:265-276)
 * as called by GPT.get_style_emb (gpt.py:351-373) with mask=None.
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_perceiver gvc_perceiver;
typedef struct gvc_perceiver_dims {
    int32_t dim, depth, dim_context, num_latents, dim_head, heads, ff_mult;
    int32_t max_batch, max_frames;
} gvc_perceiver_dims;

int gvc_perceiver_create(const gvc_perceiver_dims* dims, gvc_perceiver** out);
int gvc_perceiver_destroy(gvc_perceiver* ctx);
/* names relative to the module: "latents", "proj_context.weight", "layers.0.0.to_q.weight",
 * "layers.0.1.0.weight", "norm.gamma", ... */
int gvc_perceiver_bind_weight(gvc_perceiver* ctx, const char* name, const float* src, int64_t numel,
                              gvc_stream s);
int gvc_perceiver_missing_weights(gvc_perceiver* ctx);
/* x: [B,F,dim_context] -> out [B,num_latents,dim] */
int gvc_perceiver_forward(gvc_perceiver* ctx, const float* x, int32_t B, int32_t F, float* out,
                          gvc_stream s);

/* PerceiverResampler.forward(x, mask=) (perceiver_encoder.py:265-273, Attention.forward :305-316, 130-134): key_mask uint8
 * [B][num_latents + F] (device, nonzero = attend) over the keys [latents | frames] of every layer's cross-attention; a masked key has
 * weight exactly 0.  The mask GPT.get_style_emb(seq_lens=) builds (gpt.py:362-367) is the caller's.  Runs uncaptured. */
int gvc_perceiver_forward_masked(gvc_perceiver* ctx, const float* x, int32_t B, int32_t F, const uint8_t* key_mask, float* out,
                                 gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Log-mel front end.  Replaces utils.py:TorchMelSpectrogram.forward (:150-162) as instantiated at
 * trainers/hifigan_trainer.py:105-115 (n_fft 2048, hop 256, win 1024, 24 kHz, 0-8 kHz, 80 mels,
 * slaney norm, htk scale, centre + reflect pad).
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_mel gvc_mel;
int gvc_mel_create(int32_t n_fft, int32_t hop, int32_t win, int32_t sample_rate, float f_min,
                   float f_max, int32_t n_mels, const float* mel_norms_host, gvc_mel** out);
int gvc_mel_destroy(gvc_mel* ctx);
/* wav [B,T] -> out [B,n_mels,1+T/hop] (reference layout); if out_frames_major != NULL it also
 * receives [B,1+T/hop,n_mels] (the layout the Perceiver consumes). */
int gvc_mel_forward(gvc_mel* ctx, const float* wav, int32_t B, int32_t T, float* out,
                    float* out_frames_major, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Content tokenizer.  Replaces layers/dvae.py:DiscreteVAE.get_codebook_indices (:324-331) with
 * the 1-D encoder of :252-291 and Quantize.forward (:87-93).
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_dvae gvc_dvae;
typedef struct gvc_dvae_dims {
    int32_t channels, hidden_dim, num_layers, num_resnet_blocks, kernel_size, codebook_dim,
        num_tokens;
    int32_t max_batch, max_frames;
} gvc_dvae_dims;
int gvc_dvae_create(const gvc_dvae_dims* dims, gvc_dvae** out);
int gvc_dvae_destroy(gvc_dvae* ctx);
/* names relative to the module: "encoder.0.0.weight", "encoder.2.net.0.bias", "codebook.embed" */
int gvc_dvae_bind_weight(gvc_dvae* ctx, const char* name, const float* src, int64_t numel, gvc_stream s);
int gvc_dvae_missing_weights(gvc_dvae* ctx);
/* feat [B,channels,T] (reference layout) -> codes int32 [B,Tc], Tc = T halved num_layers times
 * (ceil); enc_out (optional, may be NULL) receives the encoder output [B,Tc,codebook_dim]. */
int gvc_dvae_encode(gvc_dvae* ctx, const float* feat, int32_t B, int32_t T, int32_t* codes_out,
                    float* enc_out, gvc_stream s);
/* same, from frame-major features [B,T,channels] -- the layout ContentVec emits, i.e. the harness's
 * `get_codebook_indices(content_feat.transpose(1, 2))` (inference/inference_utils.py:53,167) without the transpose */
int gvc_dvae_encode_frames(gvc_dvae* ctx, const float* feat, int32_t B, int32_t T, int32_t* codes_out,
                           float* enc_out, gvc_stream s);
/* The whole DiscreteVAE: a context created with GVC_DVAE_DECODER also binds the reference's `decoder.*` tensors
 * ("decoder.0.weight", "decoder.1.net.0.weight", "decoder.4.0.conv.weight", "decoder.6.bias", ...: layers/dvae.py:252-292 with
 * use_transposed_convs=False) and counts them in gvc_dvae_missing_weights; flags = 0 is gvc_dvae_create.  Each nearest-x2
 * upsampling + Conv1d stage is folded at bind time into two polyphase weight sets applied at the input rate. */
#define GVC_DVAE_DECODER 1
int gvc_dvae_create_ex(const gvc_dvae_dims* dims, int32_t flags, gvc_dvae** out);
/* DiscreteVAE.decode (:333-352): codes int32 [B,n] -> out [B,channels,n*2^num_layers]; pre_out (may be NULL) receives the last
 * layer's input [B,hidden_dim,n*2^num_layers].  Asynchronous, no allocation.  A code outside [0, num_tokens) is replaced by code 0
 * and remembered: the next gvc_dvae_code_error reports it. */
int gvc_dvae_decode(gvc_dvae* ctx, const int32_t* codes, int32_t B, int32_t n, float* out, float* pre_out, gvc_stream s);
/* synchronises the stream; GVC_ERR_ARG (and the mark is cleared) when a decode since the last call met a code out of range */
int gvc_dvae_code_error(gvc_dvae* ctx, gvc_stream s);
/* DiscreteVAE.forward in eval mode (:363-381): feat [B,channels,T], T a multiple of 2^num_layers -> out [B,channels,T],
 * codes_out (may be NULL) int32 [B,T/2^num_layers], losses (device) float[2] = mse(feat, out), mean((embed_code(codes) -
 * encoder(feat))^2).  Both sums are reduced in a fixed order (per-workgroup partials, then one workgroup in double): the same
 * bits every call. */
int gvc_dvae_reconstruct(gvc_dvae* ctx, const float* feat, int32_t B, int32_t T, float* out, int32_t* codes_out,
                         float* losses, gvc_stream s);
/* standalone VQ: x [N,dim], embed [dim,n_embed] (reference layout) -> idx int32 [N] */
int gvc_vq_argmin(const float* x, const float* embed, int32_t N, int32_t dim, int32_t n_embed,
                  int32_t* idx, float* work /* N*n_embed floats */, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * HiFi-GAN generator.  Replaces layers/hifigan.py:HiFiGAN.forward (:218-233, ResBlock2
 * :119-157, or ResBlock1 :28-117 through gvc_hifigan_create_ex) and, for the latent entry point, the x4 linear interpolation in front of it
 * (inference/inference_utils.py:81-85, 196-202).
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_hifigan gvc_hifigan;
typedef struct gvc_hifigan_dims {
    int32_t in_dim;               /* vocoder_config.input_feat_dim (1024) */
    int32_t up_init_ch;           /* upsample_initial_channel (256) */
    int32_t n_ups;                /* len(upsample_rates) <= 4 */
    int32_t up_rates[4];          /* 8, 8, 4 */
    int32_t up_kernels[4];        /* 16, 16, 8 */
    int32_t n_kernels;            /* len(resblock_kernel_sizes) <= 4 */
    int32_t res_kernels[4];       /* 3, 5, 7 */
    int32_t res_dilations[4][2];  /* ResBlock2: [[1,2],[2,6],[3,12]] */
    int32_t max_batch, max_frames; /* capacity: input frames AFTER the interpolation */
} gvc_hifigan_dims;
int gvc_hifigan_create(const gvc_hifigan_dims* dims, gvc_hifigan** out);
/* The generator with either residual block of the reference (layers/hifigan.py:181): resblock_type 1 = ResBlock1 (:28-117, per
 * dilation d a conv of dilation d and one of dilation 1: the HiFi-GAN V1 generator has kernels 3 / 7 / 11 and dilations 1 / 3 / 5),
 * 2 = ResBlock2 (only the first two entries of a res_dilations row are read).  gvc_hifigan_create is this call with resblock_type 2.
 * ResBlock1 stages of 32 / 64 / 128 channels with three kernels of <= 11 taps run as six one-round-trip launches (csrc/conv_lds.h),
 * every other shape as one tiled-GEMM launch per conv. */
typedef struct gvc_hifigan_dims_ex {
    int32_t in_dim, up_init_ch;
    int32_t n_ups;                /* <= 4 */
    int32_t up_rates[4], up_kernels[4];
    int32_t n_kernels;            /* <= 4 */
    int32_t res_kernels[4];
    int32_t resblock_type;        /* 1 or 2 */
    int32_t res_dilations[4][3];  /* ResBlock1: [[1,3,5]] * 3; ResBlock2: [[1,2,-],[2,6,-],[3,12,-]] */
    int32_t max_batch, max_frames;
} gvc_hifigan_dims_ex;
int gvc_hifigan_create_ex(const gvc_hifigan_dims_ex* dims, gvc_hifigan** out);
int gvc_hifigan_destroy(gvc_hifigan* ctx);
/* names of the reference state dict with weight-norm folded (w = g * v / |v|, as remove_weight_norm leaves
 * them): "conv_pre.weight", "ups.1.bias", "resblocks.4.convs.0.weight", "conv_post.weight", ...; a ResBlock1 context takes
 * "resblocks.4.convs1.2.weight", "resblocks.4.convs2.2.bias", ... (12 tensors per block) */
int gvc_hifigan_bind_weight(gvc_hifigan* ctx, const char* name, const float* src, int64_t numel, gvc_stream s);
int gvc_hifigan_missing_weights(gvc_hifigan* ctx);
/* how many upsampling stages run their ResBlocks on the one-round-trip kernel (the others: one launch per conv), and the node count
 * of the most recently captured whole-call graph (0 before the first call) */
int gvc_hifigan_lds_stages(gvc_hifigan* ctx);
int gvc_hifigan_graph_nodes(gvc_hifigan* ctx);
/* x [B,in_dim,T] (reference layout) -> wav [B, T * prod(up_rates)] */
int gvc_hifigan_forward(gvc_hifigan* ctx, const float* x, int32_t B, int32_t T, float* wav, gvc_stream s);
/* latents [B,n,in_dim] (as yielded by the generation loop) -> F.interpolate(scale, linear) -> wav
 * [B, n * scale * prod(up_rates)] */
int gvc_hifigan_forward_latents(gvc_hifigan* ctx, const float* latents, int32_t B, int32_t n, int32_t scale,
                                float* wav, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Resampler.  Replaces torchaudio.functional.resample(audio, lsr, sampling_rate) as called by
 * utils.load_audio (utils.py:58-62): sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99.
 * ------------------------------------------------------------------------------------------ */
int gvc_resample_length(int32_t T, int32_t orig_sr, int32_t new_sr);
/* x [B,T] -> out [B, gvc_resample_length(T, orig_sr, new_sr)]; synchronises the stream (file-loading path) */
int gvc_resample(const float* x, int32_t B, int32_t T, int32_t orig_sr, int32_t new_sr, float* out, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * ContentVec / HuBERT-base feature extractor.  Replaces
 * ContentVecExtractor.extract_content_features (layers/content_processor.py:17-31):
 *   fairseq HubertModel.extract_features(source=wav, output_layer=n_layers)[0] -> final_proj
 * i.e. 7-layer conv extractor (GroupNorm + GELU on layer 0) -> LayerNorm -> post_extract_proj -> x + GELU(grouped
 * positional conv) -> LayerNorm -> n_layers post-LN transformer layers -> final_proj.  The reference's
 * `padding_mask = (wav == 0)` (content_processor.py:24) is derived from `wav` by the library itself, with fairseq's
 * reduction to frames (trailing samples % frames dropped, a frame is padding when every sample of its chunk is exactly
 * zero): padding frames are zeroed ahead of the positional conv and their keys are excluded from every attention.
 * Weight names are fairseq's (the keys under `content_extractor.model.` in a GenVC checkpoint), except the
 * weight-normed positional conv, bound folded as "encoder.pos_conv.0.weight" [E, E/groups, k] (g * v / |v|, dim=2).
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_hubert gvc_hubert;
typedef struct {
    int32_t n_conv;                 /* <= 8 */
    int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
    int32_t embed_dim, n_layers, n_heads, ffn_dim, pos_conv_kernel, pos_conv_groups, final_dim;
    int32_t max_batch, max_samples;
} gvc_hubert_dims;
int gvc_hubert_create(const gvc_hubert_dims* dims, gvc_hubert** out);
int gvc_hubert_destroy(gvc_hubert* ctx);
int gvc_hubert_bind_weight(gvc_hubert* ctx, const char* name, const float* src, int64_t numel, gvc_stream s);
int gvc_hubert_missing_weights(gvc_hubert* ctx);
/* frames the conv stack yields for n_samples input samples (<= 0: too short) */
int gvc_hubert_frames(gvc_hubert* ctx, int32_t n_samples);
/* wav [B,T] (16 kHz) -> out [B, gvc_hubert_frames(T), final_dim] */
int gvc_hubert_forward(gvc_hubert* ctx, const float* wav, int32_t B, int32_t T, float* out, gvc_stream s);

/* ------------------------------------------------------------------------------------------
 * Vocoder evaluation (trainers/hifigan_trainer.py:346-385): the waveform-domain discriminators of layers/hifigan.py
 * (MultiScaleDiscriminator :247-314, MultiPeriodDiscriminator :316-426) in eval mode, the reductions behind the criteria of
 * layers/hifigan_loss.py, and that file's mel extractor through gvc_mel_create_ex.  fp32 only, no gradients.
 *
 * One context is one of the two discriminators.  Weights are bound under the reference's state-dict names
 * (discriminators.{i}.convs.{j}.weight_g / weight_v / bias, discriminators.{i}.conv_post.*; a spectral-normed conv:
 * weight_orig, weight_u, weight_v, bias) and folded to a plain weight once a conv's tensors are all there: weight norm
 * v * (g / |v|) per output channel, spectral norm weight_orig / (u . (W_mat v)) with the STORED u, v (eval mode).
 * The real and the generated waveform run as one batch of 2 B.  Every feature map and logit row lives in an arena of
 * gvc_disc_arena_floats floats that the caller owns (gvc_disc_set_arena) and may read after a forward: layer `layer` of
 * sub-discriminator `sub` is [2 B][C][H][W] (MSD: W = 1) at the offset gvc_disc_layer reports, items [0, B) real and
 * [B, 2 B) generated -- the reference's layouts, overwritten by the next forward.
 * ------------------------------------------------------------------------------------------ */
#define GVC_DISC_MSD 0
#define GVC_DISC_MPD 1
#define GVC_DISC_MAX_SUB 8
typedef struct gvc_disc gvc_disc;
typedef struct gvc_disc_dims {
    int32_t kind;                        /* GVC_DISC_MSD (3 scales, the first spectral-normed) or GVC_DISC_MPD */
    int32_t n_sub;                       /* MPD: number of periods (<= GVC_DISC_MAX_SUB); MSD: 3 */
    int32_t periods[GVC_DISC_MAX_SUB];   /* MPD */
    int32_t channels[5];                 /* MPD: int(32 m), int(128 m), int(512 m), int(1024 m), int(1024 m); multiples of 16 */
    int32_t spectral_norm;               /* MPD: mpd_use_spectral_norm */
    int32_t max_batch, max_samples;      /* B (not 2 B) and T */
} gvc_disc_dims;
int gvc_disc_create(const gvc_disc_dims* dims, gvc_disc** out);
int gvc_disc_destroy(gvc_disc* ctx);
int gvc_disc_bind_weight(gvc_disc* ctx, const char* name, const float* src, int64_t numel, gvc_stream s);
int gvc_disc_missing_weights(gvc_disc* ctx);
/* the folded weight of conv `layer` (n_layers - 1 = conv_post) of `sub` as [C_out][C_in / groups][k] -> out (numel floats) */
int gvc_disc_folded_weight(gvc_disc* ctx, int32_t sub, int32_t layer, float* out, int64_t numel, gvc_stream s);
int64_t gvc_disc_arena_floats(gvc_disc* ctx);
int gvc_disc_set_arena(gvc_disc* ctx, float* arena);
/* layers per sub-discriminator, conv_post included (MSD 8, MPD 6) */
int gvc_disc_layers(gvc_disc* ctx);
/* geometry of one feature map at (B, T): offset into the arena and C, H, W; the last layer is the logits [2 B][1][H][W] */
int gvc_disc_layer(gvc_disc* ctx, int32_t sub, int32_t layer, int32_t B, int32_t T, int64_t* offset, int32_t* C, int32_t* H, int32_t* W);
/* y, y_hat [B][T] -> feature maps and logits in the arena, and stats [n_sub][3 + gvc_disc_layers]: mean((1 - d_r)^2),
 * mean(d_g^2), mean((1 - d_g)^2), then mean|f_r - f_g| per layer.  The reductions have a fixed partition and order and use no
 * float atomics: the same input gives the same bits.  One captured graph per (B, T).  T must exceed every period. */
int gvc_disc_forward(gvc_disc* ctx, const float* y, const float* y_hat, int32_t B, int32_t T, float* stats, gvc_stream s);
/* measurement: layer `layer` of `sub` alone, `iters` back-to-back launches on the arena's current contents (after a forward at the
 * same (B, T)) between two events -> microseconds per launch; synchronises */
int gvc_disc_time_layer(gvc_disc* ctx, int32_t sub, int32_t layer, int32_t B, int32_t T, int32_t iters, float* avg_us, gvc_stream s);
/* out[0] = scale * mean|a - b| over n floats, reduced in a fixed order; work: 512 floats, 8-byte aligned */
int gvc_l1_mean(const float* a, const float* b, int64_t n, float scale, float* out, float* work, gvc_stream s);

/* The mel extractor of layers/hifigan_loss.py:16-75 (and, with other options, any variant of the front end above). */
#define GVC_MEL_SLANEY_SCALE 1           /* librosa's default mel scale (linear below 1 kHz, logarithmic above); 0: HTK */
#define GVC_MEL_MAGNITUDE 2              /* sqrt(re^2 + im^2 + 1e-9); 0: power */
#define GVC_MEL_PAD_HALF_OVERLAP 4       /* reflect (n_fft - hop) / 2 per side, center=False: T / hop frames; 0: n_fft / 2, 1 + T / hop */
typedef struct gvc_mel_options {
    int32_t n_fft, hop, win, sample_rate, n_mels, flags;
    float f_min, f_max;
    const float* mel_norms_host;         /* [n_mels] or NULL (no norms) */
} gvc_mel_options;
int gvc_mel_create_ex(const gvc_mel_options* opt, gvc_mel** out);
/* frames gvc_mel_forward writes for T samples (<= 0: too short for the reflect padding) */
int gvc_mel_frames(gvc_mel* ctx, int32_t T);

/* ------------------------------------------------------------------------------------------
 * Mel inversion and Griffin-Lim.  Replaces utils.py:TorchMelSpectrogram.invert (:164-172): exp(mel * norms), then
 * torchaudio.transforms.InverseMelScale (the minimum-norm least-squares inverse of the HTK / Slaney-normalised filterbank, relu'd), then
 * librosa.griffinlim (zero-padded centred STFT, periodic Hann, momentum) on the result AS A MAGNITUDE, as the reference passes it.
 *
 * The inverse matrix W [n_freq][n_mels] = fb (fb^T fb)^-1 is built at creation on the host in double (Cholesky of the Gram matrix) and
 * stored as fp32; a filterbank without an inverse (a filter with no bin) is GVC_ERR_ARG and the message names the filter.
 * Supported: n_fft a power of two in [512, 2048], win <= n_fft, hop divides win, win / hop >= 2; anything else is GVC_ERR_ARG.
 * B > max_batch or F > max_frames in gvc_gl_run is GVC_ERR_ARG (capacity, as for the other engines): create a larger context.
 * No atomics, fixed summation orders: the same input gives the same bits.  gvc_gl_run enqueues n_iter + 2 launches.
 * ------------------------------------------------------------------------------------------ */
typedef struct gvc_gl gvc_gl;
typedef struct gvc_gl_options {
    int32_t n_fft, hop, win, sample_rate, n_mels;
    int32_t max_batch, max_frames;       /* capacity of gvc_gl_run */
    float f_min, f_max;
} gvc_gl_options;
int gvc_gl_create(const gvc_gl_options* opt, const float* mel_norms_host_or_null, gvc_gl** out);
int gvc_gl_destroy(gvc_gl* ctx);
/* W [n_freq][n_mels] -> HOST memory */
int gvc_gl_inverse_matrix(gvc_gl* ctx, float* W);
/* mel [B][n_mels][F] (normalised log power mel) -> spec [B][n_freq][F] = relu(W exp(mel * norms)) */
int gvc_gl_inverse_mel(gvc_gl* ctx, const float* mel, int32_t B, int32_t F, float* spec, gvc_stream s);
/* angles [B][n_freq][F] complex64 (interleaved re, im) = exp(2 pi i u), u from the sampler's counter-based generator keyed by
 * (seed, item, bin, frame): independent of the launch geometry and of B, F of other entries */
int gvc_gl_init_angles(gvc_gl* ctx, uint64_t seed, int32_t B, int32_t F, void* angles, gvc_stream s);
/* spec [B][n_freq][F], init_angles [B][n_freq][F] complex64 -> wav [B][hop (F - 1)] after n_iter >= 0 iterations with momentum in
 * [0, 1) (librosa's alpha = momentum / (1 + momentum)); n_iter = 0 is istft(spec * init_angles).  F >= 2. */
int gvc_gl_run(gvc_gl* ctx, const float* spec, const void* init_angles, int32_t B, int32_t F, int32_t n_iter, float momentum,
               float* wav, gvc_stream s);
/* kernel launches this context has enqueued so far (measurement) */
long long gvc_gl_launches(gvc_gl* ctx);

#ifdef __cplusplus
}
#endif
#endif /* GENVC_HIP_H */
