// Assisted (speculative) decoding on the device, greedy and sampled (include/genvc_hip.h: gvc_gpt_verify, gvc_gpt_truncate,
// gvc_spec_accept[_len], gvc_spec_accept_sample[_len], gvc_spec_lookup, gvc_gpt_generate_assisted, gvc_gpt_generate_assisted_sample,
// gvc_gpt_generate_lookup): the input rows and length
// bookkeeping of a multi-row verification pass, the rollback of a slot, and the accept steps.  The block stack and the head of the
// verification are the context's own (gpt.hip: run_rows, launch_head); the round loop that chains them with the draft context's decode
// steps lives there too.
//
// Speculative sampling draws with counters keyed by POSITION, not by round: row b deciding token t (0-based within the generation) uses
// u_draft(t) = rng_uniform(seed, t, 3b), u_acc(t) = rng_uniform(seed, t, 3b + 1), u_res(t) = rng_uniform(seed, t, 3b + 2), so a result does
// not depend on how rounds are grouped into calls.  The uniforms of a position that was drafted behind a rejection are reused when
// that position is drafted again: they were never looked at by anything that was kept, so the draws stay independent.
#pragma once
#include "common.h"

namespace gvc {

constexpr int kSpecThreads = 256;
constexpr int kSpecMaxVocab = 2048;     // one byte per vocabulary entry in LDS (the sampler's bound)
constexpr int kSpecMaxDrafts = 15;      // k: a round verifies k + 1 <= 16 rows per stream
constexpr int kSpecMaxRows = 128;       // rows of one verification pass (the skinny GEMMs' bound)
constexpr int kSpecMaxNgram = 8;        // prompt lookup: the longest suffix searched for
constexpr int kSpecMaxHistory = 2048;   // prompt lookup: ids of one row's history staged in LDS (8 KB)

// Row (b, t) of a verification pass: x[b * T + t] = mel_emb[toks[b][t]] + mel_pos[mel_pos_idx[slot b] + t], the token clamped into the
// vocabulary and the position into the table.  base_out[slot b] = the cache position of row (b, 0): seq_len[slot], or the last one at
// which T rows still end below max_seq - 1 (then *err = 950; a mel position past the table sets 951): see gvc_gpt_verify
int launch_spec_embed(float* x, const int32_t* toks, const int32_t* slots, int B, int T, const int32_t* seq_len, const int32_t* mel_pos_idx,
                      const float* mel_emb, const float* mel_pos, int d, int vocab, int max_seq, int max_mel_pos, int32_t* base_out,
                      int* err, hipStream_t s);
// behind the pass: length and mel position of every slot grow by T (a slot the embed launch flagged stays where it is)
int launch_spec_advance(int32_t* seq_len, int32_t* mel_pos_idx, const int32_t* slots, int B, int T, int max_seq, int max_mel_pos,
                        hipStream_t s);
// length and mel position of slot b go down by max(drop[b], 0), not below 0
int launch_spec_truncate(int32_t* seq_len, int32_t* mel_pos_idx, const int32_t* slots, int B, const int32_t* drop, hipStream_t s);
// start of a round on the draft side: the draft sampler's own row lengths and finished flags start from the target's, its step
// counter from 0, and row 0 of every stream's verification tokens is the pending token
// rows (nullable; a sampled generation): the draft sampler's keyed row of every stream as well -- the call's settings p, p.seed,
// rng_row = 3 b, rng_step0 = emitted[b]
int launch_spec_round_begin(const gvc_spec_state& st, int k1, int32_t* step_ctr, gvc_row_sampling* rows, const gvc_sample_params& p,
                            hipStream_t s);
// start of a round whose drafts come from prompt lookup (include/genvc_hip.h: gvc_spec_lookup): per stream, row 0 of the verification
// tokens is the pending token, rows 1..draft_len[b] the ids that followed the earliest earlier occurrence of the longest suffix (up to
// max_ngram ids) of ids[from .. ids_len), the rest the pending token again; q (nullable) [B][k + 1][vocab] gets the drafts' one-hot rows
int launch_spec_lookup(const gvc_spec_state& st, int k, int max_ngram, int from, int32_t* draft_len, float* q, int vocab, hipStream_t s);
int check_spec_lookup(const gvc_spec_state* st, int k, int max_ngram, int from, const int32_t* draft_len, int vocab);
// the accept step (include/genvc_hip.h: gvc_spec_accept_len); the arguments are checked by the callers.  draft_len (nullable, device
// [B]): drafts row b has; null: every row has k
int launch_spec_accept(const gvc_spec_state& st, int k, int appended, const float* logits, const float* latents, const int32_t* drafts,
                       int draft_stride, const int32_t* draft_len, const gvc_sample_params& p, const gvc_logits_processors* proc,
                       hipStream_t s);
// the accept step of speculative sampling (include/genvc_hip.h: gvc_spec_accept_sample_len): [d_1..d_k' behind the rows' ids when
// put_drafts,] k_spec_warp of the B * (k + 1) logits rows into p_rows, then k_spec_accept_sample; the arguments are checked by the
// callers.  draft_len as in launch_spec_accept
int launch_spec_accept_sample(const gvc_spec_state& st, int k, int appended, const float* logits, const float* latents,
                              const int32_t* drafts, int draft_stride, const int32_t* draft_len, bool put_drafts, const float* q,
                              float* p_rows, const gvc_sample_params& p, const gvc_logits_processors* proc, hipStream_t s);
// host-side checks of a sampled call: the workspaces (rows only when need_rows), top_k <= vocab, temperature and repetition penalty > 0
int check_spec_sampling(const float* q, const float* p_rows, const gvc_row_sampling* rows, bool need_rows, const gvc_sample_params* p);
// host-side checks of a state and a call's k
int check_spec_state(const gvc_spec_state* st, int k, const gvc_sample_params* p, const gvc_logits_processors* proc, bool workspace);

}  // namespace gvc
