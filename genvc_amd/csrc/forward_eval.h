// The evaluation pass of GPT.forward (reference layers/gpt.py:375-537, the default call: losses, top-k accuracy and the mel logits of a
// padded batch) -- the launches that pass adds to the multi-row block stack of gpt.hip (include/genvc_hip.h: gvc_gpt_forward_rows,
// gvc_gpt_head_xent, gvc_perceiver_forward_masked).  Kernels in forward_eval.hip.
#pragma once
#include "common.h"

namespace gvc {

struct AttnArgs;      // gpt_kernels.h

// rows of a padded batch into x [B][n_cond + Lt + Lm][d] (gpt.py:476-480 and the concatenation of get_logits, :275-280):
// cond[b] (n_cond rows) | text_emb[text_ids[b][i]] + text_pos[i] | mel_emb[code_ids[b][i]] + mel_pos[i].  Ids are clamped to their tables
int launch_eval_embed(float* x, const float* cond, int n_cond, const int32_t* text_ids, int Lt, const int32_t* code_ids, int Lm, int B, int d,
                      const float* text_emb, const float* text_pos, int n_text, const float* mel_emb, const float* mel_pos, int vocab,
                      hipStream_t s);

// rows off .. off + n - 1 of every batch element: src [B][T][d] -> dst [B][n][d]
int launch_eval_gather(const float* src, float* dst, int B, int T, int off, int n, int d, hipStream_t s);

// the causal prefill attention of gpt_kernels.h (k_attention_tile / k_attention_tile_short, fp32 K/V) with the key-padding mask
// A.key_mask [batch][A.mask_stride] (nonzero = attend); every shape goes to the tile kernels, few tiles included
int launch_attention_tile_masked(int head_dim, int n_head, const AttnArgs& A, int batch, int max_keys, hipStream_t s);

// F.cross_entropy(ignore_index=-1, label_smoothing) and the top-k hit count over R logits rows [R][V] (row stride ldl), targets int32 [R]:
// one wave per row writes row_terms[r] = (nll, smoothing term, hit) -- zeros where the target is -1 --, then ONE workgroup sums the
// rows in a fixed order in double: sums = (loss, hits, count, mean nll).  No atomics: the same input gives the same bits.
//   nll = lse - x[t];  smoothing term = lse - mean_c x[c];  hit = #{c: x[c] > x[t]} < top_k;
//   loss = ((1 - ls) * sum nll + ls * sum smoothing) / count        (count = rows whose target is not -1)
int launch_head_xent(const float* logits, int ldl, const int32_t* targets, int R, int V, float label_smoothing, int top_k, float* row_terms,
                     double* sums, hipStream_t s);

// key mask uint8 [n] (nonzero = attend) -> int32 [n] (nonzero = excluded), what k_attn64_mfma<true> reads
int launch_mask_excluded(const uint8_t* key_mask, int32_t* excluded, int n, hipStream_t s);

}  // namespace gvc
