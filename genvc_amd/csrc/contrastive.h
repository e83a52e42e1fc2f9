// Contrastive search on the device (include/genvc_hip.h: gvc_contrastive_state, gvc_gpt_contrastive_generate): the recall (processors,
// softmax, top-K candidates), the hidden rows (ln_f of the candidates' residual rows), the similarity of every candidate with the item's
// context rows, and the select step.  The step graph that chains them with the decode step over B*K rows lives in gpt.hip; the KV span
// copies are beam.hip's k_kv_copy_span.
#pragma once
#include "beam.h"

namespace gvc {

constexpr int kCsMaxK = 16;
constexpr int kCsThreads = 256;
constexpr int kCsPer = (GVC_PROC_VOCAB_WORDS * 32 + kCsThreads - 1) / kCsThreads;   // vocabulary entries per recall thread
constexpr int kCsRows = 16;          // context rows per similarity workgroup (4 waves x 4 rows)

// parameters of one gvc_gpt_contrastive_generate call, resident on the device so the captured step graph is independent of them.
// bc carries what k_kv_copy_span reads (bc.st.copies, bc.st.n_copies) and the step counter t (bc.step, advanced by that launch)
struct CsCall {
    BeamCall bc;
    gvc_contrastive_state st;
    int32_t has_proc;
    gvc_logits_processors proc;
};

// the context's contrastive buffers (allocated once, by gvc_gpt_warmup_contrastive or on first use)
struct CsBufs {
    float* ctx;          // [items][max_seq][d] context rows: ln_f of the prompt rows, then of every selected candidate
    float* ctx_norm;     // [items][max_seq] their L2 norms, stored when a row is appended
    float* h;            // [slots][d] ln_f of the last decode step's candidate rows
    float* h_norm;       // [slots]
    float* prob;         // [slots] candidate probabilities (softmax of the processed scores)
    float* part;         // [items][n_chunks][kCsMaxK] max cosine of each candidate over one chunk of context rows
    int32_t* sel;        // [items] candidate the last select chose (its logits row feeds the next recall)
    int32_t* copies;     // [items][K][3] KV span copies (k_kv_copy_span layout)
    int32_t* n_copies;   // [items]
    int max_items, max_seq, n_chunks, d;
};

// the shape limits of the kernels (K, B*K, vocab, d_model), shared by the calls and gvc_gpt_warmup_contrastive
int cs_check_shape(int B, int K, int vocab, int d);
int cs_check(const gvc_contrastive_state& st, int d);
int cs_alloc(CsBufs* bf, int max_items, int max_slots, int max_seq, int d);
void cs_free(CsBufs* bf);
// start of a call: store the call state (host proc nullable), copy the slot table, un-park each item's logits and latent into row b*K; i0 == 0
// also appends the prompt's hidden rows (st.hidden0) to the context and fans the prefix of slot b*K out to the item's other slots
int launch_cs_begin(CsCall* call, const CsBufs& bf, const gvc_contrastive_state& st, const gvc_logits_processors* proc, int i0,
                    const int32_t* slots_in, int32_t* slot_table, float* logits, const float* slot_logits, float* latent,
                    const float* slot_latent, int32_t* seq_len, int32_t* mel_pos, void* kv, int n_layer, int n_head, int max_seq, int hd,
                    int max_slots, int esz, hipStream_t s);
// one step's launches around the decode step: recall (before), hidden rows + similarity + select (after); B, K as captured
int launch_cs_recall(const CsCall* call, const CsBufs& bf, int B, const float* logits, const float* latent, int32_t* tok_buf,
                     hipStream_t s);
int launch_cs_hidden(const float* x, const CsBufs& bf, int rows, const float* w, const float* b, hipStream_t s);
int launch_cs_sim(const CsCall* call, const CsBufs& bf, int B, hipStream_t s);
int launch_cs_select(const CsCall* call, const CsBufs& bf, int B, const int32_t* tok_buf, const int32_t* slot_table, const int32_t* seq_len,
                     hipStream_t s);
// end of a call: park the logits and latent of each item's chosen candidate in slot b*K's slot_logits / slot_latent
int launch_cs_end(const CsBufs& bf, const int32_t* slots, int B, int K, const float* logits, float* slot_logits, int vocab,
                  const float* latent, float* slot_latent, hipStream_t s);

}  // namespace gvc
