// Deterministic beam search on the device (include/genvc_hip.h: gvc_beam_state, gvc_beam_select, gvc_gpt_beam_generate):
// the select step (log-softmax, repetition penalty, running score, top-2K, hypothesis walk, ids gather, slot permutation) and the
// KV span copies a reorder needs.  The step graph that chains them with the decode step lives in gpt.hip.
#pragma once
#include "common.h"
#include "logits_proc.h"

namespace gvc {

constexpr int kBeamMaxK = 16;                 // 2K <= 32 candidates: one wave sorts them
constexpr int kBeamThreads = 512;
constexpr int kBeamMaxN = kBeamMaxK * 1026;   // candidates per item the register-resident select holds
constexpr int kBeamPer = (kBeamMaxN + kBeamThreads - 1) / kBeamThreads;

// parameters of one gvc_gpt_beam_generate call, resident on the device so the captured step graph is independent of them
struct BeamCall {
    gvc_beam_state st;
    int32_t step;                 // t of the next select (advanced by the span-copy launch of every step)
    int32_t has_proc;             // proc applies (gvc_gpt_beam_generate_proc); 0: the select step computes what it does without it
    gvc_logits_processors proc;
    gvc_beam_groups grp;          // gvc_gpt_group_beam_generate: the groups of the call (the plain search never reads it)
};

int beam_check(const gvc_beam_state& st);
// one select step: st by value (call == nullptr, step t) or from the device-resident call (graph replay: call->st, call->step).
// seq_len / mel_pos (nullable): per-slot decode state, copied from a copy's source slot to its destination; tok_buf (nullable): a second
// home of the next tokens (the decode step's input)
// proc (device, nullable) serves the by-value form; graph replay reads call->has_proc / call->proc
int launch_beam_select(const gvc_beam_state& st, const gvc_logits_processors* proc, const BeamCall* call, int B, int K, const float* logits, int32_t* slots, int t,
                       int32_t* seq_len, int32_t* mel_pos, int32_t* tok_buf, hipStream_t s);
// group (diverse) beam search (include/genvc_hip.h: gvc_beam_groups): the groups' own checks; one select step that walks the G
// groups of every item inside one launch (grp by value, or call->grp on graph replay; the other arguments as launch_beam_select);
// src[r] = slots[(r / K) * K], the fan-out source of every row (the prefilled slot of its item)
int group_beam_check(const gvc_beam_state& st, const gvc_beam_groups& grp);
int launch_group_beam_select(const gvc_beam_state& st, const gvc_beam_groups& grp, const gvc_logits_processors* proc, const BeamCall* call,
                             int B, const float* logits, int32_t* slots, int t, int32_t* seq_len, int32_t* mel_pos, int32_t* tok_buf,
                             hipStream_t s);
int launch_group_fan_src(const int32_t* slots, int32_t* src, int BK, int K, hipStream_t s);
// the spans of the last select's copy lists (call->st.copies), for every (layer, k|v, head) run of the cache
// [L][2][slot][H][max_seq][hd] (esz bytes per element); a fixed grid over B*(K-1) possible copies (graph replay) with early exit.
// Advances call->step by one
int launch_kv_copy_span(BeamCall* call, int B, int K, void* kv, int n_layer, int n_head, int max_seq, int hd, int max_slots, int esz,
                        const int32_t* seq_len, hipStream_t s);
// whole-slot fan-out (gvc_gpt_kv_fanout): pair i copies positions [0, seq_len[src_slots[i]]) of every (layer, k|v, head) run of the same
// cache layout from slot src_slots[i] to slot dst_slots[i], with the slot's seq_len / mel_pos / pending token and its parked logits / latent; a fixed
// grid of (runs, n pairs) workgroups (device arrays)
int launch_kv_fanout(const int32_t* src_slots, const int32_t* dst_slots, int n, void* kv, int n_layer, int n_head, int max_seq, int hd,
                     int max_slots, int esz, int32_t* seq_len, int32_t* mel_pos, float* slot_logits, int vocab, float* slot_latent, int d,
                     int32_t* pending, hipStream_t s);
// start / end of a gvc_gpt_beam_generate call: store the call state (and the processors, host proc nullable), un-park (park) the
// logits of every beam row
// grp (host, nullable): the groups of a group search
int launch_beam_begin(BeamCall* dst, const gvc_beam_state& st, const gvc_logits_processors* proc, const gvc_beam_groups* grp, int i0,
                      const int32_t* slots_in, int32_t* slot_table, float* logits, const float* slot_logits, hipStream_t s);
int launch_beam_end(const int32_t* slot_table, int32_t* slots_out, int BK, const float* logits, float* slot_logits, int vocab,
                    hipStream_t s);

}  // namespace gvc
