// Length and repetition logits processors (include/genvc_hip.h: gvc_logits_processors) restated on the device, shared by the sampler
// kernels (sampler.hip) and the beam select step (beam.hip).  Every processor except the EOS decay sets scores to -inf, and -inf is
// absorbing, so a row's bans (n-gram, min_length / min_new_tokens on EOS, suppress, begin_suppress) collapse into ONE bitmap over the
// vocabulary, built once per row and step in LDS; the per-score work is then the decay of the EOS score and one bit test.
#pragma once
#include "common.h"

namespace gvc {

constexpr int kProcWords = GVC_PROC_VOCAB_WORDS;

// host-side checks of a processor set (vocab <= 32 * kProcWords)
int check_procs(const gvc_logits_processors& P, int vocab);
// host-side checks of a call's sequence bias / bad words / forced EOS struct (include/genvc_hip.h: gvc_logits_bias)
int check_bias(const gvc_logits_bias& Z, int vocab);

// what the processors do to one row at one step, uniform over the row's workgroup (or the item's, for beams)
struct ProcStep {
    bool decay;        // the EOS score gets s + |s| * decay_c (when not already -inf)
    float decay_c;
    bool force_eos;    // ForcedEOSToken fires at this step: every score -inf, the EOS score 0 (gvc_logits_bias::force_eos_at)
};

__device__ __forceinline__ bool proc_bit(const uint32_t* bm, int i) { return (bm[i >> 5] >> (i & 31)) & 1u; }

// Row of length len (its prompt: plen ids) before the step: the scalar part.  Threads [0, kProcWords) each write one word of the
// bitmap `kill` (kProcWords words in LDS): the suppress set, the begin_suppress set at the first step, and the eos bit while
// min_length / min_new_tokens ban it.  The n-gram pass ORs into the same words after a barrier the caller places.  force_eos: HF's
// ForcedEOSToken, which comes behind min_length / min_new_tokens, fires at this step and overrides their ban of the eos
__device__ __forceinline__ ProcStep proc_row_begin(const gvc_logits_processors& P, int len, int plen, int eos, uint32_t* kill, int tid,
                                                   bool force_eos = false) {
    ProcStep ps;
    ps.force_eos = force_eos;
    const int nnew = len - plen;
    const bool eos_off = !force_eos && ((P.min_length > 0 && len < P.min_length) || (P.min_new_tokens > 0 && nnew < P.min_new_tokens));
    const bool begin = P.n_begin_suppress > 0 && len == plen;
    if (tid < kProcWords) {
        uint32_t w = P.n_suppress > 0 ? P.suppress[tid] : 0u;
        if (begin) w |= P.begin_suppress[tid];
        if (eos_off && (eos >> 5) == tid) w |= 1u << (eos & 31);
        kill[tid] = w;
    }
    const int idx = nnew - P.decay_start;             // HF: cur_len - regulation_start, regulation_start = start + prompt length
    ps.decay = P.decay_factor > 0.f && idx > 0;
    // pow in double, minus one, then one rounding to fp32: the Python scalar HF multiplies the fp32 |score| by
    ps.decay_c = ps.decay ? (float)(pow((double)P.decay_factor, (double)idx) - 1.0) : 0.f;
    return ps;
}

// NoRepeatNGram over ids[0, len): every window [j, j + n) whose first n - 1 ids equal the row's last n - 1 ids bans ids[j + n - 1]
// (n == 1: every id of the row).  Threads stride over the windows; atomicOr into kill.  O(len * (n - 1)) compares.
__device__ __forceinline__ void proc_ngram(const int32_t* ids, int len, int n, int V, uint32_t* kill, int tid, int nthreads) {
    if (n <= 0 || len < n) return;
    const int32_t* suf = ids + (len - n + 1);
    for (int j = tid; j + n <= len; j += nthreads) {
        bool m = true;
        for (int q = 0; q < n - 1; ++q)
            if (ids[j + q] != suf[q]) { m = false; break; }
        if (m) {
            const int x = ids[j + n - 1];
            if (x >= 0 && x < V) atomicOr(&kill[x >> 5], 1u << (x & 31));
        }
    }
}

// score x of vocabulary entry i after the repetition penalty -> after the processors (before temperature).  fp32 without
// contraction: HF adds |s| * c to s in two rounded fp32 operations
__device__ __forceinline__ float proc_score(float x, int i, int eos, const ProcStep& ps, const uint32_t* kill) {
    if (ps.force_eos) x = i == eos ? 0.f : -INFINITY;
    if (ps.decay && i == eos && x > -INFINITY) x = __fadd_rn(x, __fmul_rn(fabsf(x), ps.decay_c));
    if (proc_bit(kill, i)) x = -INFINITY;
    return x;
}

// ---- sequence bias / bad words (gvc_logits_bias; HF SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor) -------------------------
// What a row's workgroup keeps of the call's entries for one step, in LDS: which entries hit the row, and each entry's last id and value
struct BiasHits {
    uint32_t hit;                          // bit e: entry e's first len - 1 ids equal the row's last len - 1 ids
    int32_t last[GVC_BIAS_MAX_SEQS];       // entry e's last id: the one it biases or bans
    float val[GVC_BIAS_MAX_SEQS];
};

// Match: threads [0, n_bias + n_ban) of the workgroup's first wave compare one entry each with the tail of ids[0, len), at most
// GVC_BIAS_MAX_LEN - 1 loads.  The whole first wave calls this (it votes); the caller's next barrier publishes *H
__device__ __forceinline__ void bias_match(const gvc_logits_bias& Z, const int32_t* ids, int len, BiasHits* H, int tid) {
    const int n = Z.n_bias + Z.n_ban;
    bool m = false;
    if (tid < n) {
        const int L = Z.len[tid];
        m = L <= len;                                  // an entry longer than the row never hits (HF skips it)
        for (int q = 0; m && q < L - 1; ++q) m = Z.ids[tid][q] == ids[len - (L - 1) + q];
        H->last[tid] = Z.ids[tid][L - 1];
        H->val[tid] = Z.bias[tid];
    }
    const unsigned long long vote = __ballot(m);
    if (tid == 0) H->hit = (uint32_t)vote;
}

// the hit bad-word entries OR their last id into the kill bitmap (after the barrier behind bias_match / proc_row_begin)
__device__ __forceinline__ void bias_bans(const gvc_logits_bias& Z, const BiasHits& H, int V, uint32_t* kill, int tid) {
    if (tid >= Z.n_bias && tid < Z.n_bias + Z.n_ban && ((H.hit >> tid) & 1u)) {
        const int x = H.last[tid];
        if (x >= 0 && x < V) atomicOr(&kill[x >> 5], 1u << (x & 31));
    }
}

// logit x of vocabulary entry i -> x + bias, ahead of the repetition penalty.  HF builds the row's bias from zeros -- the length-1
// entries, then every hit longer entry in order, one rounded fp32 add each -- and adds it to the scores once; hits: H.hit masked to
// the n_bias sequence_bias entries (uniform over the workgroup).  The one place that computes it: every pass over the row calls this
__device__ __forceinline__ float bias_logit(float x, int i, uint32_t hits, const BiasHits& H) {
    if (!hits) return x;
    float acc = 0.f;
    for (uint32_t h = hits; h; h &= h - 1u) {
        const int e = __ffs(h) - 1;
        if (H.last[e] == i) acc = __fadd_rn(acc, H.val[e]);
    }
    return __fadd_rn(x, acc);
}

}  // namespace gvc
