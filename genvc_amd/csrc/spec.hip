// Assisted (speculative) decoding: the kernels around a verification pass and the accept steps (spec.h).  The greedy accept step
// restates nothing of the sampler: the repetition penalty is k_sample_greedy's expression and the processors are logits_proc.h's
// device functions, run once per verified position at the length the row has there.  Speculative sampling restates nothing either:
// k_spec_warp IS the sampler's chain (sample_body.h: sample_row<true>) on the k + 1 verification rows, and the draft's rows come
// from k_sample itself (SampleCall::scores_out).  k_spec_accept_sample only compares and draws.
//
// RNG of a sampled generation: counters are keyed by POSITION, not by round.  Deciding token t (0-based index within the generation)
// of row b uses  u_draft(t) = rng_uniform(seed, t, 3b)  for the draft's draw,  u_acc(t) = rng_uniform(seed, t, 3b + 1)  for the accept
// test and  u_res(t) = rng_uniform(seed, t, 3b + 2)  for the residual / bonus / opening draw, so a result does not depend on how rounds
// are grouped into calls.  A position that was drafted BEHIND a rejection is drafted again in a later round with the same u_draft,
// u_acc and u_res: none of them was ever looked at by a decision that was kept (the draft tokens behind a rejection are discarded
// unread, and the accept loop stops at the rejection), so every uniform that reaches an emitted token is used for exactly one
// decision and the draws stay independent.
#include "spec.h"

#include "logits_proc.h"
#include "sample_body.h"

namespace gvc {

__global__ void k_spec_embed(float* x, const int32_t* toks, const int32_t* slots, int T, const int32_t* seq_len, const int32_t* mel_pos_idx,
                             const float* mel_emb, const float* mel_pos, int d, int vocab, int max_seq, int max_mel_pos, int32_t* base_out,
                             int* err) {
    const int row = blockIdx.x, b = row / T, t = row - b * T;
    const int slot = slots[b];
    const int mp = mel_pos_idx[slot];
    if (t == 0 && threadIdx.x == 0) {
        const int len = seq_len[slot];
        const bool full = len + T > max_seq - 1;
        base_out[slot] = full ? max(max_seq - 1 - T, 0) : len;
        if (full && err) *err = 950;
        if (mp + T > max_mel_pos - 1 && err) *err = 951;
    }
    const float* e = mel_emb + (size_t)min(max(toks[row], 0), vocab - 1) * d;
    const float* p = mel_pos + (size_t)min(max(mp + t, 0), max_mel_pos - 1) * d;
    float* dst = x + (size_t)row * d;
    for (int k = threadIdx.x * 4; k < d; k += blockDim.x * 4) {
        const float4 a = *reinterpret_cast<const float4*>(e + k);
        const float4 c = *reinterpret_cast<const float4*>(p + k);
        *reinterpret_cast<float4*>(dst + k) = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
}

__global__ void k_spec_advance(int32_t* seq_len, int32_t* mel_pos_idx, const int32_t* slots, int B, int T, int max_seq, int max_mel_pos) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int slot = slots[b];
    if (seq_len[slot] + T <= max_seq - 1) seq_len[slot] += T;
    if (mel_pos_idx[slot] + T <= max_mel_pos - 1) mel_pos_idx[slot] += T;
}

__global__ void k_spec_truncate(int32_t* seq_len, int32_t* mel_pos_idx, const int32_t* slots, int B, const int32_t* drop) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int slot = slots[b], n = max(drop[b], 0);
    seq_len[slot] = max(seq_len[slot] - n, 0);
    mel_pos_idx[slot] = max(mel_pos_idx[slot] - n, 0);
}

__global__ void k_spec_round_begin(gvc_spec_state S, int k1, int32_t* step_ctr, gvc_row_sampling* rows, gvc_sample_params p) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *step_ctr = 0;
    if (b >= S.B) return;
    S.d_ids_len[b] = S.ids_len[b];
    S.d_finished[b] = S.finished[b];
    S.v_toks[(size_t)b * k1] = S.pending[b];
    if (rows) {
        // the draft sampler's keyed row: the call's settings, and u_draft of the position its first draft decides
        gvc_row_sampling r;
        r.repetition_penalty = p.repetition_penalty; r.temperature = p.temperature; r.top_p = p.top_p; r.top_k = p.top_k;
        r.seed = p.seed; r.rng_row = 3 * b; r.rng_step0 = S.emitted[b];
        rows[b] = r;
    }
}

// Prompt lookup (spec.h: launch_spec_lookup): the draft side of a round without a draft model, and the round's begin.  One workgroup
// per stream.  The history h = ids[from .. ids_len) is staged in LDS; for n = min(max_ngram, len - 1) down to 1 thread t tests the start
// indices t, t + 256, .. (ascending, so its first hit is its lowest), the lowest hit of the workgroup is found by a wave reduction and
// four LDS words, and the loop leaves at the first n with a hit: len, n and the reduced index are the same in every thread, so every
// barrier is reached by all of them.  Plain stores only
__global__ __launch_bounds__(kSpecThreads) void k_spec_lookup(gvc_spec_state S, int k, int max_ngram, int from, int32_t* draft_len,
                                                              float* q, int V) {
    __shared__ int32_t h[kSpecMaxHistory];
    __shared__ int red[kSpecThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pend = S.pending[b];
    int32_t* vt = S.v_toks + (size_t)b * (k + 1);
    // (uniform over the workgroup: a finished row leaves before the first barrier)
    if (S.finished[b]) {
        if (tid <= k) vt[tid] = pend;
        if (tid == 0) draft_len[b] = 0;
        return;
    }
    const int32_t* ids = S.ids + (size_t)b * S.ids_stride + from;
    const int len = min(max(min(S.ids_len[b], S.ids_stride) - from, 0), kSpecMaxHistory);
    for (int i = tid; i < len; i += kSpecThreads) h[i] = ids[i];
    __syncthreads();
    int start = -1;          // index of the first draft in h
    for (int n = min(max_ngram, len - 1); n >= 1; --n) {
        const int32_t* suf = h + len - n;
        int best = 0x7fffffff;
        for (int i = tid; i + n < len; i += kSpecThreads) {
            bool eq = true;
            for (int j = 0; j < n; ++j) eq = eq && h[i + j] == suf[j];
            if (eq) { best = i; break; }
        }
        for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off));
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
        best = min(min(red[0], red[1]), min(red[2], red[3]));
        __syncthreads();          // red is written again for the next n
        if (best != 0x7fffffff) { start = best + n; break; }
    }
    const int cnt = start >= 0 ? min(k, len - start) : 0;
    // column 0: the pending token; columns 1..cnt: the drafts; the rest: the pending token again, a valid id nobody compares
    if (tid <= k) vt[tid] = tid >= 1 && tid <= cnt ? h[start + tid - 1] : pend;
    if (tid == 0) draft_len[b] = cnt;
    if (q) {
        // the one-hot row of draft j in the form the accept step reads (warped scores): 0 at the token and -inf elsewhere, which
        // weighs expf(0) = 1 there and nothing elsewhere -- probability exactly 1.0 at v_toks[b][j] and 0 at every other id
        for (int j = 1; j <= k; ++j) {
            const int tok = j <= cnt ? h[start + j - 1] : pend;
            float* row = q + ((size_t)b * (k + 1) + j) * V;
            for (int v = tid; v < V; v += kSpecThreads) row[v] = v == tok ? 0.f : -INFINITY;
        }
    }
}

// k' of a live row: min(k, budget[, draft_len[b]]) -- draft_len null is the count every row had before there was one
__device__ __forceinline__ int spec_drafts(int k, int budget, const int32_t* draft_len, int b) {
    const int kk = min(k, budget);
    return draft_len ? min(kk, max(draft_len[b], 0)) : kk;
}

// the call's processors BY VALUE as a kernel argument (the caller's struct is free when the launch is enqueued)
struct SpecProc {
    int on;
    gvc_logits_processors P;
};

__global__ __launch_bounds__(kSpecThreads) void k_spec_accept(gvc_spec_state S, int k, int appended, const float* logits,
                                                              const float* latents, const int32_t* drafts, int draft_stride,
                                                              const int32_t* draft_len, gvc_sample_params p, SpecProc pr) {
    __shared__ unsigned seen_w[kSpecMaxVocab / 4];          // one byte per vocabulary entry
    __shared__ float red_v[kSpecThreads / 64];
    __shared__ int red_i[kSpecThreads / 64];
    __shared__ uint32_t kill[kProcWords];
    __shared__ int s_tok;
    unsigned char* seen = reinterpret_cast<unsigned char*>(seen_w);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = p.vocab, eos = p.eos_token;
    const int len0 = S.ids_len[b], em0 = S.emitted[b];
    // (uniform over the workgroup: a finished row leaves before the first barrier)
    if (S.finished[b] || em0 >= S.max_new) {
        if (tid == 0) {
            S.finished[b] = 1;
            S.drop_target[b] = appended;
            S.drop_assistant[b] = appended;
        }
        return;
    }
    int32_t* ids = S.ids + (size_t)b * S.ids_stride;
    const int32_t* dr = drafts ? drafts + (size_t)b * draft_stride : nullptr;
    // drafts compared: HF's clamp of the draft length to the budget, and the row's own count where the draft source gives one
    const int kk = dr ? spec_drafts(k, S.max_new - em0 - 1, draft_len, b) : 0;
    const float rep_pen = p.repetition_penalty, temp = p.temperature;
    for (int i = tid; i < kSpecMaxVocab / 4; i += kSpecThreads) seen_w[i] = 0u;
    __syncthreads();
    for (int i = tid; i < min(len0, S.ids_stride); i += kSpecThreads) {
        const int id = ids[i];
        if (id >= 0 && id < V) seen[id] = 1;
    }
    int m = 0, acc = 0, last = eos;
    bool fin = false;
    for (int i = 0; i <= kk; ++i) {
        const int len = min(len0 + i, S.ids_stride);
        if (i > 0 && tid == 0) {
            const int dtok = dr[i - 1];
            if (len0 + i - 1 < S.ids_stride) ids[len0 + i - 1] = dtok;
            if (dtok >= 0 && dtok < V) seen[dtok] = 1;
        }
        ProcStep ps{false, 0.f, false};
        if (pr.on) ps = proc_row_begin(pr.P, len, pr.P.prompt_lens ? pr.P.prompt_lens[b] : pr.P.prompt_len, eos, kill, tid);
        __syncthreads();
        if (pr.on) {
            proc_ngram(ids, len, pr.P.no_repeat_ngram_size, V, kill, tid, kSpecThreads);
            __syncthreads();
        }
        // k_sample_greedy's chain on row i: repetition penalty, processors, temperature, argmax (the lower index wins a tie)
        const float* lg = logits + ((size_t)b * (k + 1) + i) * V;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = tid; j < V; j += kSpecThreads) {
            float x = lg[j];
            if (seen[j]) x = x < 0.f ? x * rep_pen : x / rep_pen;
            if (pr.on) x = proc_score(x, j, eos, ps, kill);
            x = x / temp;
            if (x > bv || (x == bv && j < bi)) { bv = x; bi = j; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kSpecThreads / 64; ++w)
                if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi)) { bv = red_v[w]; bi = red_i[w]; }
            const int tok = bi < V ? bi : 0;          // (every score NaN: any valid id, as the sampler)
            s_tok = tok;
            S.toks[(size_t)b * S.tok_stride + em0 + m] = tok;
            if (len0 + i < S.ids_stride) ids[len0 + i] = tok;
        }
        __syncthreads();
        last = s_tok;
        ++m;
        if (last == eos) { fin = true; break; }
        if (i < kk && last == dr[i]) ++acc;
        else break;
    }
    if (tid == 0) {
        S.ids_len[b] = min(len0 + m, S.ids_stride);
        S.emitted[b] = em0 + m;
        S.pending[b] = last;
        S.finished[b] = (fin || em0 + m >= S.max_new) ? 1 : 0;
        const int drop = appended > 0 ? appended - m : 0;
        S.drop_target[b] = drop;
        S.drop_assistant[b] = drop;
        if (appended > 0) {
            if (S.rounds) S.rounds[b] += 1;
            if (S.drafted) S.drafted[b] += kk;
            if (S.accepted) S.accepted[b] += acc;
        }
    }
    if (S.lats && latents) {
        // token j of this round was chosen from row j: its latent goes to the row's own emitted offset
        for (int j = 0; j < m; ++j) {
            const float* src = latents + ((size_t)b * (k + 1) + j) * S.d;
            float* dst = S.lats + ((size_t)b * S.lat_stride + em0 + j) * S.d;
            for (int q = tid * 4; q < S.d; q += kSpecThreads * 4)
                *reinterpret_cast<float4*>(dst + q) = *reinterpret_cast<const float4*>(src + q);
        }
    }
}

// ---- speculative sampling ---------------------------------------------------------------------------------------------------------
// d_1..d_k' behind the ids of every live row (the draft sampler has put them there in a generation; gvc_spec_accept_sample alone has
// only the draft array)
__global__ void k_spec_put_drafts(gvc_spec_state S, int k, const int32_t* drafts, int draft_stride, const int32_t* draft_len) {
    const int b = blockIdx.x, em0 = S.emitted[b];
    if (S.finished[b] || em0 >= S.max_new) return;
    const int kk = spec_drafts(k, S.max_new - em0 - 1, draft_len, b), len0 = S.ids_len[b];
    for (int j = threadIdx.x; j < kk; j += blockDim.x)
        if (len0 + j < S.ids_stride) S.ids[(size_t)b * S.ids_stride + len0 + j] = drafts[(size_t)b * draft_stride + j];
}

// p_i of verification row (b, i): the sampler's chain at ids length ids_len[b] + i, stored as the sampler stores scores_out.  One
// workgroup per row, so the sorts of a stream run side by side.  Rows of finished streams and rows behind the k' drafts the accept
// step compares return at once
__global__ __launch_bounds__(kSampThreads) void k_spec_warp(gvc_spec_state S, int k, const float* logits, float* p_out,
                                                            const int32_t* draft_len, gvc_sample_params p, SpecProc pr) {
    const int r = blockIdx.x, b = r / (k + 1), i = r - b * (k + 1);
    const int em0 = S.emitted[b];
    // (uniform over the workgroup)
    if (S.finished[b] || em0 >= S.max_new || i > spec_drafts(k, S.max_new - em0 - 1, draft_len, b)) return;
    SampleCall C = {};
    C.p = p;
    C.scores_warped = 1;
    sample_row<true>(C, b, logits + (size_t)r * p.vocab, S.ids + (size_t)b * S.ids_stride, min(S.ids_len[b] + i, S.ids_stride),
                     pr.on ? &pr.P : nullptr, p_out + (size_t)r * p.vocab, 0);
}

constexpr int kSpecPer = kSpecMaxVocab / kSpecThreads;          // 8 consecutive vocabulary entries per thread

// entries [8 tid, 8 tid + 8) of a scores row, -inf past the vocabulary; vector loads where the row's alignment allows
__device__ __forceinline__ void spec_load8(const float* row, int V, int tid, float* s) {
    const int i0 = tid * kSpecPer;
    const uintptr_t a = reinterpret_cast<uintptr_t>(row);
    if (i0 + kSpecPer <= V && (a & 15) == 0) {
        const float4 x = *reinterpret_cast<const float4*>(row + i0), y = *reinterpret_cast<const float4*>(row + i0 + 4);
        s[0] = x.x; s[1] = x.y; s[2] = x.z; s[3] = x.w; s[4] = y.x; s[5] = y.y; s[6] = y.z; s[7] = y.w;
    } else if (i0 + kSpecPer <= V && (a & 7) == 0) {
#pragma unroll
        for (int u = 0; u < kSpecPer; u += 2) {
            const float2 x = *reinterpret_cast<const float2*>(row + i0 + u);
            s[u] = x.x; s[u + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int u = 0; u < kSpecPer; ++u) s[u] = i0 + u < V ? row[i0 + u] : -INFINITY;
    }
}

// maxima of (a, b) over the workgroup of kSpecThreads; scr: [8] floats
__device__ __forceinline__ void spec_max2(float& a, float& b, float* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a = fmaxf(a, __shfl_xor(a, off)); b = fmaxf(b, __shfl_xor(b, off)); }
    __syncthreads();                         // scr may still be read from the row before
    if (lane == 0) { scr[wave] = a; scr[4 + wave] = b; }
    __syncthreads();
    a = fmaxf(fmaxf(scr[0], scr[1]), fmaxf(scr[2], scr[3]));
    b = fmaxf(fmaxf(scr[4], scr[5]), fmaxf(scr[6], scr[7]));
}

// exclusive prefix sums of (a, b) per thread over the workgroup of kSpecThreads in thread order (= vocabulary order); the totals in
// ta / tb.  scr: [8] doubles
__device__ __forceinline__ void spec_scan2(double& a, double& b, double* scr, double* ta, double* tb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double ia = a, ib = b;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double oa = __shfl_up(ia, off), ob = __shfl_up(ib, off);
        if (lane >= off) { ia += oa; ib += ob; }
    }
    __syncthreads();                         // scr may still be read from the scan before
    if (lane == 63) { scr[wave] = ia; scr[4 + wave] = ib; }
    __syncthreads();
    double ba = 0.0, bb = 0.0, sa = 0.0, sb = 0.0;
#pragma unroll
    for (int w = 0; w < kSpecThreads / 64; ++w) {
        if (w < wave) { ba += scr[w]; bb += scr[4 + w]; }
        sa += scr[w]; sb += scr[4 + w];
    }
    a = ba + ia - a; b = bb + ib - b;
    *ta = sa; *tb = sb;
}

// The accept rule of speculative sampling (include/genvc_hip.h: gvc_spec_accept_sample), one workgroup per stream.  q / p: the warped
// rows [B][k + 1][vocab] of the draft (row j: what d_j was drawn from) and of the target (row i: verification row i).  Only the rows up
// to the first rejection are read.  The bookkeeping is k_spec_accept's, field for field
__global__ __launch_bounds__(kSpecThreads) void k_spec_accept_sample(gvc_spec_state S, int k, int appended, const float* latents,
                                                                     const int32_t* drafts, int draft_stride,
                                                                     const int32_t* draft_len, const float* q, const float* p,
                                                                     gvc_sample_params sp) {
    __shared__ double dscr[8];
    __shared__ float fscr[8];
    __shared__ int s_pick, s_last, s_acc;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = sp.vocab, eos = sp.eos_token;
    const int len0 = S.ids_len[b], em0 = S.emitted[b];
    // (uniform over the workgroup: a finished row leaves before the first barrier)
    if (S.finished[b] || em0 >= S.max_new) {
        if (tid == 0) {
            S.finished[b] = 1;
            S.drop_target[b] = appended;
            S.drop_assistant[b] = appended;
        }
        return;
    }
    int32_t* ids = S.ids + (size_t)b * S.ids_stride;
    const int32_t* dr = drafts ? drafts + (size_t)b * draft_stride : nullptr;
    const int kk = dr ? spec_drafts(k, S.max_new - em0 - 1, draft_len, b) : 0;
    const int i0 = tid * kSpecPer;
    int m = 0, acc = 0, last = eos;
    bool fin = false;
    for (int i = 0; i <= kk; ++i) {
        const size_t r = (size_t)b * (k + 1) + i;
        const bool hasq = i < kk;
        float ps[kSpecPer], qs[kSpecPer];
        spec_load8(p + r * V, V, tid, ps);
        if (hasq) spec_load8(q + (r + 1) * V, V, tid, qs);
        else {
#pragma unroll
            for (int u = 0; u < kSpecPer; ++u) qs[u] = -INFINITY;
        }
        float pm = -INFINITY, qm = -INFINITY;
#pragma unroll
        for (int u = 0; u < kSpecPer; ++u) { pm = fmaxf(pm, ps[u]); qm = fmaxf(qm, qs[u]); }
        spec_max2(pm, qm, fscr);
        // the sampler's weights: expf(s - max) in fp32 for kept entries, summed in double in vocabulary order
        float wp[kSpecPer], wq[kSpecPer];
        double exP = 0.0, exQ = 0.0, totP, totQ;
#pragma unroll
        for (int u = 0; u < kSpecPer; ++u) {
            wp[u] = ps[u] > -INFINITY ? expf(ps[u] - pm) : 0.f;
            wq[u] = qs[u] > -INFINITY ? expf(qs[u] - qm) : 0.f;
            exP += (double)wp[u]; exQ += (double)wq[u];
        }
        spec_scan2(exP, exQ, dscr, &totP, &totQ);
        const int x = hasq ? dr[i] : -1;
        bool ok = false;
        if (hasq) {
            if (tid == 0) s_acc = 0;          // (a draft outside the vocabulary is rejected)
            __syncthreads();
            if (x >= 0 && x < V && (x >> 3) == tid) {
                double px = 0.0, qx = 0.0;
#pragma unroll
                for (int u = 0; u < kSpecPer; ++u)
                    if (u == (x & 7)) { px = (double)wp[u] / totP; qx = (double)wq[u] / totQ; }
                const double rr = (double)rng_uniform(sp.seed, (uint64_t)(em0 + i), (uint64_t)(3 * b + 1));
                s_acc = rr * qx <= px ? 1 : 0;          // no division by q: q(x) == 0 accepts
            }
            __syncthreads();
            ok = s_acc != 0;
        }
        int tok = x;
        if (!ok) {
            // one token from max(p - q, 0) behind a rejection (from p when that is empty), from p behind k' accepted drafts
            double w[kSpecPer], ex = 0.0, tot = 0.0, unused_a = 0.0, unused_t;
            bool resid = false;
            if (hasq) {
#pragma unroll
                for (int u = 0; u < kSpecPer; ++u) {
                    w[u] = fmax((double)wp[u] / totP - (double)wq[u] / totQ, 0.0);
                    ex += w[u];
                }
                spec_scan2(ex, unused_a, dscr, &tot, &unused_t);
                resid = tot > 0.0;          // (uniform: every thread holds the same total)
            }
            if (!resid) {
#pragma unroll
                for (int u = 0; u < kSpecPer; ++u) w[u] = (double)wp[u];
                ex = exP; tot = totP;
            }
            const double target = (double)rng_uniform(sp.seed, (uint64_t)(em0 + i), (uint64_t)(3 * b + 2)) * tot;
            // the sampler's inverse-CDF rule: the first kept index whose running mass reaches the target, else the last kept index
            int pick = 0x7fffffff, lastk = -1;
            double a = ex;
#pragma unroll
            for (int u = 0; u < kSpecPer; ++u) {
                a += w[u];
                const bool kept = resid ? w[u] > 0.0 : ps[u] > -INFINITY;
                if (kept) { lastk = i0 + u; if (a >= target && pick == 0x7fffffff) pick = i0 + u; }
            }
            if (tid == 0) { s_pick = 0x7fffffff; s_last = -1; }
            __syncthreads();
            if (pick != 0x7fffffff) atomicMin(&s_pick, pick);
            if (lastk >= 0) atomicMax(&s_last, lastk);
            __syncthreads();
            tok = s_pick != 0x7fffffff ? s_pick : (s_last >= 0 ? s_last : 0);
        }
        if (tid == 0) {
            S.toks[(size_t)b * S.tok_stride + em0 + m] = tok;
            if (len0 + i < S.ids_stride) ids[len0 + i] = tok;
        }
        last = tok;
        ++m;
        if (last == eos) { fin = true; break; }
        if (ok) ++acc;
        else break;
    }
    if (tid == 0) {
        S.ids_len[b] = min(len0 + m, S.ids_stride);
        S.emitted[b] = em0 + m;
        S.pending[b] = last;
        S.finished[b] = (fin || em0 + m >= S.max_new) ? 1 : 0;
        const int drop = appended > 0 ? appended - m : 0;
        S.drop_target[b] = drop;
        S.drop_assistant[b] = drop;
        if (appended > 0) {
            if (S.rounds) S.rounds[b] += 1;
            if (S.drafted) S.drafted[b] += kk;
            if (S.accepted) S.accepted[b] += acc;
        }
    }
    if (S.lats && latents) {
        for (int j = 0; j < m; ++j) {
            const float* src = latents + ((size_t)b * (k + 1) + j) * S.d;
            float* dst = S.lats + ((size_t)b * S.lat_stride + em0 + j) * S.d;
            for (int c = tid * 4; c < S.d; c += kSpecThreads * 4)
                *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(src + c);
        }
    }
}

int launch_spec_embed(float* x, const int32_t* toks, const int32_t* slots, int B, int T, const int32_t* seq_len, const int32_t* mel_pos_idx,
                      const float* mel_emb, const float* mel_pos, int d, int vocab, int max_seq, int max_mel_pos, int32_t* base_out,
                      int* err, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_embed, dim3(B * T), dim3(256), 0, s, x, toks, slots, T, seq_len, mel_pos_idx, mel_emb, mel_pos, d, vocab,
                       max_seq, max_mel_pos, base_out, err);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_spec_advance(int32_t* seq_len, int32_t* mel_pos_idx, const int32_t* slots, int B, int T, int max_seq, int max_mel_pos,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_spec_advance, dim3(cdiv(B, 64)), dim3(64), 0, s, seq_len, mel_pos_idx, slots, B, T, max_seq, max_mel_pos);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_spec_truncate(int32_t* seq_len, int32_t* mel_pos_idx, const int32_t* slots, int B, const int32_t* drop, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_truncate, dim3(cdiv(B, 64)), dim3(64), 0, s, seq_len, mel_pos_idx, slots, B, drop);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_spec_round_begin(const gvc_spec_state& st, int k1, int32_t* step_ctr, gvc_row_sampling* rows, const gvc_sample_params& p,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_spec_round_begin, dim3(cdiv(st.B, 64)), dim3(64), 0, s, st, k1, step_ctr, rows, p);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_spec_lookup(const gvc_spec_state& st, int k, int max_ngram, int from, int32_t* draft_len, float* q, int vocab, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_lookup, dim3(st.B), dim3(kSpecThreads), 0, s, st, k, max_ngram, from, draft_len, q, vocab);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_spec_accept(const gvc_spec_state& st, int k, int appended, const float* logits, const float* latents, const int32_t* drafts,
                       int draft_stride, const int32_t* draft_len, const gvc_sample_params& p, const gvc_logits_processors* proc,
                       hipStream_t s) {
    SpecProc pr;
    memset(&pr, 0, sizeof(pr));
    if (proc) { pr.on = 1; pr.P = *proc; }
    hipLaunchKernelGGL(k_spec_accept, dim3(st.B), dim3(kSpecThreads), 0, s, st, k, appended, logits, latents, drafts, draft_stride,
                       draft_len, p, pr);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_spec_accept_sample(const gvc_spec_state& st, int k, int appended, const float* logits, const float* latents,
                              const int32_t* drafts, int draft_stride, const int32_t* draft_len, bool put_drafts, const float* q,
                              float* p_rows, const gvc_sample_params& p, const gvc_logits_processors* proc, hipStream_t s) {
    SpecProc pr;
    memset(&pr, 0, sizeof(pr));
    if (proc) { pr.on = 1; pr.P = *proc; }
    if (put_drafts && drafts && k > 0)
        hipLaunchKernelGGL(k_spec_put_drafts, dim3(st.B), dim3(64), 0, s, st, k, drafts, draft_stride, draft_len);
    hipLaunchKernelGGL(k_spec_warp, dim3(st.B * (k + 1)), dim3(kSampThreads), 0, s, st, k, logits, p_rows, draft_len, p, pr);
    hipLaunchKernelGGL(k_spec_accept_sample, dim3(st.B), dim3(kSpecThreads), 0, s, st, k, appended, latents, drafts, draft_stride,
                       draft_len, q, (const float*)p_rows, p);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int check_spec_sampling(const float* q, const float* p_rows, const gvc_row_sampling* rows, bool need_rows, const gvc_sample_params* p) {
    GVC_REQUIRE(p, GVC_ERR_ARG, "spec sampling: null argument");
    GVC_REQUIRE(q && p_rows && (rows || !need_rows), GVC_ERR_ARG, "spec sampling: a null workspace array");
    GVC_REQUIRE(p->temperature > 0.f && p->top_k <= p->vocab && p->repetition_penalty > 0.f, GVC_ERR_ARG,
                "spec sampling: temperature %g, top_k %d (vocab %d), repetition_penalty %g", (double)p->temperature, p->top_k, p->vocab,
                (double)p->repetition_penalty);
    return GVC_OK;
}

int check_spec_state(const gvc_spec_state* st, int k, const gvc_sample_params* p, const gvc_logits_processors* proc, bool workspace) {
    GVC_REQUIRE(st && p, GVC_ERR_ARG, "spec: null argument");
    GVC_REQUIRE(k >= 0 && k <= kSpecMaxDrafts, GVC_ERR_ARG, "spec: %d draft tokens outside [0, %d]", k, kSpecMaxDrafts);
    GVC_REQUIRE(st->B >= 1 && st->B * (k + 1) <= kSpecMaxRows, GVC_ERR_ARG, "spec: %d streams x %d rows exceed %d rows", st->B, k + 1,
                kSpecMaxRows);
    GVC_REQUIRE(st->ids && st->ids_len && st->finished && st->emitted && st->pending && st->toks && st->drop_target && st->drop_assistant,
                GVC_ERR_ARG, "spec: a null state array");
    GVC_REQUIRE(st->max_new >= 1 && st->tok_stride >= st->max_new && st->ids_stride >= 1, GVC_ERR_ARG,
                "spec: max_new %d, tok_stride %d, ids_stride %d", st->max_new, st->tok_stride, st->ids_stride);
    GVC_REQUIRE(!st->lats || (st->d >= 4 && st->d % 4 == 0 && st->lat_stride >= st->max_new), GVC_ERR_ARG,
                "spec: latents need d %% 4 == 0 and lat_stride >= max_new (d %d, lat_stride %d)", st->d, st->lat_stride);
    GVC_REQUIRE(p->vocab >= 1 && p->vocab <= kSpecMaxVocab, GVC_ERR_UNSUPPORTED, "spec: vocab %d outside [1, %d]", p->vocab, kSpecMaxVocab);
    GVC_REQUIRE(p->eos_token >= 0 && p->eos_token < p->vocab && p->temperature > 0.f, GVC_ERR_ARG, "spec: bad eos token or temperature");
    GVC_REQUIRE(!workspace || (st->v_toks && st->v_logits && st->v_latents && st->d_ids_len && st->d_finished), GVC_ERR_ARG,
                "spec: a null workspace array");
    if (proc) return check_procs(*proc, p->vocab);
    return GVC_OK;
}

int check_spec_lookup(const gvc_spec_state* st, int k, int max_ngram, int from, const int32_t* draft_len, int vocab) {
    GVC_REQUIRE(st && draft_len, GVC_ERR_ARG, "spec lookup: null argument");
    GVC_REQUIRE(k >= 1 && k <= kSpecMaxDrafts, GVC_ERR_ARG, "spec lookup: %d draft tokens outside [1, %d]", k, kSpecMaxDrafts);
    GVC_REQUIRE(max_ngram >= 1 && max_ngram <= kSpecMaxNgram, GVC_ERR_ARG, "spec lookup: max_ngram %d outside [1, %d]", max_ngram,
                kSpecMaxNgram);
    GVC_REQUIRE(st->B >= 1 && st->ids_stride >= 1 && from >= 0 && vocab >= 1, GVC_ERR_ARG, "spec lookup: B %d, ids_stride %d, from %d, vocab %d",
                st->B, st->ids_stride, from, vocab);
    GVC_REQUIRE(st->ids && st->ids_len && st->finished && st->pending && st->v_toks, GVC_ERR_ARG, "spec lookup: a null state array");
    GVC_REQUIRE(st->ids_stride - from <= kSpecMaxHistory, GVC_ERR_ARG, "spec lookup: a history of up to %d ids (ids_stride %d - from %d) exceeds %d",
                st->ids_stride - from, st->ids_stride, from, kSpecMaxHistory);
    return GVC_OK;
}

}  // namespace gvc

using namespace gvc;

extern "C" int gvc_spec_lookup(const gvc_spec_state* st, int32_t k, int32_t max_ngram, int32_t from, int32_t* draft_len, float* q_scores,
                               int32_t vocab, gvc_stream sv) {
    int rc = check_spec_lookup(st, k, max_ngram, from, draft_len, vocab);
    if (rc) return rc;
    return launch_spec_lookup(*st, k, max_ngram, from, draft_len, q_scores, vocab, (hipStream_t)sv);
}

extern "C" int gvc_spec_accept_len(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                                   const int32_t* drafts, int32_t draft_stride, const int32_t* draft_len, const gvc_sample_params* p,
                                   const gvc_logits_processors* proc, gvc_stream sv) {
    int rc = check_spec_state(st, k, p, proc, false);
    if (rc) return rc;
    GVC_REQUIRE(logits && (k == 0 || (drafts && draft_stride >= k)) && (appended == 0 || appended == k + 1), GVC_ERR_ARG,
                "gvc_spec_accept: bad argument (k %d, appended %d, draft_stride %d)", k, appended, draft_stride);
    GVC_REQUIRE(!st->lats || latents, GVC_ERR_ARG, "gvc_spec_accept: a latent buffer without latent rows");
    return launch_spec_accept(*st, k, appended, logits, latents, k > 0 ? drafts : nullptr, draft_stride, draft_len, *p, proc, (hipStream_t)sv);
}

extern "C" int gvc_spec_accept(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                               const int32_t* drafts, int32_t draft_stride, const gvc_sample_params* p, const gvc_logits_processors* proc,
                               gvc_stream sv) {
    return gvc_spec_accept_len(st, k, appended, logits, latents, drafts, draft_stride, nullptr, p, proc, sv);
}

extern "C" int gvc_spec_accept_sample_len(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                                          const int32_t* drafts, int32_t draft_stride, const int32_t* draft_len, const float* q_scores,
                                          float* p_scores, const gvc_sample_params* p, const gvc_logits_processors* proc, gvc_stream sv) {
    int rc = check_spec_state(st, k, p, proc, false);
    if (rc) return rc;
    if ((rc = check_spec_sampling(k > 0 ? q_scores : p_scores, p_scores, nullptr, false, p))) return rc;
    GVC_REQUIRE(logits && (k == 0 || (drafts && draft_stride >= k)) && (appended == 0 || appended == k + 1), GVC_ERR_ARG,
                "gvc_spec_accept_sample: bad argument (k %d, appended %d, draft_stride %d)", k, appended, draft_stride);
    GVC_REQUIRE(!st->lats || latents, GVC_ERR_ARG, "gvc_spec_accept_sample: a latent buffer without latent rows");
    return launch_spec_accept_sample(*st, k, appended, logits, latents, k > 0 ? drafts : nullptr, draft_stride, draft_len, true, q_scores,
                                     p_scores, *p, proc, (hipStream_t)sv);
}

extern "C" int gvc_spec_accept_sample(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                                      const int32_t* drafts, int32_t draft_stride, const float* q_scores, float* p_scores,
                                      const gvc_sample_params* p, const gvc_logits_processors* proc, gvc_stream sv) {
    return gvc_spec_accept_sample_len(st, k, appended, logits, latents, drafts, draft_stride, nullptr, q_scores, p_scores, p, proc, sv);
}
