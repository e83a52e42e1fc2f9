// The body of the sampler's full kernel (sampler.hip: k_sample) and the workgroup primitives under it, in a header so that the
// speculative-sampling warp kernel (spec.hip: k_spec_warp) runs the SAME chain -- repetition penalty, processors, Temperature, TopK, TopP,
// MinP, the typical / epsilon / eta warpers -- on a verification row instead of restating it.  sample_row<false> is k_sample;
// sample_row<true> stops where the chain has stored the warped row and draws nothing.
#pragma once
#include "sampler.h"

namespace gvc {

constexpr int kSortN = 2048;          // vocab (1026) padded to a power of two
constexpr int kSampThreads = 1024;

__device__ __forceinline__ float rng_uniform(uint64_t seed, uint64_t step, uint64_t row) {
    // same integer hash as oracle/genvc_oracle.py:rng_uniform
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + step * 0xBF58476D1CE4E5B9ull + row * 0x94D049BB133111EBull +
                 0x2545F4914F6CDD1Dull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (float)(x >> 40) * (1.0f / 16777216.0f);
}

// exclusive prefix sum of one value per thread over the workgroup (kSampThreads = 16 waves) in thread order; *total = sum
template <typename T>
__device__ __forceinline__ T block_scan_excl(T v, T* scr /*[17]*/, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();                         // scr may still be read from a previous scan
    if (lane == 63) scr[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        T w = lane < kSampThreads / 64 ? scr[lane] : T(0);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const T o = __shfl_up(w, off);
            if (lane >= off) w += o;
        }
        if (lane < kSampThreads / 64) scr[lane] = w;
    }
    __syncthreads();
    const T base = wave > 0 ? scr[wave - 1] : T(0);
    *total = scr[kSampThreads / 64 - 1];
    return base + inc - v;
}

// sum of (a, b) over the workgroup, the same bits in every thread and on every run: the xor butterfly gives all 64 lanes of a wave one
// value (each pairing adds x + y and y + x, which round alike), and every thread adds the 16 wave sums in wave order.  scr: [32] floats
// that no thread reads past the leading barrier
template <int NT = kSampThreads>
__device__ __forceinline__ void block_sum2(float& a, float& b, float* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    __syncthreads();
    if (lane == 0) { scr[wave] = a; scr[16 + wave] = b; }
    __syncthreads();
    a = 0.f; b = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) { a += scr[w]; b += scr[16 + w]; }
}

template <int NT = kSampThreads>
__device__ __forceinline__ float block_max(float v, float* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    __syncthreads();
    if (lane == 0) scr[wave] = v;
    __syncthreads();
    v = -INFINITY;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) v = fmaxf(v, scr[w]);
    return v;
}

// LogitNormalization (gvc_logits_bias::renormalize) of the scores row a step has just stored: so[i] <- log_softmax(so)[i], in place,
// by the whole workgroup of NT threads.  The maximum comes off before exp, -inf entries stay and add nothing, and the sum is the
// fixed-order workgroup sum.  Nothing else reads the row: the tokens do not move.  scr: [32] floats
template <int NT>
__device__ void renorm_row(float* so, int V, float* scr) {
    __syncthreads();                         // the row as the other threads stored it
    float m = -INFINITY;
    for (int i = threadIdx.x; i < V; i += NT) m = fmaxf(m, so[i]);
    m = block_max<NT>(m, scr);
    float z = 0.f, unused = 0.f;
    for (int i = threadIdx.x; i < V; i += NT) {
        const float x = so[i];
        if (x > -INFINITY) z += expf(x - m);
    }
    block_sum2<NT>(z, unused, scr);
    const float lz = logf(z);
    for (int i = threadIdx.x; i < V; i += NT) {
        const float x = so[i];
        if (x > -INFINITY) so[i] = (x - m) - lz;
    }
}

// softmax mass (.x) and entropy (.y) of the survivors (k0, k1) of this thread's pair (s0, s1); m = the largest surviving score.
// HF's log_softmax / Categorical(logits).entropy() arithmetic: logp = (s - m) - log Z, H = -sum p logp
__device__ __forceinline__ float2 survivor_entropy(float s0, float s1, bool k0, bool k1, float m, float* scr) {
    const float e0 = k0 ? expf(s0 - m) : 0.f, e1 = k1 ? expf(s1 - m) : 0.f;
    float Z = e0 + e1, unused = 0.f;
    block_sum2(Z, unused, scr);
    const float lZ = logf(Z);
    float h = 0.f;
    if (k0) h -= (e0 / Z) * ((s0 - m) - lZ);
    if (k1) h -= (e1 / Z) * ((s1 - m) - lZ);
    block_sum2(h, unused, scr);
    return make_float2(Z, h);
}

// TypicalLogitsWarper -> EpsilonLogitsWarper -> EtaLogitsWarper (transformers' order) on the survivors k0 / k1 of this thread's pair
// (s0, s1); m: the largest surviving score; scr: [32] floats.  Returns the largest score that survives them (typical may drop the
// argmax; the cutoffs never drop it).  Every sum is a fixed-order workgroup sum: the same row, key and settings keep the same ids on
// every run.
__device__ float apply_warpers(const gvc_logits_warpers& W, float s0, float s1, bool& k0, bool& k1, float m, float* scr) {
    if (W.typical_p > 0.f) {
        const float2 zh = survivor_entropy(s0, s1, k0, k1, m, scr);
        const float lZ = logf(zh.x), H = zh.y;
        // key = |-logp - H| >= 0: its bit pattern orders like its value.  T = the smallest key value at which the mass of ids with
        // key <= T reaches typical_p (HF's sort / cumsum / last_ind), found bit by bit from the top: one fixed-order workgroup sum of
        // the mass at or below a candidate per bit (a radix select of radix 2 weighted by mass; radix 4 -- 16 digits of three sums --
        // measured slower)
        const float p0 = k0 ? expf(s0 - m) / zh.x : 0.f, p1 = k1 ? expf(s1 - m) / zh.x : 0.f;
        const uint32_t kb0 = k0 ? __float_as_uint(fabsf(-((s0 - m) - lZ) - H)) : 0xffffffffu;
        const uint32_t kb1 = k1 ? __float_as_uint(fabsf(-((s1 - m) - lZ) - H)) : 0xffffffffu;
        // One barrier per bit: the wave sums alternate between the two halves of scr, so a half is rewritten only after the barrier
        // of the next bit, which every thread passes once it has read that half
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        uint32_t T = 0;
        __syncthreads();                                         // (scr: survivor_entropy's last sum may still be read)
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = T | ((1u << bit) - 1u);       // T so far, this bit clear, every lower bit set
            float a = (kb0 <= cand ? p0 : 0.f) + (kb1 <= cand ? p1 : 0.f);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
            float* half = scr + ((bit & 1) << 4);
            if (lane == 0) half[wave] = a;
            __syncthreads();
            a = 0.f;
#pragma unroll
            for (int w = 0; w < kSampThreads / 64; ++w) a += half[w];
            if (!(a >= W.typical_p)) T |= 1u << bit;            // (no key reaches the mass: T ends above every key, all stay)
        }
        k0 = k0 && kb0 <= T;
        k1 = k1 && kb1 <= T;
        m = block_max(fmaxf(k0 ? s0 : -INFINITY, k1 ? s1 : -INFINITY), scr);
    }
    if (W.epsilon_cutoff > 0.f) {
        const float e0 = k0 ? expf(s0 - m) : 0.f, e1 = k1 ? expf(s1 - m) : 0.f;
        float Z = e0 + e1, unused = 0.f;
        block_sum2(Z, unused, scr);
        if (k0 && e0 / Z < W.epsilon_cutoff && s0 < m) k0 = false;
        if (k1 && e1 / Z < W.epsilon_cutoff && s1 < m) k1 = false;
    }
    if (W.eta_cutoff > 0.f) {
        const float2 zh = survivor_entropy(s0, s1, k0, k1, m, scr);
        const float eta = fminf(W.eta_cutoff, sqrtf(W.eta_cutoff) * expf(-zh.y));
        if (k0 && expf(s0 - m) / zh.x < eta && s0 < m) k0 = false;
        if (k1 && expf(s1 - m) / zh.x < eta && s1 < m) k1 = false;
    }
    return m;
}

// One row of a sampler call on one workgroup of kSampThreads.  b: the stream (its settings, key, processors and warpers); lg: its logits
// row [vocab]; ids / len: its input_ids row and length at this position; P: its processors (nullable); so: where the row the draw is
// taken from is stored (SampleCall::scores_out resolved by the caller, nullable); step: the RNG counter of the call.
// kWarpOnly: return behind that store -- nothing is drawn, no id, length, flag, token or latent is written
template <bool kWarpOnly>
__device__ __forceinline__ void sample_row(const SampleCall& C, int b, const float* lg, int32_t* ids, int len,
                                           const gvc_logits_processors* P, float* so, int step) {
    __shared__ float sc[kSortN];        // processed scores in vocabulary order
    __shared__ float srt[kSortN];       // descending sort of the scores
    __shared__ unsigned char seen[kSortN];
    __shared__ int cnt[kSortN];         // counts of a gvc_logits_penalties row (touched only by such a row)
    __shared__ float red_v[16];
    __shared__ int red_i[16];
    __shared__ int s_tok, s_nk, s_pick, s_last;
    __shared__ float fscr[17];
    __shared__ int iscr[17];
    __shared__ double dscr[17];
    __shared__ float wscr[32];
    __shared__ uint32_t kill[kProcWords];
    __shared__ BiasHits bh;
    __shared__ uint32_t wmg[kProcWords];          // this step's green list of a gvc_logits_watermark row (touched only by such a row)
    const int tid = threadIdx.x;
    const int V = C.p.vocab;
    // processor settings and RNG key of this row (uniform over the workgroup: one workgroup = one row)
    const gvc_row_sampling* R = C.rows ? C.rows + b : nullptr;
    const float rep_pen = R ? R->repetition_penalty : C.p.repetition_penalty;
    const float temp = R ? R->temperature : C.p.temperature;
    const float top_p = R ? R->top_p : C.p.top_p;
    const int top_k = R ? R->top_k : C.p.top_k;

    // sequence bias / bad words / forced EOS of the call (null: none of the lines that read Z runs)
    const gvc_logits_bias* Z = C.bias;
    const bool force = Z && Z->force_eos_at > 0 && len - Z->prompt_len == Z->force_eos_at - 1;
    const bool pr = P || Z;                   // a kill bitmap and a ProcStep exist

    // presence / frequency / windowed repetition penalties of the row (uniform; off: `cnt` is neither cleared, added to nor read)
    const PenRow Q = pen_row(C, b, len);
    for (int i = tid; i < kSortN; i += kSampThreads) seen[i] = 0;
    if (Q.on)
        for (int i = tid; i < kSortN; i += kSampThreads) cnt[i] = 0;
    ProcStep ps{false, 0.f, force};
    if (P) ps = proc_row_begin(*P, len, P->prompt_lens ? P->prompt_lens[b] : P->prompt_len, C.p.eos_token, kill, tid, force);
    else if (Z && tid < kProcWords) kill[tid] = 0u;
    if (Z && tid < 64) bias_match(*Z, ids, len, &bh, tid);
    // green-list watermark of the row (uniform; off: `wmg` is neither written nor read): the 33 words of this step's list, one
    // coalesced read by the first lanes, visible behind the barrier below.  The warp-only kernel never sees a table
    WmRow M{false, false, nullptr, 0, 0.f};
    if constexpr (!kWarpOnly) M = wm_row(C, b, ids, len);
    if (M.on && tid < M.words) wmg[tid] = M.row[tid];
    __syncthreads();
    for (int i = tid; i < len; i += kSampThreads) {
        const int id = ids[i];
        if (id >= 0 && id < V) {
            seen[id] = 1;
            if (i >= Q.lo) atomicAdd(&cnt[id], 1);          // (Q.lo == len without penalties; integer adds: any order, the same counts)
        }
    }
    // (a forced EOS overrides the bans of the processors ahead of it in HF's list: n-gram and bad words)
    if (P && !force) proc_ngram(ids, len, P->no_repeat_ngram_size, V, kill, tid, kSampThreads);
    if (Z && !force) bias_bans(*Z, bh, V, kill, tid);
    const uint32_t hits = Z ? bh.hit & (uint32_t)((1ull << Z->n_bias) - 1ull) : 0u;
    __syncthreads();
    // SequenceBias, RepetitionPenalty (every id of input_ids incl. the fake prefix, once; the counted ids of a windowed row), the
    // presence / frequency penalties, the processors, then Temperature
    for (int i = tid; i < kSortN; i += kSampThreads) {
        float v = -INFINITY;
        if (i < V) {
            v = bias_logit(lg[i], i, hits, bh);
            const int c = Q.on ? cnt[i] : 0;
            if (Q.windowed ? c > 0 : seen[i]) v = v < 0.f ? v * rep_pen : v / rep_pen;
            if (c > 0) v = pen_score(v, c, Q);
            if (pr) v = proc_score(v, i, C.p.eos_token, ps, kill);
            v = v / temp;
        }
        sc[i] = v;
        srt[i] = v;
    }
    __syncthreads();

    int tok;
    float rmx;          // the largest entry of sc (the redraw of a gvc_logits_ras row takes its weights relative to it)
    if (top_k == 1) {
        // exactly one candidate survives TopK(1): argmax of the penalised scores, first index on ties
        // (a watermarked row: of the scores with the bias on the green ids, one fp32 add each -- greedy search with the mark)
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int i = tid; i < V; i += kSampThreads) {
            const float x = M.on && wm_green(wmg, i) ? __fadd_rn(sc[i], M.bias) : sc[i];
            if (x > bv || (x == bv && i < bi)) { bv = x; bi = i; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kSampThreads / 64; ++w)
                if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi)) { bv = red_v[w]; bi = red_i[w]; }
            s_tok = bi < V ? bi : 0;          // (all scores NaN -- the step before produced garbage: any valid id, never an out-of-range one)
        }
        __syncthreads();
        tok = s_tok;
        rmx = sc[tok];
        if (so) {
            if (C.scores_warped) {
                // TopK(1): the entries that equal the maximum stay (HF keeps ties), at their temperature-scaled score
                const float top = M.on && wm_green(wmg, tok) ? __fadd_rn(sc[tok], M.bias) : sc[tok];
                for (int i = tid; i < V; i += kSampThreads) {
                    const float x = M.on && wm_green(wmg, i) ? __fadd_rn(sc[i], M.bias) : sc[i];
                    so[i] = x >= top ? x : -INFINITY;
                }
            } else {
                // greedy search has no Temperature: the row as it stood before the division above
                for (int i = tid; i < V; i += kSampThreads) {
                    float v = bias_logit(lg[i], i, hits, bh);
                    const int c = Q.on ? cnt[i] : 0;
                    if (Q.windowed ? c > 0 : seen[i]) v = v < 0.f ? v * rep_pen : v / rep_pen;
                    if (c > 0) v = pen_score(v, c, Q);
                    if (pr) v = proc_score(v, i, C.p.eos_token, ps, kill);
                    if (M.on && wm_green(wmg, i)) v = __fadd_rn(v, M.bias);          // (the mark is a processor: the biased row)
                    so[i] = v;
                }
            }
        }
    } else {
        // bitonic sort, descending.  Thread t keeps elements t and t + 1024 in registers; a partner at distance j < 64 is a
        // lane of the same wave (shuffle, no barrier), j = 1024 is the thread's own second element, and only the 14 stages
        // with 64 <= j <= 512 go through LDS (the 66 LDS + barrier stages of the plain version cost ~30 us per step).
        {
            float v0 = srt[tid], v1 = srt[tid + kSampThreads];
            for (int k = 2; k <= kSortN; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    const bool d0 = (tid & k) == 0, d1 = ((tid + kSampThreads) & k) == 0;
                    if (j == kSampThreads) {                       // only k == 2048: i = tid is the low index, descending
                        const float hi = fmaxf(v0, v1), lo = fminf(v0, v1);
                        v0 = hi; v1 = lo;
                    } else if (j >= 64) {
                        __syncthreads();
                        srt[tid] = v0; srt[tid + kSampThreads] = v1;
                        __syncthreads();
                        const float p0 = srt[tid ^ j], p1 = srt[(tid ^ j) + kSampThreads];
                        const bool low = (tid & j) == 0;
                        v0 = (low == d0) ? fmaxf(v0, p0) : fminf(v0, p0);
                        v1 = (low == d1) ? fmaxf(v1, p1) : fminf(v1, p1);
                    } else {
                        const float p0 = __shfl_xor(v0, j), p1 = __shfl_xor(v1, j);
                        const bool low = (tid & j) == 0;
                        v0 = (low == d0) ? fmaxf(v0, p0) : fminf(v0, p0);
                        v1 = (low == d1) ? fmaxf(v1, p1) : fminf(v1, p1);
                    }
                }
            }
            __syncthreads();
            srt[tid] = v0; srt[tid + kSampThreads] = v1;
            __syncthreads();
        }
        // Everything below is workgroup-parallel (a single lane doing the top-p / inverse-CDF loops over the vocabulary cost
        // ~120 us per step at top_k = 15 and ~330 us without top-k).  Thread t owns the element pair (2t, 2t+1).
        const float mx = srt[0];
        // TopK: keep scores >= k-th largest (ties kept); nk = how many lead the descending order
        float thresh = -INFINITY;
        if (top_k > 0 && top_k < V) thresh = srt[top_k - 1];
        if (tid == 0) s_nk = 0;
        __syncthreads();
        for (int i = tid; i < kSortN; i += kSampThreads) {
            const bool in = srt[i] >= thresh && srt[i] > -INFINITY;
            const bool nxt = i + 1 < kSortN && srt[i + 1] >= thresh && srt[i + 1] > -INFINITY;
            if (in && !nxt) s_nk = i + 1;                       // exactly one boundary in a sorted array
        }
        __syncthreads();
        const int nk = s_nk;
        if (top_p < 1.0f && nk > 1) {
            // ascending order j = 0..nk-1 <-> descending index nk-1-j; p_j = exp(s - max) / Z; drop the leading run with
            // cumulative mass <= 1 - top_p, always keeping the largest
            const int j0 = 2 * tid, j1 = 2 * tid + 1;
            const float e0 = j0 < nk ? expf(srt[nk - 1 - j0] - mx) : 0.f;
            const float e1 = j1 < nk ? expf(srt[nk - 1 - j1] - mx) : 0.f;
            float Z;
            (void)block_scan_excl<float>(e0 + e1, fscr, &Z);
            const float q0 = e0 / Z, q1 = e1 / Z;
            float tot;
            const float ex = block_scan_excl<float>(q0 + q1, fscr, &tot);
            const float c0 = ex + q0, c1 = c0 + q1;
            int removed = 0;
            if (j0 < nk - 1 && c0 <= 1.0f - top_p) ++removed;
            if (j1 < nk - 1 && c1 <= 1.0f - top_p) ++removed;
            int nrem;
            (void)block_scan_excl<int>(removed, iscr, &nrem);
            thresh = srt[nk - nrem - 1];
        }
        // draw: first kept vocabulary index whose running mass (double, vocabulary order) reaches u * total
        {
            const int i0v = 2 * tid, i1v = 2 * tid + 1;
            bool k0 = i0v < V && sc[i0v] >= thresh, k1 = i1v < V && sc[i1v] >= thresh;
            // MinP (after TopP): softmax(s)_i < min_p * max softmax  <=>  exp(s_i - max) < min_p; the top score always stays
            const float min_p = P ? P->min_p : 0.f;
            if (min_p > 0.f) {
                if (k0 && expf(sc[i0v] - mx) < min_p) k0 = false;
                if (k1 && expf(sc[i1v] - mx) < min_p) k1 = false;
            }
            // Typical / Epsilon / Eta (after MinP); off -- every field 0, or no warpers -- leaves the arithmetic as it was.  The
            // weights are taken relative to the largest surviving score (typical may drop mx)
            float dmx = mx;
            const gvc_logits_warpers* W = row_warps(C, b);
            if (W && (W->typical_p > 0.f || W->epsilon_cutoff > 0.f || W->eta_cutoff > 0.f))
                dmx = apply_warpers(*W, i0v < V ? sc[i0v] : -INFINITY, i1v < V ? sc[i1v] : -INFINITY, k0, k1, mx, wscr);
            // Green-list watermark, behind the last warper (transformers appends it there): the survivors that are green gain the
            // bias, one fp32 add; under selfhash only those among the GVC_WM_SELFHASH_TOP highest scores of the row (the survivors of
            // TopK / TopP / MinP / epsilon / eta lead the sorted order, so srt[39] is that threshold; ties at it keep more).  The draw
            // takes its weights relative to the largest biased survivor: one more workgroup maximum.  Off: b0 / b1 are the scores
            // the lines below read where k0 / k1 hold and nothing else runs
            float b0 = i0v < V ? sc[i0v] : -INFINITY, b1 = i1v < V ? sc[i1v] : -INFINITY;
            if (M.on) {
                const float t40 = M.self ? srt[GVC_WM_SELFHASH_TOP - 1] : -INFINITY;
                if (k0 && b0 >= t40 && wm_green(wmg, i0v)) b0 = __fadd_rn(b0, M.bias);
                if (k1 && b1 >= t40 && wm_green(wmg, i1v)) b1 = __fadd_rn(b1, M.bias);
                dmx = block_max(fmaxf(k0 ? b0 : -INFINITY, k1 ? b1 : -INFINITY), wscr);
            }
            if (so) {
                // what survives the last warper keeps its temperature-scaled score, not renormalised; thread t stores its pair
                const float o0 = k0 ? b0 : -INFINITY, o1 = k1 ? b1 : -INFINITY;
                if (i1v < V && (reinterpret_cast<uintptr_t>(so) & 7) == 0) {
                    *reinterpret_cast<float2*>(so + i0v) = make_float2(o0, o1);
                } else {
                    if (i0v < V) so[i0v] = o0;
                    if (i1v < V) so[i1v] = o1;
                }
            }
            if constexpr (kWarpOnly) return;          // (uniform: every thread is past the last barrier of the chain)
            const double w0 = k0 ? (double)expf(b0 - dmx) : 0.0, w1 = k1 ? (double)expf(b1 - dmx) : 0.0;
            double total;
            const double ex = block_scan_excl<double>(w0 + w1, dscr, &total);
            // the RNG counter is the position of the step in the whole run of the stream (i0 + step, or rng_step0 + step of a keyed
            // row), not in this call; a keyed row is numbered inside its own job, not by its place in the call
            const double target = (R ? (double)rng_uniform(R->seed, (uint64_t)(R->rng_step0 + step), (uint64_t)R->rng_row)
                                     : (double)rng_uniform(C.p.seed, (uint64_t)(C.i0 + step), (uint64_t)b)) * total;
            const double a0 = ex + w0, a1 = a0 + w1;
            int pick = 0x7fffffff, lastk = -1;
            if (k0) { lastk = i0v; if (a0 >= target) pick = i0v; }
            if (k1) { lastk = i1v; if (a1 >= target && pick == 0x7fffffff) pick = i1v; }
            if (tid == 0) { s_pick = 0x7fffffff; s_last = -1; }
            __syncthreads();
            if (pick != 0x7fffffff) atomicMin(&s_pick, pick);
            if (lastk >= 0) atomicMax(&s_last, lastk);
            __syncthreads();
            if (tid == 0) s_tok = s_pick != 0x7fffffff ? s_pick : (s_last >= 0 ? s_last : 0);
        }
        __syncthreads();
        tok = s_tok;
        rmx = mx;
    }

    if constexpr (kWarpOnly) return;
    // Repetition-aware sampling (gvc_logits_ras): the token stands unless it fills min_count of the row's last
    // `window` generated ids; then it is drawn again from the whole row as the chain left it ahead of truncation (sc).  Every
    // condition below is uniform over the workgroup; a row without RAS meets no barrier here
    if (const gvc_logits_ras* A = row_ras(C, b); A && !C.finished[b] && len < C.ids_stride) {
        const int n_gen = len - min(max(A->prompt_len, 0), len);          // the fake prompt ids never count
        const int w = min(min(A->window, GVC_RAS_MAX_WINDOW), n_gen);
        if (tid < 64) {                                                     // (wave 0: w <= 64 ids, ids[len - w .. len))
            const unsigned long long hit = __ballot(tid < w && ids[len - 1 - tid] == tok);
            if (tid == 0) s_nk = __popcll(hit);
        }
        __syncthreads();
        if (s_nk >= A->min_count && tok != C.p.eos_token) {
            // the draw's arithmetic on every finite entry: expf in fp32 relative to the row maximum, widened; running mass in double
            // in vocabulary order; first index that reaches u2 * total; else the last kept index
            const int i0v = 2 * tid, i1v = 2 * tid + 1;
            const bool k0 = i0v < V && sc[i0v] > -INFINITY, k1 = i1v < V && sc[i1v] > -INFINITY;
            const double w0 = k0 ? (double)expf(sc[i0v] - rmx) : 0.0, w1 = k1 ? (double)expf(sc[i1v] - rmx) : 0.0;
            double total;
            const double ex = block_scan_excl<double>(w0 + w1, dscr, &total);
            const double target = (R ? (double)rng_uniform(R->seed ^ GVC_RAS_SALT, (uint64_t)(R->rng_step0 + step), (uint64_t)R->rng_row)
                                     : (double)rng_uniform(C.p.seed ^ GVC_RAS_SALT, (uint64_t)(C.i0 + step), (uint64_t)b)) * total;
            const double a0 = ex + w0, a1 = a0 + w1;
            int pick = 0x7fffffff, lastk = -1;
            if (k0) { lastk = i0v; if (a0 >= target) pick = i0v; }
            if (k1) { lastk = i1v; if (a1 >= target && pick == 0x7fffffff) pick = i1v; }
            if (tid == 0) { s_pick = 0x7fffffff; s_last = -1; }          // (behind the scan's barriers: every thread has read s_tok)
            __syncthreads();
            if (pick != 0x7fffffff) atomicMin(&s_pick, pick);
            if (lastk >= 0) atomicMax(&s_last, lastk);
            __syncthreads();
            if (tid == 0) {
                s_tok = s_pick != 0x7fffffff ? s_pick : (s_last >= 0 ? s_last : tok);
                if (C.ras_redraws) C.ras_redraws[b] += 1;
            }
            __syncthreads();
            tok = s_tok;
        }
    }
    // finished rows emit the pad (= eos) token (stream_generator.py:861-864, 872-874); a row whose ids buffer is
    // full is finished too (the caller sized it for the whole run: nothing past it can be accounted for)
    if (C.finished[b] || len >= C.ids_stride) tok = C.p.eos_token;
    __syncthreads();
    if (tid == 0) {
        if (len < C.ids_stride) { ids[len] = tok; C.ids_len[b] = len + 1; }
        if (tok == C.p.eos_token) C.finished[b] = 1;
        C.tok_out[b] = tok;
        if (C.tokens_out) C.tokens_out[(size_t)b * C.tok_stride + C.i0 + step] = tok;
        if (C.run_flag) { *C.run_flag = 1; *const_cast<int32_t*>(C.step_ptr) = step + 1; }      // (every thread read `step` before the barriers above)
    }
    if (C.latents_out && C.latent_src) {
        const float* src = C.latent_src + (size_t)b * C.d;
        float* dst = C.latents_out + ((size_t)b * C.lat_stride + C.i0 + step) * C.d;
        for (int k = tid; k < C.d; k += kSampThreads) dst[k] = src[k];
    }
    if (C.logits_out) {
        const float* raw = C.logits_src ? C.logits_src + (size_t)b * V : lg;
        float* lo = step_row(C.logits_out, C, b, step);
        for (int i = tid; i < V; i += kSampThreads) lo[i] = raw[i];
    }
    if (Z && Z->renormalize && so) renorm_row<kSampThreads>(so, V, wscr);
}

}  // namespace gvc
