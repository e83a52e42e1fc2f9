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

__global__ __launch_bounds__(kSampThreads) void k_sample(SampleCall cv, const SampleCall* cp) {
    __shared__ float sc[kSortN];        // processed scores in vocabulary order
    __shared__ float srt[kSortN];       // descending sort of the scores
    __shared__ unsigned char seen[kSortN];
    __shared__ float red_v[16];
    __shared__ int red_i[16];
    __shared__ int s_tok, s_nk, s_pick, s_last;
    __shared__ float fscr[17];
    __shared__ int iscr[17];
    __shared__ double dscr[17];
    __shared__ float wscr[32];
    __shared__ uint32_t kill[kProcWords];
    __shared__ BiasHits bh;
    const SampleCall& C = cp ? *cp : cv;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = C.p.vocab;
    const int step = C.step_ptr ? *C.step_ptr : C.step;
    const float* lg = C.logits + (size_t)b * V;
    int32_t* ids = C.ids + (size_t)b * C.ids_stride;
    const int len = C.ids_len[b];
    // processor settings and RNG key of this row (uniform over the workgroup: one workgroup = one row)
    const gvc_row_sampling* R = C.rows ? C.rows + b : nullptr;
    const float rep_pen = R ? R->repetition_penalty : C.p.repetition_penalty;
    const float temp = R ? R->temperature : C.p.temperature;
    const float top_p = R ? R->top_p : C.p.top_p;
    const int top_k = R ? R->top_k : C.p.top_k;
    const gvc_logits_processors* P = row_procs(C, b);

    // sequence bias / bad words / forced EOS of the call (null: none of the lines that read Z runs)
    const gvc_logits_bias* Z = C.bias;
    const bool force = Z && Z->force_eos_at > 0 && len - Z->prompt_len == Z->force_eos_at - 1;
    const bool pr = P || Z;                   // a kill bitmap and a ProcStep exist

    for (int i = tid; i < kSortN; i += kSampThreads) seen[i] = 0;
    ProcStep ps{false, 0.f, force};
    if (P) ps = proc_row_begin(*P, len, P->prompt_lens ? P->prompt_lens[b] : P->prompt_len, C.p.eos_token, kill, tid, force);
    else if (Z && tid < kProcWords) kill[tid] = 0u;
    if (Z && tid < 64) bias_match(*Z, ids, len, &bh, tid);
    __syncthreads();
    for (int i = tid; i < len; i += kSampThreads) {
        const int id = ids[i];
        if (id >= 0 && id < V) seen[id] = 1;
    }
    // (a forced EOS overrides the bans of the processors ahead of it in HF's list: n-gram and bad words)
    if (P && !force) proc_ngram(ids, len, P->no_repeat_ngram_size, V, kill, tid, kSampThreads);
    if (Z && !force) bias_bans(*Z, bh, V, kill, tid);
    const uint32_t hits = Z ? bh.hit & (uint32_t)((1ull << Z->n_bias) - 1ull) : 0u;
    __syncthreads();
    // SequenceBias, RepetitionPenalty (every id of input_ids incl. the fake prefix, once), the processors, then Temperature
    for (int i = tid; i < kSortN; i += kSampThreads) {
        float v = -INFINITY;
        if (i < V) {
            v = bias_logit(lg[i], i, hits, bh);
            if (seen[i]) v = v < 0.f ? v * rep_pen : v / rep_pen;
            if (pr) v = proc_score(v, i, C.p.eos_token, ps, kill);
            v = v / temp;
        }
        sc[i] = v;
        srt[i] = v;
    }
    __syncthreads();

    int tok;
    if (top_k == 1) {
        // exactly one candidate survives TopK(1): argmax of the penalised scores, first index on ties
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int i = tid; i < V; i += kSampThreads)
            if (sc[i] > bv || (sc[i] == bv && i < bi)) { bv = sc[i]; bi = i; }
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
        if (C.scores_out) {
            float* so = step_row(C.scores_out, C, b, step);
            if (C.scores_warped) {
                // TopK(1): the entries that equal the maximum stay (HF keeps ties), at their temperature-scaled score
                const float top = sc[tok];
                for (int i = tid; i < V; i += kSampThreads) so[i] = sc[i] >= top ? sc[i] : -INFINITY;
            } else {
                // greedy search has no Temperature: the row as it stood before the division above
                for (int i = tid; i < V; i += kSampThreads) {
                    float v = bias_logit(lg[i], i, hits, bh);
                    if (seen[i]) v = v < 0.f ? v * rep_pen : v / rep_pen;
                    if (pr) v = proc_score(v, i, C.p.eos_token, ps, kill);
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
            if (C.scores_out) {
                // what survives the last warper keeps its temperature-scaled score, not renormalised; thread t stores its pair
                float* so = step_row(C.scores_out, C, b, step);
                const float o0 = k0 ? sc[i0v] : -INFINITY, o1 = k1 ? sc[i1v] : -INFINITY;
                if (i1v < V && (reinterpret_cast<uintptr_t>(so) & 7) == 0) {
                    *reinterpret_cast<float2*>(so + i0v) = make_float2(o0, o1);
                } else {
                    if (i0v < V) so[i0v] = o0;
                    if (i1v < V) so[i1v] = o1;
                }
            }
            const double w0 = k0 ? (double)expf(sc[i0v] - dmx) : 0.0, w1 = k1 ? (double)expf(sc[i1v] - dmx) : 0.0;
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
    if (Z && Z->renormalize && C.scores_out) renorm_row<kSampThreads>(step_row(C.scores_out, C, b, step), V, wscr);
}

// top_k = 1 (the configuration of every BASELINE workload that fixes top_k: TopK(1) leaves one candidate, so top-p and the draw are
// no-ops): RepetitionPenalty -> [processors] -> Temperature -> argmax with the arithmetic of k_sample, on 256 threads -- four waves meet at four
// barriers instead of sixteen at six, and nothing is sorted (7.7 -> ~5 us per decode step)
constexpr int kGreedyThreads = 256;
__global__ __launch_bounds__(kGreedyThreads) void k_sample_greedy(SampleCall cv, const SampleCall* cp) {
    __shared__ unsigned seen_w[kSortN / 4];          // one byte per vocabulary entry
    __shared__ float red_v[kGreedyThreads / 64];
    __shared__ int red_i[kGreedyThreads / 64];
    __shared__ int s_tok;
    __shared__ float s_top;
    __shared__ uint32_t kill[kProcWords];
    __shared__ BiasHits bh;
    __shared__ float rscr[32];
    unsigned char* seen = reinterpret_cast<unsigned char*>(seen_w);
    const SampleCall& C = cp ? *cp : cv;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = C.p.vocab;
    const int step = C.step_ptr ? *C.step_ptr : C.step;
    const float* lg = C.logits + (size_t)b * V;
    int32_t* ids = C.ids + (size_t)b * C.ids_stride;
    const int len = C.ids_len[b];
    const float rep_pen = C.rows ? C.rows[b].repetition_penalty : C.p.repetition_penalty;
    const float temp = C.rows ? C.rows[b].temperature : C.p.temperature;
    // this thread's logits are requested before the id pass (they do not depend on it)
    constexpr int PER = kSortN / kGreedyThreads;
    float v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int i = tid + u * kGreedyThreads; v[u] = i < V ? lg[i] : -INFINITY; }
    for (int i = tid; i < kSortN / 4; i += kGreedyThreads) seen_w[i] = 0u;
    const gvc_logits_processors* P = row_procs(C, b);
    // sequence bias / bad words / forced EOS of the call, as in k_sample
    const gvc_logits_bias* Z = C.bias;
    const bool force = Z && Z->force_eos_at > 0 && len - Z->prompt_len == Z->force_eos_at - 1;
    const bool pr = P || Z;
    ProcStep ps{false, 0.f, force};
    if (P) ps = proc_row_begin(*P, len, P->prompt_lens ? P->prompt_lens[b] : P->prompt_len, C.p.eos_token, kill, tid, force);
    else if (Z && tid < kProcWords) kill[tid] = 0u;
    if (Z && tid < 64) bias_match(*Z, ids, len, &bh, tid);
    __syncthreads();
    for (int i = tid; i < len; i += kGreedyThreads) {
        const int id = ids[i];
        if (id >= 0 && id < V) seen[id] = 1;
    }
    if (P && !force) proc_ngram(ids, len, P->no_repeat_ngram_size, V, kill, tid, kGreedyThreads);
    if (Z && !force) bias_bans(*Z, bh, V, kill, tid);
    const uint32_t hits = Z ? bh.hit & (uint32_t)((1ull << Z->n_bias) - 1ull) : 0u;
    __syncthreads();
    // per-step scores of a gvc_gpt_generate_scores call (SampleCall::scores_out): the loop below stores the row of a greedy search
    float* so = C.scores_out && !C.scores_warped ? step_row(C.scores_out, C, b, step) : nullptr;
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = tid + u * kGreedyThreads;
        if (i < V) {
            float x = bias_logit(v[u], i, hits, bh);
            if (seen[i]) x = x < 0.f ? x * rep_pen : x / rep_pen;
            if (pr) x = proc_score(x, i, C.p.eos_token, ps, kill);
            if (so) so[i] = x;                // greedy search: the processed row, no Temperature
            x = x / temp;
            if (x > bv || (x == bv && i < bi)) { bv = x; bi = i; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kGreedyThreads / 64; ++w)
            if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi)) { bv = red_v[w]; bi = red_i[w]; }
        int tok = bi < V ? bi : 0;            // (all scores NaN -- the step before produced garbage: any valid id, never an out-of-range one)
        s_top = bv;
        // finished rows emit the pad (= eos) token; a row whose ids buffer is full is finished too (see k_sample)
        if (C.finished[b] || len >= C.ids_stride) tok = C.p.eos_token;
        if (len < C.ids_stride) { ids[len] = tok; C.ids_len[b] = len + 1; }
        if (tok == C.p.eos_token) C.finished[b] = 1;
        C.tok_out[b] = tok;
        if (C.tokens_out) C.tokens_out[(size_t)b * C.tok_stride + C.i0 + step] = tok;
        if (C.run_flag) { *C.run_flag = 1; *const_cast<int32_t*>(C.step_ptr) = step + 1; }      // (every thread read `step` before the barriers above)
    }
    if (C.latents_out && C.latent_src) {
        const float* src = C.latent_src + (size_t)b * C.d;
        float* dst = C.latents_out + ((size_t)b * C.lat_stride + C.i0 + step) * C.d;
        for (int k = tid * 4; k < C.d; k += kGreedyThreads * 4) *reinterpret_cast<float4*>(dst + k) = *reinterpret_cast<const float4*>(src + k);
    }
    if (C.scores_out && C.scores_warped) {
        // sampling with top_k == 1: Temperature, then TopK(1) keeps the entries that equal the maximum (ties stay, as in HF)
        __syncthreads();
        const float top = s_top;
        float* sw = step_row(C.scores_out, C, b, step);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = tid + u * kGreedyThreads;
            if (i < V) {
                float x = bias_logit(v[u], i, hits, bh);
                if (seen[i]) x = x < 0.f ? x * rep_pen : x / rep_pen;
                if (pr) x = proc_score(x, i, C.p.eos_token, ps, kill);
                x = x / temp;
                sw[i] = x >= top ? x : -INFINITY;
            }
        }
    }
    if (C.logits_out) {
        const float* raw = C.logits_src ? C.logits_src + (size_t)b * V : lg;
        float* lo = step_row(C.logits_out, C, b, step);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = tid + u * kGreedyThreads;
            if (i < V) lo[i] = C.logits_src ? raw[i] : v[u];
        }
    }
    if (Z && Z->renormalize && C.scores_out) renorm_row<kGreedyThreads>(step_row(C.scores_out, C, b, step), V, rscr);
}
__global__ void k_stage_rows(gvc_row_sampling* dst, SampleRows src, int B) {
    if ((int)threadIdx.x < B) dst[threadIdx.x] = src.r[threadIdx.x];
}

__global__ void k_stage_proc(gvc_logits_processors* dst, gvc_logits_processors src) {
    if (threadIdx.x == 0) *dst = src;
}

// up to kProcSetChunk sets by value: set j goes to dst[at[j]]
struct ProcSetChunk {
    gvc_logits_processors s[kProcSetChunk];
    int32_t at[kProcSetChunk];
    int32_t n;
};
__global__ void k_stage_proc_sets(gvc_logits_processors* dst, ProcSetChunk c) {
    if ((int)threadIdx.x < c.n) dst[c.at[threadIdx.x]] = c.s[threadIdx.x];
}

__global__ void k_stage_set_index(int32_t* dst, SetIndex src, int B) {
    if ((int)threadIdx.x < B) dst[threadIdx.x] = src.k[threadIdx.x];
}

__global__ void k_stage_warps(gvc_logits_warpers* dst, WarpTable t) {
    if ((int)threadIdx.x < t.n) dst[threadIdx.x] = t.w[threadIdx.x];
}

__global__ void k_stage_bias(gvc_logits_bias* dst, gvc_logits_bias src) {
    int32_t* d = reinterpret_cast<int32_t*>(dst);
    const int32_t* w = reinterpret_cast<const int32_t*>(&src);
    for (int i = threadIdx.x; i < (int)(sizeof(gvc_logits_bias) / sizeof(int32_t)); i += blockDim.x) d[i] = w[i];
}

int check_bias(const gvc_logits_bias& Z, int vocab) {
    GVC_REQUIRE(vocab <= 32 * kProcWords, GVC_ERR_UNSUPPORTED, "bias: vocab %d > %d", vocab, 32 * kProcWords);
    GVC_REQUIRE(Z.n_bias >= 0 && Z.n_ban >= 0 && Z.n_bias <= GVC_BIAS_MAX_SEQS && Z.n_ban <= GVC_BIAS_MAX_SEQS &&
                    Z.n_bias + Z.n_ban <= GVC_BIAS_MAX_SEQS,
                GVC_ERR_ARG, "bias: %d sequence_bias + %d bad-word entries outside [0, %d]", Z.n_bias, Z.n_ban, GVC_BIAS_MAX_SEQS);
    GVC_REQUIRE(Z.force_eos_at >= 0 && Z.prompt_len >= 0 && (Z.renormalize == 0 || Z.renormalize == 1), GVC_ERR_ARG,
                "bias: force_eos_at %d / prompt_len %d negative, or renormalize %d not 0 / 1", Z.force_eos_at, Z.prompt_len, Z.renormalize);
    GVC_REQUIRE(Z.reserved[0] == 0 && Z.reserved[1] == 0 && Z.reserved[2] == 0, GVC_ERR_ARG, "bias: reserved fields must be 0");
    for (int e = 0; e < Z.n_bias + Z.n_ban; ++e) {
        GVC_REQUIRE(Z.len[e] >= 1 && Z.len[e] <= GVC_BIAS_MAX_LEN, GVC_ERR_ARG, "bias: entry %d has length %d outside [1, %d]", e, Z.len[e],
                    GVC_BIAS_MAX_LEN);
        for (int q = 0; q < Z.len[e]; ++q)
            GVC_REQUIRE(Z.ids[e][q] >= 0 && Z.ids[e][q] < vocab, GVC_ERR_ARG, "bias: entry %d holds id %d outside [0, %d)", e, Z.ids[e][q],
                        vocab);
        // finite or -inf (a ban): NaN and +inf would poison the row
        GVC_REQUIRE(e >= Z.n_bias || (Z.bias[e] == Z.bias[e] && Z.bias[e] <= 3.4028234664e38f), GVC_ERR_ARG,
                    "bias: entry %d has bias %g (finite or -inf)", e, (double)Z.bias[e]);
    }
    return GVC_OK;
}

int launch_stage_bias(gvc_logits_bias* dst, const gvc_logits_bias* bias, hipStream_t s) {
    hipLaunchKernelGGL(k_stage_bias, dim3(1), dim3(64), 0, s, dst, *bias);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int check_procs(const gvc_logits_processors& P, int vocab) {
    GVC_REQUIRE(vocab <= 32 * kProcWords, GVC_ERR_UNSUPPORTED, "processors: vocab %d > %d", vocab, 32 * kProcWords);
    GVC_REQUIRE(P.no_repeat_ngram_size >= 0 && P.no_repeat_ngram_size <= GVC_PROC_MAX_NGRAM, GVC_ERR_ARG,
                "processors: no_repeat_ngram_size %d outside [0, %d]", P.no_repeat_ngram_size, GVC_PROC_MAX_NGRAM);
    GVC_REQUIRE(P.min_length >= 0 && P.min_new_tokens >= 0 && P.prompt_len >= 0 && P.n_suppress >= 0 && P.n_begin_suppress >= 0,
                GVC_ERR_ARG, "processors: negative min_length %d / min_new_tokens %d / prompt_len %d", P.min_length, P.min_new_tokens,
                P.prompt_len);
    GVC_REQUIRE(P.decay_factor >= 0.f && P.min_p >= 0.f && P.min_p <= 1.f, GVC_ERR_ARG,
                "processors: decay factor %g (0 = off, else > 0), min_p %g outside [0, 1]", (double)P.decay_factor, (double)P.min_p);
    // ids past the vocabulary would never be scored: a set bit there is a caller error
    const int w = vocab >> 5, b = vocab & 31;
    for (int i = w; i < kProcWords; ++i) {
        const uint32_t m = i == w ? ~((1u << b) - 1u) : ~0u;
        GVC_REQUIRE(!(P.suppress[i] & m) && !(P.begin_suppress[i] & m), GVC_ERR_ARG, "processors: suppressed id >= vocab %d", vocab);
    }
    return GVC_OK;
}

int check_sample_rows(const gvc_row_sampling* rows, int B, int vocab, bool* all_greedy) {
    GVC_REQUIRE(rows && B >= 1 && B <= kMaxSampleRows, GVC_ERR_ARG, "sample rows: need 1..%d host rows, got %d", kMaxSampleRows, B);
    bool g = true;
    for (int b = 0; b < B; ++b) {
        const gvc_row_sampling& r = rows[b];
        GVC_REQUIRE(r.temperature > 0.f && r.top_k <= vocab && r.repetition_penalty > 0.f, GVC_ERR_ARG,
                    "sample rows: row %d has temperature %g, top_k %d (vocab %d), repetition_penalty %g", b, (double)r.temperature,
                    r.top_k, vocab, (double)r.repetition_penalty);
        g = g && r.top_k == 1;
    }
    *all_greedy = g;
    return GVC_OK;
}

int launch_stage_rows(gvc_row_sampling* dst, const gvc_row_sampling* rows, int B, hipStream_t s) {
    SampleRows sr;
    memset(&sr, 0, sizeof(sr));
    memcpy(sr.r, rows, (size_t)B * sizeof(gvc_row_sampling));
    hipLaunchKernelGGL(k_stage_rows, dim3(1), dim3(kMaxSampleRows), 0, s, dst, sr, B);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int check_proc_sets(const gvc_logits_processors* sets, int n_sets, const int32_t* set_of_row, int B, int vocab) {
    GVC_REQUIRE(sets && set_of_row && B >= 1 && B <= kMaxSampleRows, GVC_ERR_ARG, "processor sets: need host sets and 1..%d rows, got %d",
                kMaxSampleRows, B);
    GVC_REQUIRE(n_sets >= 1 && n_sets <= B, GVC_ERR_ARG, "processor sets: %d sets for %d rows (1..B)", n_sets, B);
    for (int b = 0; b < B; ++b)
        GVC_REQUIRE(set_of_row[b] >= -1 && set_of_row[b] < n_sets, GVC_ERR_ARG, "processor sets: row %d has set %d outside [-1, %d)", b,
                    set_of_row[b], n_sets);
    for (int k = 0; k < n_sets; ++k) {
        const int rc = check_procs(sets[k], vocab);
        if (rc) return rc;
    }
    return GVC_OK;
}

int launch_stage_proc_sets(gvc_logits_processors* dst, const gvc_logits_processors* sets, int n_sets, const int32_t* set_of_row, int B,
                           hipStream_t s) {
    bool used[kMaxSampleRows] = {};
    for (int b = 0; b < B; ++b)
        if (set_of_row[b] >= 0) used[set_of_row[b]] = true;
    ProcSetChunk c;
    memset(&c, 0, sizeof(c));
    for (int k = 0; k <= n_sets; ++k) {
        if (c.n == kProcSetChunk || (k == n_sets && c.n > 0)) {
            hipLaunchKernelGGL(k_stage_proc_sets, dim3(1), dim3(64), 0, s, dst, c);
            GVC_LAUNCH_CHECK();
            c.n = 0;
        }
        if (k < n_sets && used[k]) {
            c.s[c.n] = sets[k];
            c.at[c.n] = k;
            ++c.n;
        }
    }
    return GVC_OK;
}

int launch_stage_set_index(int32_t* dst, const int32_t* set_of_row, int B, hipStream_t s) {
    SetIndex si;
    memset(&si, 0, sizeof(si));
    memcpy(si.k, set_of_row, (size_t)B * sizeof(int32_t));
    hipLaunchKernelGGL(k_stage_set_index, dim3(1), dim3(kMaxSampleRows), 0, s, dst, si, B);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int check_warp_sets(const gvc_logits_processors* sets, const gvc_logits_warpers* warps, int n_sets, const int32_t* set_of_row, int B,
                    int vocab) {
    GVC_REQUIRE(B >= 1 && B <= kMaxSampleRows, GVC_ERR_ARG, "warpers: need 1..%d rows, got %d", kMaxSampleRows, B);
    GVC_REQUIRE(n_sets >= 1 && n_sets <= B, GVC_ERR_ARG, "warpers: %d sets for %d rows (1..B)", n_sets, B);
    if (set_of_row)
        for (int b = 0; b < B; ++b)
            GVC_REQUIRE(set_of_row[b] >= -1 && set_of_row[b] < n_sets, GVC_ERR_ARG, "warpers: row %d has set %d outside [-1, %d)", b,
                        set_of_row[b], n_sets);
    for (int k = 0; k < n_sets; ++k) {
        if (sets) {
            const int rc = check_procs(sets[k], vocab);
            if (rc) return rc;
        }
        if (warps) {
            const gvc_logits_warpers& w = warps[k];
            const bool ok = [](float x) { return x == 0.f || (x > 0.f && x < 1.f); }(w.typical_p) &&
                            [](float x) { return x == 0.f || (x > 0.f && x < 1.f); }(w.epsilon_cutoff) &&
                            [](float x) { return x == 0.f || (x > 0.f && x < 1.f); }(w.eta_cutoff);
            GVC_REQUIRE(ok && w.reserved == 0, GVC_ERR_ARG,
                        "warpers: set %d has typical_p %g, epsilon_cutoff %g, eta_cutoff %g (each 0 = off or in (0, 1)), reserved %d", k,
                        (double)w.typical_p, (double)w.epsilon_cutoff, (double)w.eta_cutoff, w.reserved);
        }
    }
    return GVC_OK;
}

static int launch_stage_proc(gvc_logits_processors* dst, const gvc_logits_processors* proc, hipStream_t s) {
    hipLaunchKernelGGL(k_stage_proc, dim3(1), dim3(64), 0, s, dst, *proc);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_stage_warps(gvc_logits_warpers* dst, const gvc_logits_warpers* warps, int n_sets, hipStream_t s) {
    WarpTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.w, warps, (size_t)n_sets * sizeof(gvc_logits_warpers));
    t.n = n_sets;
    hipLaunchKernelGGL(k_stage_warps, dim3(1), dim3(kMaxSampleRows), 0, s, dst, t);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_sample(const SampleCall& sc, hipStream_t s) {
    GVC_REQUIRE(sc.p.vocab > 0 && sc.p.vocab <= kSortN, GVC_ERR_UNSUPPORTED, "sample: vocab %d > %d", sc.p.vocab, kSortN);
    if (sample_greedy_ok(sc.p.top_k, sc.latents_out ? sc.d : 0)) hipLaunchKernelGGL(k_sample_greedy, dim3(sc.B), dim3(kGreedyThreads), 0, s, sc, (const SampleCall*)nullptr);
    else hipLaunchKernelGGL(k_sample, dim3(sc.B), dim3(kSampThreads), 0, s, sc, (const SampleCall*)nullptr);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_sample_indirect(const SampleCall* sc_dev, int B, bool greedy, hipStream_t s) {
    SampleCall dummy;
    memset(&dummy, 0, sizeof(dummy));
    if (greedy) hipLaunchKernelGGL(k_sample_greedy, dim3(B), dim3(kGreedyThreads), 0, s, dummy, sc_dev);
    else hipLaunchKernelGGL(k_sample, dim3(B), dim3(kSampThreads), 0, s, dummy, sc_dev);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// The one path behind gvc_sample_rows / _proc / _proc_sets / _warp / _bias.  Each entry checks its own arguments and passes what it has;
// everything null here is simply absent from the launch.  What is present needs device memory for the duration of this call only: one
// stream-ordered allocation, carved up, staged by value, and freed behind the sampler launch (no synchronisation; these context-free
// entries serve tests and callers that sample themselves, not the generation loop).  `greedy` is what check_sample_rows found when rows
// are given.  `proc` is the single by-value set of gvc_sample_proc; `sets` / `warps` are tables of n_sets indexed through set_of_row
// (null: every row uses entry 0).
struct SampleOptions {
    const gvc_row_sampling* rows = nullptr;
    bool greedy = false;
    const gvc_logits_processors* proc = nullptr;
    const gvc_logits_processors* sets = nullptr;
    const gvc_logits_warpers* warps = nullptr;
    int n_sets = 0;
    const int32_t* set_of_row = nullptr;
    const gvc_logits_bias* bias = nullptr;
    bool index = false;          // stage set_of_row and hand it to the kernel (the entries that take sets or warpers)
};

static int sample_once(const float* logits, int B, int32_t* ids, int ids_stride, int32_t* ids_len, int32_t* finished,
                       const gvc_sample_params& p, int step, int32_t* tok_out, const SampleOptions& o, hipStream_t s) {
    static const int32_t zeros[kMaxSampleRows] = {};
    const int32_t* sor = o.set_of_row ? o.set_of_row : zeros;
    const size_t bias_bytes = o.bias ? sizeof(gvc_logits_bias) : 0;
    const size_t proc_bytes = o.proc ? sizeof(gvc_logits_processors) : 0;
    const size_t set_bytes = o.sets ? (size_t)o.n_sets * sizeof(gvc_logits_processors) : 0;
    const size_t warp_bytes = o.warps ? (size_t)o.n_sets * sizeof(gvc_logits_warpers) : 0;
    const size_t row_bytes = o.rows ? (size_t)B * sizeof(gvc_row_sampling) : 0;
    const size_t sor_bytes = (size_t)B * sizeof(int32_t);          // (always there: the allocation is never empty)
    char* d = nullptr;
    GVC_CHECK_HIP(hipMallocAsync((void**)&d, bias_bytes + proc_bytes + set_bytes + warp_bytes + row_bytes + sor_bytes, s));
    char* at = d;
    auto carve = [&at](size_t bytes) { char* q = bytes ? at : nullptr; at += bytes; return q; };
    gvc_logits_bias* d_bias = reinterpret_cast<gvc_logits_bias*>(carve(bias_bytes));
    gvc_logits_processors* d_proc = reinterpret_cast<gvc_logits_processors*>(carve(proc_bytes));
    gvc_logits_processors* d_sets = reinterpret_cast<gvc_logits_processors*>(carve(set_bytes));
    gvc_logits_warpers* d_warps = reinterpret_cast<gvc_logits_warpers*>(carve(warp_bytes));
    gvc_row_sampling* d_rows = reinterpret_cast<gvc_row_sampling*>(carve(row_bytes));
    int32_t* d_sor = reinterpret_cast<int32_t*>(carve(sor_bytes));
    int rc = GVC_OK;
    if (o.bias) rc = launch_stage_bias(d_bias, o.bias, s);
    if (rc == GVC_OK && o.proc) rc = launch_stage_proc(d_proc, o.proc, s);
    if (rc == GVC_OK && o.sets) rc = launch_stage_proc_sets(d_sets, o.sets, o.n_sets, sor, B, s);
    if (rc == GVC_OK && o.warps) rc = launch_stage_warps(d_warps, o.warps, o.n_sets, s);
    if (rc == GVC_OK && o.index) rc = launch_stage_set_index(d_sor, sor, B, s);
    if (rc == GVC_OK && o.rows) rc = launch_stage_rows(d_rows, o.rows, B, s);
    if (rc == GVC_OK) {
        SampleCall sc;
        memset(&sc, 0, sizeof(sc));
        sc.logits = logits; sc.B = B; sc.ids = ids; sc.ids_stride = ids_stride; sc.ids_len = ids_len;
        sc.finished = finished; sc.p = p; sc.step = step; sc.tok_out = tok_out; sc.rows = d_rows; sc.proc = d_proc;
        sc.proc_sets = d_sets; sc.set_of_row = o.index ? d_sor : nullptr; sc.warps = d_warps; sc.bias = d_bias;
        if (o.rows) sc.p.top_k = o.greedy ? 1 : 0;          // (kernel choice only: every row's settings come from d_rows)
        rc = launch_sample(sc, s);
    }
    const hipError_t e = hipFreeAsync(d, s);
    if (rc) return rc;
    GVC_CHECK_HIP(e);
    return GVC_OK;
}

}  // namespace gvc

extern "C" int gvc_sample(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                          int32_t* finished, const gvc_sample_params* p, int32_t step, int32_t* tok_out,
                          gvc_stream s) {
    GVC_REQUIRE(logits && ids && ids_len && finished && p && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample: bad argument");
    gvc::SampleCall sc;
    memset(&sc, 0, sizeof(sc));
    sc.logits = logits; sc.B = B; sc.ids = ids; sc.ids_stride = ids_stride; sc.ids_len = ids_len;
    sc.finished = finished; sc.p = *p; sc.step = step; sc.tok_out = tok_out;
    return gvc::launch_sample(sc, (hipStream_t)s);
}

extern "C" int gvc_sample_rows(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                               int32_t* finished, const gvc_sample_params* common, const gvc_row_sampling* rows, int32_t step,
                               int32_t* tok_out, gvc_stream sv) {
    GVC_REQUIRE(logits && ids && ids_len && finished && common && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_rows: bad argument");
    gvc::SampleOptions o;
    o.rows = rows;
    const int rc = gvc::check_sample_rows(rows, B, common->vocab, &o.greedy);
    if (rc) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *common, step, tok_out, o, (hipStream_t)sv);
}

extern "C" int gvc_sample_proc(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                               const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* proc, int32_t step,
                               int32_t* tok_out, gvc_stream sv) {
    GVC_REQUIRE(logits && ids && ids_len && finished && p && proc && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_proc: bad argument");
    int rc = gvc::check_procs(*proc, p->vocab);
    if (rc) return rc;
    gvc::SampleOptions o;
    o.rows = rows; o.proc = proc;
    if (rows && (rc = gvc::check_sample_rows(rows, B, p->vocab, &o.greedy))) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *p, step, tok_out, o, (hipStream_t)sv);
}

extern "C" int gvc_sample_proc_sets(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                                    const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                                    int32_t n_sets, const int32_t* set_of_row, int32_t step, int32_t* tok_out, gvc_stream sv) {
    GVC_REQUIRE(logits && ids && ids_len && finished && p && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_proc_sets: bad argument");
    int rc = gvc::check_proc_sets(sets, n_sets, set_of_row, B, p->vocab);
    if (rc) return rc;
    gvc::SampleOptions o;
    o.rows = rows; o.sets = sets; o.n_sets = n_sets; o.set_of_row = set_of_row; o.index = true;
    if (rows && (rc = gvc::check_sample_rows(rows, B, p->vocab, &o.greedy))) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *p, step, tok_out, o, (hipStream_t)sv);
}

extern "C" int gvc_sample_warp(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                               const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                               const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, int32_t step, int32_t* tok_out,
                               gvc_stream sv) {
    GVC_REQUIRE(logits && ids && ids_len && finished && p && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_warp: bad argument");
    int rc = gvc::check_warp_sets(sets, warps, n_sets, set_of_row, B, p->vocab);
    if (rc) return rc;
    gvc::SampleOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row; o.index = true;
    if (rows && (rc = gvc::check_sample_rows(rows, B, p->vocab, &o.greedy))) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *p, step, tok_out, o, (hipStream_t)sv);
}

extern "C" int gvc_sample_bias(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                               const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                               const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias,
                               int32_t step, int32_t* tok_out, gvc_stream sv) {
    GVC_REQUIRE(logits && ids && ids_len && finished && p && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_bias: bad argument");
    const bool any = sets || warps;
    if (!bias && any) return gvc_sample_warp(logits, B, ids, ids_stride, ids_len, finished, p, rows, sets, warps, n_sets, set_of_row, step, tok_out, sv);
    GVC_REQUIRE(B <= gvc::kMaxSampleRows, GVC_ERR_ARG, "gvc_sample_bias: need 1..%d rows, got %d", gvc::kMaxSampleRows, B);
    int rc = GVC_OK;
    if (bias && (rc = gvc::check_bias(*bias, p->vocab))) return rc;
    if (any && (rc = gvc::check_warp_sets(sets, warps, n_sets, set_of_row, B, p->vocab))) return rc;
    gvc::SampleOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row; o.bias = bias; o.index = any;
    if (rows && (rc = gvc::check_sample_rows(rows, B, p->vocab, &o.greedy))) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *p, step, tok_out, o, (hipStream_t)sv);
}
