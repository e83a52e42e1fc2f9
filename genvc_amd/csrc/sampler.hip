#include "sample_body.h"

namespace gvc {

// the full sampler: one workgroup per row of the call (sample_body.h)
__global__ __launch_bounds__(kSampThreads) void k_sample(SampleCall cv, const SampleCall* cp) {
    const SampleCall& C = cp ? *cp : cv;
    const int b = blockIdx.x;
    const int step = C.step_ptr ? *C.step_ptr : C.step;
    sample_row<false>(C, b, C.logits + (size_t)b * C.p.vocab, C.ids + (size_t)b * C.ids_stride, C.ids_len[b], row_procs(C, b),
                      C.scores_out ? step_row(C.scores_out, C, b, step) : nullptr, step);
}

// top_k = 1 (the configuration of every BASELINE workload that fixes top_k: TopK(1) leaves one candidate, so top-p and the draw are
// no-ops): RepetitionPenalty -> [processors] -> Temperature -> argmax with the arithmetic of k_sample, on 256 threads -- four waves meet at four
// barriers instead of sixteen at six, and nothing is sorted (7.7 -> ~5 us per decode step)
constexpr int kGreedyThreads = 256;
__global__ __launch_bounds__(kGreedyThreads) void k_sample_greedy(SampleCall cv, const SampleCall* cp) {
    __shared__ unsigned seen_w[kSortN / 4];          // one byte per vocabulary entry
    __shared__ int cnt[kSortN];                      // counts of a gvc_logits_penalties row (touched only by such a row)
    __shared__ float red_v[kGreedyThreads / 64];
    __shared__ int red_i[kGreedyThreads / 64];
    __shared__ int s_tok;
    __shared__ float s_top;
    __shared__ uint32_t kill[kProcWords];
    __shared__ BiasHits bh;
    __shared__ float rscr[32];
    __shared__ uint32_t wmg[kProcWords];             // this step's green list of a gvc_logits_watermark row (touched only by such a row)
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
    // presence / frequency / windowed repetition penalties of the row, as in k_sample (off: `cnt` is neither cleared, added to nor read)
    const PenRow Q = pen_row(C, b, len);
    if (Q.on)
        for (int i = tid; i < kSortN; i += kGreedyThreads) cnt[i] = 0;
    const gvc_logits_processors* P = row_procs(C, b);
    // sequence bias / bad words / forced EOS of the call, as in k_sample
    const gvc_logits_bias* Z = C.bias;
    const bool force = Z && Z->force_eos_at > 0 && len - Z->prompt_len == Z->force_eos_at - 1;
    const bool pr = P || Z;
    ProcStep ps{false, 0.f, force};
    if (P) ps = proc_row_begin(*P, len, P->prompt_lens ? P->prompt_lens[b] : P->prompt_len, C.p.eos_token, kill, tid, force);
    else if (Z && tid < kProcWords) kill[tid] = 0u;
    if (Z && tid < 64) bias_match(*Z, ids, len, &bh, tid);
    // green-list watermark of the row, as in k_sample (off: `wmg` is neither written nor read): greedy search with the mark
    const WmRow M = wm_row(C, b, ids, len);
    if (M.on && tid < M.words) wmg[tid] = M.row[tid];
    __syncthreads();
    for (int i = tid; i < len; i += kGreedyThreads) {
        const int id = ids[i];
        if (id >= 0 && id < V) {
            seen[id] = 1;
            if (i >= Q.lo) atomicAdd(&cnt[id], 1);          // (Q.lo == len without penalties)
        }
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
            const int c = Q.on ? cnt[i] : 0;
            if (Q.windowed ? c > 0 : seen[i]) x = x < 0.f ? x * rep_pen : x / rep_pen;
            if (c > 0) x = pen_score(x, c, Q);
            if (pr) x = proc_score(x, i, C.p.eos_token, ps, kill);
            const bool green = M.on && wm_green(wmg, i);
            if (so) so[i] = green ? __fadd_rn(x, M.bias) : x;                // greedy search: the processed row, no Temperature
            x = x / temp;
            if (green) x = __fadd_rn(x, M.bias);
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
                const int c = Q.on ? cnt[i] : 0;
                if (Q.windowed ? c > 0 : seen[i]) x = x < 0.f ? x * rep_pen : x / rep_pen;
                if (c > 0) x = pen_score(x, c, Q);
                if (pr) x = proc_score(x, i, C.p.eos_token, ps, kill);
                x = x / temp;
                if (M.on && wm_green(wmg, i)) x = __fadd_rn(x, M.bias);
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

__global__ void k_stage_ras(gvc_logits_ras* dst, RasTable t) {
    if ((int)threadIdx.x < t.n) dst[threadIdx.x] = t.r[threadIdx.x];
}

__global__ void k_stage_pen(gvc_logits_penalties* dst, PenTable t) {
    if ((int)threadIdx.x < t.n) dst[threadIdx.x] = t.q[threadIdx.x];
}

__global__ void k_stage_wm(gvc_logits_watermark* dst, WmTable t) {
    if ((int)threadIdx.x < t.n) dst[threadIdx.x] = t.m[threadIdx.x];
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

int check_ras(const gvc_logits_ras* ras, int n_sets) {
    GVC_REQUIRE(ras && n_sets >= 1 && n_sets <= kMaxSampleRows, GVC_ERR_ARG, "ras: need 1..%d entries, got %d", kMaxSampleRows, n_sets);
    for (int k = 0; k < n_sets; ++k) {
        const gvc_logits_ras& r = ras[k];
        GVC_REQUIRE(r.window >= 0 && r.window <= GVC_RAS_MAX_WINDOW && (r.window == 0 || r.min_count >= 1) && r.prompt_len >= 0 &&
                        r.reserved == 0,
                    GVC_ERR_ARG, "ras: entry %d has window %d (0..%d), min_count %d (>= 1), prompt_len %d (>= 0), reserved %d (0)", k,
                    r.window, GVC_RAS_MAX_WINDOW, r.min_count, r.prompt_len, r.reserved);
    }
    return GVC_OK;
}

int launch_stage_ras(gvc_logits_ras* dst, const gvc_logits_ras* ras, int n_sets, hipStream_t s) {
    RasTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.r, ras, (size_t)n_sets * sizeof(gvc_logits_ras));
    t.n = n_sets;
    hipLaunchKernelGGL(k_stage_ras, dim3(1), dim3(kMaxSampleRows), 0, s, dst, t);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int check_pen(const gvc_logits_penalties* pen, int n_sets) {
    GVC_REQUIRE(pen && n_sets >= 1 && n_sets <= kMaxSampleRows, GVC_ERR_ARG, "penalties: need 1..%d entries, got %d", kMaxSampleRows,
                n_sets);
    for (int k = 0; k < n_sets; ++k) {
        const gvc_logits_penalties& q = pen[k];
        // (a NaN fails both comparisons of its pair)
        GVC_REQUIRE(q.presence >= -GVC_PENALTY_MAX && q.presence <= GVC_PENALTY_MAX && q.frequency >= -GVC_PENALTY_MAX &&
                        q.frequency <= GVC_PENALTY_MAX && q.window >= 0 && q.prompt_len >= 0,
                    GVC_ERR_ARG, "penalties: entry %d has presence %g, frequency %g (each in [-2, 2]), window %d (>= 0), prompt_len %d (>= 0)",
                    k, (double)q.presence, (double)q.frequency, q.window, q.prompt_len);
    }
    return GVC_OK;
}

int launch_stage_pen(gvc_logits_penalties* dst, const gvc_logits_penalties* pen, int n_sets, hipStream_t s) {
    PenTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.q, pen, (size_t)n_sets * sizeof(gvc_logits_penalties));
    t.n = n_sets;
    hipLaunchKernelGGL(k_stage_pen, dim3(1), dim3(kMaxSampleRows), 0, s, dst, t);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int check_wm(const gvc_logits_watermark* wm, int n_sets, int vocab) {
    GVC_REQUIRE(wm && n_sets >= 1 && n_sets <= kMaxSampleRows, GVC_ERR_ARG, "watermark: need 1..%d entries, got %d", kMaxSampleRows,
                n_sets);
    for (int k = 0; k < n_sets; ++k) {
        const gvc_logits_watermark& m = wm[k];
        if (!m.table) continue;          // (an off entry: its other fields are not read)
        GVC_REQUIRE(wm_entry_ok(m.bias, m.scheme, m.words, m.reserved, vocab, kProcWords), GVC_ERR_ARG,
                    "watermark: entry %d has bias %g (finite), scheme %d (0 / 1), words %d (ceil(%d / 32), at most %d), reserved %d (0)", k,
                    (double)m.bias, m.scheme, m.words, vocab, kProcWords, m.reserved);
    }
    return GVC_OK;
}

int launch_stage_wm(gvc_logits_watermark* dst, const gvc_logits_watermark* wm, int n_sets, hipStream_t s) {
    WmTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.m, wm, (size_t)n_sets * sizeof(gvc_logits_watermark));
    t.n = n_sets;
    hipLaunchKernelGGL(k_stage_wm, dim3(1), dim3(kMaxSampleRows), 0, s, dst, t);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_sample(const SampleCall& sc, hipStream_t s) {
    GVC_REQUIRE(sc.p.vocab > 0 && sc.p.vocab <= kSortN, GVC_ERR_UNSUPPORTED, "sample: vocab %d > %d", sc.p.vocab, kSortN);
    if (!sc.ras && sample_greedy_ok(sc.p.top_k, sc.latents_out ? sc.d : 0)) hipLaunchKernelGGL(k_sample_greedy, dim3(sc.B), dim3(kGreedyThreads), 0, s, sc, (const SampleCall*)nullptr);
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
    const gvc_logits_ras* ras = nullptr;          // n_sets RAS entries (gvc_sample_ras) ...
    int32_t* ras_redraws = nullptr;               // ... and the rows' redraw counters (device)
    const gvc_logits_penalties* pen = nullptr;    // n_sets penalty entries (gvc_sample_pen)
    const gvc_logits_watermark* wm = nullptr;     // n_sets watermark entries (gvc_sample_wm)
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
    const size_t ras_bytes = o.ras ? (size_t)o.n_sets * sizeof(gvc_logits_ras) : 0;
    const size_t pen_bytes = o.pen ? (size_t)o.n_sets * sizeof(gvc_logits_penalties) : 0;
    // (8-byte entries -- a pointer each -- behind 4-byte ones: the carve below rounds their offset up)
    const size_t wm_bytes = o.wm ? (size_t)o.n_sets * sizeof(gvc_logits_watermark) + 8 : 0;
    char* d = nullptr;
    GVC_CHECK_HIP(hipMallocAsync((void**)&d, bias_bytes + proc_bytes + set_bytes + warp_bytes + row_bytes + sor_bytes + ras_bytes + pen_bytes +
                                     wm_bytes,
                                 s));
    char* at = d;
    auto carve = [&at](size_t bytes) { char* q = bytes ? at : nullptr; at += bytes; return q; };
    gvc_logits_bias* d_bias = reinterpret_cast<gvc_logits_bias*>(carve(bias_bytes));
    gvc_logits_processors* d_proc = reinterpret_cast<gvc_logits_processors*>(carve(proc_bytes));
    gvc_logits_processors* d_sets = reinterpret_cast<gvc_logits_processors*>(carve(set_bytes));
    gvc_logits_warpers* d_warps = reinterpret_cast<gvc_logits_warpers*>(carve(warp_bytes));
    gvc_row_sampling* d_rows = reinterpret_cast<gvc_row_sampling*>(carve(row_bytes));
    int32_t* d_sor = reinterpret_cast<int32_t*>(carve(sor_bytes));
    gvc_logits_ras* d_ras = reinterpret_cast<gvc_logits_ras*>(carve(ras_bytes));
    gvc_logits_penalties* d_pen = reinterpret_cast<gvc_logits_penalties*>(carve(pen_bytes));
    gvc_logits_watermark* d_wm = nullptr;
    if (o.wm) d_wm = reinterpret_cast<gvc_logits_watermark*>(d + (((size_t)(carve(wm_bytes) - d) + 7) & ~(size_t)7));
    int rc = GVC_OK;
    if (o.bias) rc = launch_stage_bias(d_bias, o.bias, s);
    if (rc == GVC_OK && o.proc) rc = launch_stage_proc(d_proc, o.proc, s);
    if (rc == GVC_OK && o.sets) rc = launch_stage_proc_sets(d_sets, o.sets, o.n_sets, sor, B, s);
    if (rc == GVC_OK && o.warps) rc = launch_stage_warps(d_warps, o.warps, o.n_sets, s);
    if (rc == GVC_OK && o.index) rc = launch_stage_set_index(d_sor, sor, B, s);
    if (rc == GVC_OK && o.rows) rc = launch_stage_rows(d_rows, o.rows, B, s);
    if (rc == GVC_OK && o.ras) rc = launch_stage_ras(d_ras, o.ras, o.n_sets, s);
    if (rc == GVC_OK && o.pen) rc = launch_stage_pen(d_pen, o.pen, o.n_sets, s);
    if (rc == GVC_OK && o.wm) rc = launch_stage_wm(d_wm, o.wm, o.n_sets, s);
    if (rc == GVC_OK) {
        SampleCall sc;
        memset(&sc, 0, sizeof(sc));
        sc.logits = logits; sc.B = B; sc.ids = ids; sc.ids_stride = ids_stride; sc.ids_len = ids_len;
        sc.finished = finished; sc.p = p; sc.step = step; sc.tok_out = tok_out; sc.rows = d_rows; sc.proc = d_proc;
        sc.proc_sets = d_sets; sc.set_of_row = o.index ? d_sor : nullptr; sc.warps = d_warps; sc.bias = d_bias;
        sc.ras = d_ras; sc.ras_redraws = o.ras ? o.ras_redraws : nullptr;
        sc.pen = d_pen;
        sc.wm = d_wm;
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

extern "C" int gvc_sample_ras(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                              const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                              const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias,
                              const gvc_logits_ras* ras, int32_t* ras_redraws, int32_t step, int32_t* tok_out, gvc_stream sv) {
    if (!ras) return gvc_sample_bias(logits, B, ids, ids_stride, ids_len, finished, p, rows, sets, warps, n_sets, set_of_row, bias, step, tok_out, sv);
    GVC_REQUIRE(logits && ids && ids_len && finished && p && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_ras: bad argument");
    GVC_REQUIRE(B <= gvc::kMaxSampleRows, GVC_ERR_ARG, "gvc_sample_ras: need 1..%d rows, got %d", gvc::kMaxSampleRows, B);
    int rc = gvc::check_ras(ras, n_sets);
    if (rc) return rc;
    if (bias && (rc = gvc::check_bias(*bias, p->vocab))) return rc;
    // (check_warp_sets reads neither table when both are null: the bounds of n_sets and of the indices are what is left)
    if ((rc = gvc::check_warp_sets(sets, warps, n_sets, set_of_row, B, p->vocab))) return rc;
    gvc::SampleOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row; o.bias = bias; o.index = true;
    o.ras = ras; o.ras_redraws = ras_redraws;
    if (rows && (rc = gvc::check_sample_rows(rows, B, p->vocab, &o.greedy))) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *p, step, tok_out, o, (hipStream_t)sv);
}

extern "C" int gvc_sample_pen(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                              const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                              const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias,
                              const gvc_logits_ras* ras, int32_t* ras_redraws, const gvc_logits_penalties* pen, int32_t step,
                              int32_t* tok_out, gvc_stream sv) {
    if (!pen) return gvc_sample_ras(logits, B, ids, ids_stride, ids_len, finished, p, rows, sets, warps, n_sets, set_of_row, bias, ras, ras_redraws, step, tok_out, sv);
    GVC_REQUIRE(logits && ids && ids_len && finished && p && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_pen: bad argument");
    GVC_REQUIRE(B <= gvc::kMaxSampleRows, GVC_ERR_ARG, "gvc_sample_pen: need 1..%d rows, got %d", gvc::kMaxSampleRows, B);
    int rc = gvc::check_pen(pen, n_sets);
    if (rc) return rc;
    if (ras && (rc = gvc::check_ras(ras, n_sets))) return rc;
    if (bias && (rc = gvc::check_bias(*bias, p->vocab))) return rc;
    // (check_warp_sets reads neither table when both are null: the bounds of n_sets and of the indices are what is left)
    if ((rc = gvc::check_warp_sets(sets, warps, n_sets, set_of_row, B, p->vocab))) return rc;
    gvc::SampleOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row; o.bias = bias; o.index = true;
    o.ras = ras; o.ras_redraws = ras_redraws; o.pen = pen;
    if (rows && (rc = gvc::check_sample_rows(rows, B, p->vocab, &o.greedy))) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *p, step, tok_out, o, (hipStream_t)sv);
}

extern "C" int gvc_sample_wm(const float* logits, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                             const gvc_sample_params* p, const gvc_row_sampling* rows, const gvc_logits_processors* sets,
                             const gvc_logits_warpers* warps, int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias,
                             const gvc_logits_ras* ras, int32_t* ras_redraws, const gvc_logits_penalties* pen,
                             const gvc_logits_watermark* wm, int32_t step, int32_t* tok_out, gvc_stream sv) {
    if (!wm) return gvc_sample_pen(logits, B, ids, ids_stride, ids_len, finished, p, rows, sets, warps, n_sets, set_of_row, bias, ras, ras_redraws, pen, step, tok_out, sv);
    GVC_REQUIRE(logits && ids && ids_len && finished && p && tok_out && B >= 1, GVC_ERR_ARG, "gvc_sample_wm: bad argument");
    GVC_REQUIRE(B <= gvc::kMaxSampleRows, GVC_ERR_ARG, "gvc_sample_wm: need 1..%d rows, got %d", gvc::kMaxSampleRows, B);
    int rc = gvc::check_wm(wm, n_sets, p->vocab);
    if (rc) return rc;
    if (pen && (rc = gvc::check_pen(pen, n_sets))) return rc;
    if (ras && (rc = gvc::check_ras(ras, n_sets))) return rc;
    if (bias && (rc = gvc::check_bias(*bias, p->vocab))) return rc;
    // (check_warp_sets reads neither table when both are null: the bounds of n_sets and of the indices are what is left)
    if ((rc = gvc::check_warp_sets(sets, warps, n_sets, set_of_row, B, p->vocab))) return rc;
    gvc::SampleOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row; o.bias = bias; o.index = true;
    o.ras = ras; o.ras_redraws = ras_redraws; o.pen = pen; o.wm = wm;
    if (rows && (rc = gvc::check_sample_rows(rows, B, p->vocab, &o.greedy))) return rc;
    return gvc::sample_once(logits, B, ids, ids_stride, ids_len, finished, *p, step, tok_out, o, (hipStream_t)sv);
}
