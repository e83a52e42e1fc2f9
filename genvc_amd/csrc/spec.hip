// Assisted (speculative) greedy decoding: the kernels around a verification pass and the accept step (spec.h).  The accept step
// restates nothing of the sampler: the repetition penalty is k_sample_greedy's expression and the processors are logits_proc.h's
// device functions, run once per verified position at the length the row has there.
#include "spec.h"

#include "logits_proc.h"

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

__global__ void k_spec_round_begin(gvc_spec_state S, int k1, int32_t* step_ctr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *step_ctr = 0;
    if (b >= S.B) return;
    S.d_ids_len[b] = S.ids_len[b];
    S.d_finished[b] = S.finished[b];
    S.v_toks[(size_t)b * k1] = S.pending[b];
}

// the call's processors BY VALUE as a kernel argument (the caller's struct is free when the launch is enqueued)
struct SpecProc {
    int on;
    gvc_logits_processors P;
};

__global__ __launch_bounds__(kSpecThreads) void k_spec_accept(gvc_spec_state S, int k, int appended, const float* logits,
                                                              const float* latents, const int32_t* drafts, int draft_stride,
                                                              gvc_sample_params p, SpecProc pr) {
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
    const int kk = dr ? min(k, S.max_new - em0 - 1) : 0;          // drafts compared: HF's clamp of the draft length to the budget
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

int launch_spec_round_begin(const gvc_spec_state& st, int k1, int32_t* step_ctr, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_round_begin, dim3(cdiv(st.B, 64)), dim3(64), 0, s, st, k1, step_ctr);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_spec_accept(const gvc_spec_state& st, int k, int appended, const float* logits, const float* latents, const int32_t* drafts,
                       int draft_stride, const gvc_sample_params& p, const gvc_logits_processors* proc, hipStream_t s) {
    SpecProc pr;
    memset(&pr, 0, sizeof(pr));
    if (proc) { pr.on = 1; pr.P = *proc; }
    hipLaunchKernelGGL(k_spec_accept, dim3(st.B), dim3(kSpecThreads), 0, s, st, k, appended, logits, latents, drafts, draft_stride, p, pr);
    GVC_LAUNCH_CHECK();
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

}  // namespace gvc

using namespace gvc;

extern "C" int gvc_spec_accept(const gvc_spec_state* st, int32_t k, int32_t appended, const float* logits, const float* latents,
                               const int32_t* drafts, int32_t draft_stride, const gvc_sample_params* p, const gvc_logits_processors* proc,
                               gvc_stream sv) {
    int rc = check_spec_state(st, k, p, proc, false);
    if (rc) return rc;
    GVC_REQUIRE(logits && (k == 0 || (drafts && draft_stride >= k)) && (appended == 0 || appended == k + 1), GVC_ERR_ARG,
                "gvc_spec_accept: bad argument (k %d, appended %d, draft_stride %d)", k, appended, draft_stride);
    GVC_REQUIRE(!st->lats || latents, GVC_ERR_ARG, "gvc_spec_accept: a latent buffer without latent rows");
    return launch_spec_accept(*st, k, appended, logits, latents, k > 0 ? drafts : nullptr, draft_stride, *p, proc, (hipStream_t)sv);
}
