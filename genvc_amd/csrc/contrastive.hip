// Contrastive search: recall, hidden rows, similarity and select (contrastive.h; semantics in include/genvc_hip.h and DESIGN.md 4.10).
#include <limits.h>

#include <cmath>

#include "contrastive.h"

namespace gvc {

// One workgroup per item: the item's current logits row (the chosen candidate's of the last step, or the prefill's) -> repetition penalty
// over the ids row (each id once, on the raw score: s < 0 ? s * p : s / p) -> the processors (logits_proc.h bitmap) -> fp32 softmax ->
// the top-K probabilities, descending, ties by lower id (K rounds of a block argmax over <= 5 register-resident entries per thread).
// The candidate tokens go to the decode step's input (tok_buf[b*K + k]) and their probabilities to bf.prob; the final_norm latent of the
// row whose logits these are (the one that predicts step t's token, as gvc_gpt_generate's latents) goes to latents_out column t.
__global__ void __launch_bounds__(kCsThreads) k_cs_recall(const CsCall* call, CsBufs bf, const float* logits, const float* latent,
                                                          int32_t* tok_buf) {
    const gvc_contrastive_state& st = call->st;
    const int t = call->bc.step;
    const gvc_logits_processors* P = call->has_proc ? &call->proc : nullptr;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = st.K, V = st.vocab, L = st.n0 + t, eos = st.eos;
    const int32_t* row = st.ids + (size_t)b * st.ids_stride;
    const float* lg = logits + (size_t)(b * K + bf.sel[b]) * V;
    if (st.latents_out) {
        const float* src = latent + (size_t)(b * K + bf.sel[b]) * bf.d;
        float* dst = st.latents_out + ((size_t)b * st.max_new + t) * bf.d;
        for (int i = tid * 4; i < bf.d; i += kCsThreads * 4) *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
    }
    __shared__ uint32_t pen[GVC_PROC_VOCAB_WORDS];
    __shared__ uint32_t kill[kProcWords];
    __shared__ float red[4];
    __shared__ float wv_v[4];
    __shared__ int wv_i[4];
    __shared__ int sh_pick;
    if (tid < GVC_PROC_VOCAB_WORDS) pen[tid] = 0u;
    ProcStep ps{false, 0.f};
    if (P) ps = proc_row_begin(*P, L, st.n0, eos, kill, tid);
    __syncthreads();
    for (int p = tid; p < L; p += kCsThreads) {
        const int id = row[p];
        if (id >= 0 && id < V) atomicOr(&pen[id >> 5], 1u << (id & 31));
    }
    if (P) proc_ngram(row, L, P->no_repeat_ngram_size, V, kill, tid, kCsThreads);
    __syncthreads();
    const float rp = st.repetition_penalty;
    float v[kCsPer];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < kCsPer; ++i) {
        const int x = tid + i * kCsThreads;
        float s = -INFINITY;
        if (x < V) {
            s = lg[x];
            if (pen[x >> 5] & (1u << (x & 31))) s = s < 0.f ? s * rp : s / rp;
            if (P) s = proc_score(s, x, eos, ps, kill);
        }
        v[i] = s;
        m = fmaxf(m, s);
    }
    m = block4_max(m, red);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kCsPer; ++i)
        if (tid + i * kCsThreads < V) sum += expf(v[i] - m);
    sum = block4_sum(sum, red);
#pragma unroll
    for (int i = 0; i < kCsPer; ++i) v[i] = tid + i * kCsThreads < V ? expf(v[i] - m) / sum : -1.f;
    for (int k = 0; k < K; ++k) {
        float bv = -2.f;
        int bi = INT_MAX;
#pragma unroll
        for (int i = 0; i < kCsPer; ++i) {
            const int x = tid + i * kCsThreads;
            if (x < V && (v[i] > bv || (v[i] == bv && x < bi))) { bv = v[i]; bi = x; }
        }
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { wv_v[wv] = bv; wv_i[wv] = bi; }
        __syncthreads();
        if (tid == 0) {
            float cv = wv_v[0];
            int ci = wv_i[0];
            for (int w = 1; w < 4; ++w)
                if (wv_v[w] > cv || (wv_v[w] == cv && wv_i[w] < ci)) { cv = wv_v[w]; ci = wv_i[w]; }
            tok_buf[b * K + k] = ci;
            bf.prob[b * K + k] = cv;
            sh_pick = ci;
        }
        __syncthreads();
        const int pick = sh_pick;
#pragma unroll
        for (int i = 0; i < kCsPer; ++i)
            if (tid + i * kCsThreads == pick) v[i] = -2.f;
    }
}

// one wave per row: h = ln_f(x[row]) (k_ln_rows' arithmetic) and its L2 norm
__global__ void __launch_bounds__(256) k_cs_hidden(const float* x, float* h, float* h_norm, int rows, int d, const float* w,
                                                   const float* bias) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* in = x + (size_t)r * d;
    float* y = h + (size_t)r * d;
    const float inv_d = 1.0f / (float)d;
    float s = 0.f;
    for (int k = lane * 4; k < d; k += 256) {
        const float4 a = *reinterpret_cast<const float4*>(in + k);
        s += (a.x + a.y) + (a.z + a.w);
    }
    const float mean = wave_sum(s) * inv_d;
    float q = 0.f;
    for (int k = lane * 4; k < d; k += 256) {
        const float4 a = *reinterpret_cast<const float4*>(in + k);
        const float a0 = a.x - mean, a1 = a.y - mean, a2 = a.z - mean, a3 = a.w - mean;
        q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_d + 1e-5f);
    float n2 = 0.f;
    for (int k = lane * 4; k < d; k += 256) {
        float4 a = *reinterpret_cast<const float4*>(in + k);
        const float4 g = *reinterpret_cast<const float4*>(w + k);
        const float4 c = *reinterpret_cast<const float4*>(bias + k);
        a.x = (a.x - mean) * rstd * g.x + c.x; a.y = (a.y - mean) * rstd * g.y + c.y;
        a.z = (a.z - mean) * rstd * g.z + c.z; a.w = (a.w - mean) * rstd * g.w + c.w;
        *reinterpret_cast<float4*>(y + k) = a;
        n2 += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
    }
    n2 = wave_sum(n2);
    if (lane == 0) h_norm[r] = sqrtf(n2);
}

// one wave per row: ctx[item][j] = src row, ctx_norm = its L2 norm (the prompt's hidden rows at the start of a search)
__global__ void __launch_bounds__(256) k_cs_ctx0(const float* src, int n0, int B, CsBufs bf) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B * n0) return;
    const int b = r / n0, j = r - b * n0, d = bf.d;
    const float* in = src + (size_t)r * d;
    float* y = bf.ctx + ((size_t)b * bf.max_seq + j) * d;
    float n2 = 0.f;
    for (int k = lane * 4; k < d; k += 256) {
        const float4 a = *reinterpret_cast<const float4*>(in + k);
        *reinterpret_cast<float4*>(y + k) = a;
        n2 += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
    }
    n2 = wave_sum(n2);
    if (lane == 0) bf.ctx_norm[(size_t)b * bf.max_seq + j] = sqrtf(n2);
}

// grid (n_chunks, B): workgroup (ch, b) takes context rows [16 ch, 16 ch + 16) of item b, wave w rows 16 ch + 4 w .. + 3 held in
// registers; for each candidate k the four dots are wave sums and cos = dot / (|ctx_j| |h_k|); the chunk's max per candidate goes to
// bf.part.  Chunks past the item's n0 + t rows exit at once (the grid is fixed at capture: max_seq / 16 chunks).
__global__ void __launch_bounds__(256) k_cs_sim(const CsCall* call, CsBufs bf) {
    const gvc_contrastive_state& st = call->st;
    const int n_ctx = st.n0 + call->bc.step, K = st.K, d = bf.d, NI = d / 256;
    const int b = blockIdx.y, ch = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j0 = ch * kCsRows;
    if (j0 >= n_ctx) return;
    __shared__ float wmax[4][kCsMaxK];
    float4 cr[4][8];
    float cn[4];
    bool ok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + wv * 4 + r;
        ok[r] = j < n_ctx;
        const float* src = bf.ctx + ((size_t)b * bf.max_seq + (ok[r] ? j : 0)) * d;
        cn[r] = ok[r] ? bf.ctx_norm[(size_t)b * bf.max_seq + j] : 1.f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < NI) cr[r][i] = ok[r] ? *reinterpret_cast<const float4*>(src + i * 256 + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int k = 0; k < K; ++k) {
        const float* hk = bf.h + (size_t)(b * K + k) * d;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < NI) {
                const float4 hv = *reinterpret_cast<const float4*>(hk + i * 256 + lane * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] += dot4(cr[r][i], hv);
            }
        }
        const float hn = bf.h_norm[b * K + k];
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dt = wave_sum(acc[r]);
            if (ok[r]) mx = fmaxf(mx, dt / (cn[r] * hn));
        }
        if (lane == 0) wmax[wv][k] = mx;
    }
    __syncthreads();
    if ((int)threadIdx.x < K)
        bf.part[((size_t)b * bf.n_chunks + ch) * kCsMaxK + threadIdx.x] =
            fmaxf(fmaxf(wmax[0][threadIdx.x], wmax[1][threadIdx.x]), fmaxf(wmax[2][threadIdx.x], wmax[3][threadIdx.x]));
}

// One workgroup per item: pen_k = max over the chunks, score_k = (1 - a) p_k - a pen_k, k* = the first argmax (lane k of wave 0 owns
// candidate k).  Writes the token (eos once the item has finished) into the ids row and tokens_out, finished, appends the chosen
// candidate's hidden row and norm to the context, records k* (the next recall reads its logits and latent rows) and the K-1
// one-position copies slot(k*) -> the item's other slots for k_kv_copy_span.
__global__ void __launch_bounds__(256) k_cs_select(const CsCall* call, CsBufs bf, const int32_t* tok_buf,
                                                   const int32_t* slot_table, const int32_t* seq_len) {
    const gvc_contrastive_state& st = call->st;
    const int t = call->bc.step, n_ctx = st.n0 + t, K = st.K, d = bf.d;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    __shared__ int sh_k;
    if (tid < 64) {
        const int nch = (n_ctx + kCsRows - 1) / kCsRows;
        float pen = -INFINITY;
        if (lane < K)
            for (int ch = 0; ch < nch; ++ch) pen = fmaxf(pen, bf.part[((size_t)b * bf.n_chunks + ch) * kCsMaxK + lane]);
        const float a = st.penalty_alpha;
        float sc = lane < K ? (1.0f - a) * bf.prob[b * K + lane] - a * pen : -INFINITY;
        int ki = lane < K ? lane : INT_MAX;
        for (int o = 32; o >= 1; o >>= 1) {
            const float os = __shfl_xor(sc, o);
            const int oi = __shfl_xor(ki, o);
            if (os > sc || (os == sc && oi < ki)) { sc = os; ki = oi; }
        }
        if (lane == 0) sh_k = ki < K ? ki : 0;
    }
    __syncthreads();
    const int ks = sh_k, r = b * K + ks;
    float* crow = bf.ctx + ((size_t)b * bf.max_seq + n_ctx) * d;
    const float* hrow = bf.h + (size_t)r * d;
    for (int i = tid * 4; i < d; i += 256 * 4) *reinterpret_cast<float4*>(crow + i) = *reinterpret_cast<const float4*>(hrow + i);
    if (tid == 0) {
        const int tok = st.finished[b] ? st.eos : tok_buf[r];
        st.ids[(size_t)b * st.ids_stride + n_ctx] = tok;
        st.tokens_out[(size_t)b * st.max_new + t] = tok;
        if (tok == st.eos) st.finished[b] = 1;
        bf.sel[b] = ks;
        bf.ctx_norm[(size_t)b * bf.max_seq + n_ctx] = bf.h_norm[r];
        const int src = slot_table[r], lo = seq_len[src] - 1;
        int n = 0;
        for (int q = 0; q < K; ++q) {
            if (q == ks) continue;
            int32_t* c = bf.copies + ((size_t)b * K + n) * 3;
            c[0] = src; c[1] = slot_table[b * K + q]; c[2] = lo;
            ++n;
        }
        bf.n_copies[b] = n;
    }
}

// workgroup b < B: logits of slot b*K -> row b*K of the staging buffer; workgroup B: the call state, the slot table, sel = 0 and (i0 == 0)
// the fan-out copy lists (slot b*K -> the other slots, from position 0) with their lengths and mel positions
__global__ void k_cs_begin(CsCall* dst, gvc_contrastive_state st, CsBufs bf, int i0, const int32_t* slots_in, int32_t* slot_table,
                           float* logits, const float* slot_logits, float* latent, const float* slot_latent, int32_t* seq_len,
                           int32_t* mel_pos) {
    const int B = st.B, K = st.K, BK = B * K, b = blockIdx.x, tid = threadIdx.x;
    if (b == B) {
        if (tid == 0) {
            dst->st = st;
            dst->bc.st.copies = bf.copies;
            dst->bc.st.n_copies = bf.n_copies;
            dst->bc.step = i0 == 0 ? -1 : i0;        // (the fan-out's span-copy launch advances it to 0)
            dst->has_proc = 0;
        }
        if (tid < BK) slot_table[tid] = slots_in[tid];
        if (tid < B) {
            bf.sel[tid] = 0;
            if (i0 == 0) {
                const int src = slots_in[tid * K];
                for (int q = 1; q < K; ++q) {
                    const int ds = slots_in[tid * K + q];
                    int32_t* c = bf.copies + ((size_t)tid * K + q - 1) * 3;
                    c[0] = src; c[1] = ds; c[2] = 0;
                    seq_len[ds] = seq_len[src];
                    mel_pos[ds] = mel_pos[src];
                }
                bf.n_copies[tid] = K - 1;
            }
        }
        return;
    }
    const size_t sl = (size_t)slots_in[b * K];
    for (int i = tid; i < st.vocab; i += blockDim.x) logits[(size_t)b * K * st.vocab + i] = slot_logits[sl * st.vocab + i];
    for (int i = tid; i < bf.d; i += blockDim.x) latent[(size_t)b * K * bf.d + i] = slot_latent[sl * bf.d + i];
}

__global__ void k_cs_proc(CsCall* dst, gvc_logits_processors proc) {
    if (threadIdx.x == 0) { dst->proc = proc; dst->has_proc = 1; }
}

__global__ void k_cs_end(const int32_t* slots, const int32_t* sel, int K, const float* logits, float* slot_logits, int vocab,
                         const float* latent, float* slot_latent, int d) {
    const int b = blockIdx.x;
    const size_t sl = (size_t)slots[b * K];
    const float* src = logits + (size_t)(b * K + sel[b]) * vocab;
    for (int i = threadIdx.x; i < vocab; i += blockDim.x) slot_logits[sl * vocab + i] = src[i];
    const float* lsrc = latent + (size_t)(b * K + sel[b]) * d;
    for (int i = threadIdx.x; i < d; i += blockDim.x) slot_latent[sl * d + i] = lsrc[i];
}

int cs_check_shape(int B, int K, int vocab, int d) {
    GVC_REQUIRE(B >= 1 && K >= 2 && K <= kCsMaxK && B * K <= 64 && vocab >= 2 && vocab <= GVC_PROC_VOCAB_WORDS * 32, GVC_ERR_ARG,
                "contrastive: B=%d K=%d vocab=%d outside the supported range (2 <= K <= %d, B*K <= 64, vocab <= %d)", B, K, vocab, kCsMaxK,
                GVC_PROC_VOCAB_WORDS * 32);
    GVC_REQUIRE(d % 256 == 0 && d <= 2048, GVC_ERR_UNSUPPORTED, "contrastive: d_model %d (a multiple of 256 up to 2048)", d);
    return GVC_OK;
}

int cs_check(const gvc_contrastive_state& st, int d) {
    int rc = cs_check_shape(st.B, st.K, st.vocab, d);
    if (rc) return rc;
    GVC_REQUIRE(st.eos >= 0 && st.eos < st.vocab && st.n0 >= 1 && st.max_new >= 1 && st.ids_stride >= st.n0 + st.max_new &&
                    st.repetition_penalty > 0.f && st.penalty_alpha > 0.f && std::isfinite(st.penalty_alpha),
                GVC_ERR_ARG, "contrastive: bad state (n0 %d, max_new %d, ids_stride %d, penalty_alpha %g, repetition_penalty %g)", st.n0,
                st.max_new, st.ids_stride, (double)st.penalty_alpha, (double)st.repetition_penalty);
    GVC_REQUIRE(st.ids && st.finished && st.tokens_out && st.hidden0, GVC_ERR_ARG, "contrastive: null state array");
    return GVC_OK;
}

int cs_alloc(CsBufs* bf, int max_items, int max_slots, int max_seq, int d) {
    memset(bf, 0, sizeof(*bf));
    bf->max_items = max_items; bf->max_seq = max_seq; bf->d = d;
    bf->n_chunks = (max_seq + kCsRows - 1) / kCsRows;
    // one allocation, every sub-buffer starting on a 16-byte boundary (rows are read and written as float4): sizes in 4-byte
    // elements, each rounded up to a multiple of 4
    const size_t sz[9] = {(size_t)max_items * max_seq * d, (size_t)max_items * max_seq, (size_t)max_slots * d, (size_t)max_slots,
                          (size_t)max_slots, (size_t)max_items * bf->n_chunks * kCsMaxK, (size_t)max_items,
                          (size_t)max_items * kCsMaxK * 3, (size_t)max_items};
    size_t off[9], total = 0;
    for (int i = 0; i < 9; ++i) { off[i] = total; total += (sz[i] + 3) & ~(size_t)3; }
    float* p = nullptr;
    GVC_CHECK_HIP(hipMalloc((void**)&p, total * sizeof(float)));
    bf->ctx = p + off[0];
    bf->ctx_norm = p + off[1];
    bf->h = p + off[2];
    bf->h_norm = p + off[3];
    bf->prob = p + off[4];
    bf->part = p + off[5];
    bf->sel = reinterpret_cast<int32_t*>(p + off[6]);
    bf->copies = reinterpret_cast<int32_t*>(p + off[7]);
    bf->n_copies = reinterpret_cast<int32_t*>(p + off[8]);
    return GVC_OK;
}

void cs_free(CsBufs* bf) {
    if (bf->ctx) (void)hipFree(bf->ctx);
    memset(bf, 0, sizeof(*bf));
}

int launch_cs_begin(CsCall* call, const CsBufs& bf, const gvc_contrastive_state& st, const gvc_logits_processors* proc, int i0,
                    const int32_t* slots_in, int32_t* slot_table, float* logits, const float* slot_logits, float* latent,
                    const float* slot_latent, int32_t* seq_len, int32_t* mel_pos, void* kv, int n_layer, int n_head, int max_seq, int hd,
                    int max_slots, int esz, hipStream_t s) {
    hipLaunchKernelGGL(k_cs_begin, dim3(st.B + 1), dim3(256), 0, s, call, st, bf, i0, slots_in, slot_table, logits, slot_logits, latent,
                       slot_latent, seq_len, mel_pos);
    GVC_LAUNCH_CHECK();
    if (proc) {
        // (stream-ordered behind the begin that cleared has_proc; the struct travels as a kernel argument)
        hipLaunchKernelGGL(k_cs_proc, dim3(1), dim3(64), 0, s, call, *proc);
        GVC_LAUNCH_CHECK();
    }
    if (i0 == 0) {
        hipLaunchKernelGGL(k_cs_ctx0, dim3(cdiv(st.B * st.n0, 4)), dim3(256), 0, s, st.hidden0, st.n0, st.B, bf);
        GVC_LAUNCH_CHECK();
        return launch_kv_copy_span(&call->bc, st.B, st.K, kv, n_layer, n_head, max_seq, hd, max_slots, esz, seq_len, s);
    }
    return GVC_OK;
}

int launch_cs_recall(const CsCall* call, const CsBufs& bf, int B, const float* logits, const float* latent, int32_t* tok_buf,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_cs_recall, dim3(B), dim3(kCsThreads), 0, s, call, bf, logits, latent, tok_buf);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_cs_hidden(const float* x, const CsBufs& bf, int rows, const float* w, const float* b, hipStream_t s) {
    hipLaunchKernelGGL(k_cs_hidden, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, bf.h, bf.h_norm, rows, bf.d, w, b);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_cs_sim(const CsCall* call, const CsBufs& bf, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_cs_sim, dim3(bf.n_chunks, B), dim3(256), 0, s, call, bf);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_cs_select(const CsCall* call, const CsBufs& bf, int B, const int32_t* tok_buf, const int32_t* slot_table, const int32_t* seq_len,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_cs_select, dim3(B), dim3(256), 0, s, call, bf, tok_buf, slot_table, seq_len);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_cs_end(const CsBufs& bf, const int32_t* slots, int B, int K, const float* logits, float* slot_logits, int vocab,
                  const float* latent, float* slot_latent, hipStream_t s) {
    hipLaunchKernelGGL(k_cs_end, dim3(B), dim3(256), 0, s, slots, bf.sel, K, logits, slot_logits, vocab, latent, slot_latent, bf.d);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc
