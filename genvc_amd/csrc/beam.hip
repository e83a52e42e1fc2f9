// Deterministic beam search: select step and KV span copies (beam.h; semantics in include/genvc_hip.h and DESIGN.md 4.7).
#include "beam.h"

namespace gvc {

__device__ __forceinline__ uint32_t f2key(float v) {         // monotone: a larger float has a larger key
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per item.  Candidate e = k * V + x (beam k, token x) of the item lives in thread e % 512's registers, slot e / 512.
// The top-2K is a 4-pass 8-bit radix select on the keys (histograms in LDS), then a one-wave rank sort of the <= 32 survivors
// (ties by lower flat index); one lane walks them.
// GRP (k_group_beam_select): the item's K rows are G groups of S = K / G, selected one after the other inside the launch with K
// replaced by S: candidate e = i * V + x is row g * S + i of group g, the top is 2S, the kept set, its count / worst and the done flag
// are the (item, group)'s, parents and slot moves stay inside the group.  Group g > 0 first subtracts lambda * freq[x], freq (LDS) counting
// the tokens groups < g of the item have just chosen (a done group: eos S times).  !GRP is one group of K: the plain search.
template <bool GRP>
__device__ __forceinline__ void beam_select_body(const gvc_beam_state& st, const gvc_beam_groups* grp, const gvc_logits_processors* P,
                                                 const int t, const float* logits, int32_t* slots, int32_t* seq_len, int32_t* mel_pos,
                                                 int32_t* tok_buf) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = st.K, V = st.vocab, eos = st.eos;
    const int G = GRP ? grp->G : 1, S = GRP ? K / G : K;
    const int M = 2 * S;
    const int BK = st.B * K, W = st.ids_stride, L = st.n0 + t;
    const int32_t* ids_in = st.ids + (size_t)(t & 1) * BK * W;
    int32_t* ids_out = st.ids + (size_t)((t + 1) & 1) * BK * W;

    __shared__ float lse[kBeamMaxK], run[kBeamMaxK];
    __shared__ uint32_t pen[kBeamMaxK * 33];                    // repetition-penalty bitmaps, V <= 1056
    __shared__ int hist[256];
    __shared__ uint32_t sh_prefix;
    __shared__ int sh_need, cnt_gt, cnt_eq;
    __shared__ float cv[32], sv[32];
    __shared__ int ci[32], si[32];
    __shared__ int nx_tok[kBeamMaxK], nx_par[kBeamMaxK], new_slot[kBeamMaxK], pend[kBeamMaxK];
    __shared__ float nx_sc[kBeamMaxK];
    __shared__ int sh_done;
    __shared__ int first[kBeamMaxK], free_s[kBeamMaxK], old_slot[kBeamMaxK];   // thread 0's, for the slot permutation
    __shared__ uint32_t kill[kBeamMaxK * kProcWords];           // processor bans per beam (logits_proc.h)
    __shared__ int freq[GRP ? 33 * 32 : 1];                     // GRP: tokens the earlier groups of the item chose at this step
    __shared__ int gdone[GRP ? kBeamMaxK : 1];                  // GRP: done flag of each group at entry

    ProcStep ps{false, 0.f};
    if (tid == 0) sh_done = st.done[b];
    for (int i = tid; i < K * 33; i += kBeamThreads) pen[i] = 0u;
    if (GRP) {
        for (int i = tid; i < 33 * 32; i += kBeamThreads) freq[i] = 0;
        if (tid < G) gdone[tid] = grp->done[b * G + tid];
    }
    __syncthreads();
    const int was_done = sh_done;
    if (!was_done) {
        // log-sum-exp per beam row: beam k on wave k % 8, accurate expf / logf
        for (int k = wv; k < K; k += kBeamThreads / 64) {
            const float* row = logits + (size_t)(b * K + k) * V;
            float m = -INFINITY;
            for (int x = lane; x < V; x += 64) m = fmaxf(m, row[x]);
            m = wave_max(m);
            float sum = 0.f;
            for (int x = lane; x < V; x += 64) sum += expf(row[x] - m);
            sum = wave_sum(sum);
            if (lane == 0) { lse[k] = m; run[k] = logf(sum); }
        }
        for (int k = 0; k < K; ++k) {
            const int32_t* r = ids_in + (size_t)(b * K + k) * W;
            for (int p = tid; p < L; p += kBeamThreads) {
                const int id = r[p];
                if (id >= 0 && id < V) atomicOr(&pen[k * 33 + (id >> 5)], 1u << (id & 31));
            }
        }
        if (P) {
            // every beam row has length L = n0 + t and prompt n0: the scalar bans are the item's, the n-gram bans each beam's own
            for (int k = 0; k < K; ++k) ps = proc_row_begin(*P, L, st.n0, eos, kill + k * kProcWords, tid);
            __syncthreads();
            for (int k = 0; k < K; ++k)
                proc_ngram(ids_in + (size_t)(b * K + k) * W, L, P->no_repeat_ngram_size, V, kill + k * kProcWords, tid, kBeamThreads);
        }
        __syncthreads();
    }
    const float rp = st.repetition_penalty;
    const float lam = GRP ? grp->diversity_penalty : 0.f;
    uint32_t key[kBeamPer];
    float val[kBeamPer];
    if (!was_done) {
        int nc = 0, all_done = 1;                                // (thread 0's: copies of the item so far, every group done)
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
            const int r0 = g * S;                                // first row of the group within the item
            if (GRP && gdone[g]) {
                // a done group keeps its beams and counts as S choices of eos
                if (tid < S) {
                    nx_tok[r0 + tid] = eos; nx_par[r0 + tid] = r0 + tid; pend[r0 + tid] = -1;
                    st.tokens[b * K + r0 + tid] = eos;
                    if (tok_buf) tok_buf[b * K + r0 + tid] = eos;
                    st.parents[b * K + r0 + tid] = r0 + tid;
                }
                if (tid == 0) freq[eos] += S;
                __syncthreads();
                continue;
            }
            // (GRP: V made opaque per group, or the 33 divisions and bounds below are hoisted out of the group loop into registers
            // that then live across it -- 256 VGPRs and spills to scratch)
            int Vg = V;
            if (GRP) asm volatile("" : "+v"(Vg));
            const int Ng = S * Vg;
#pragma unroll
            for (int i = 0; i < kBeamPer; ++i) {
                const int e = tid + i * kBeamThreads;
                float v = -INFINITY;
                if (e < Ng) {
                    const int k = r0 + e / Vg, x = e - (k - r0) * Vg;
                    v = (logits[(size_t)(b * K + k) * V + x] - lse[k]) - run[k];
                    if (GRP && g > 0) v -= lam * (float)freq[x];
                    if (pen[k * 33 + (x >> 5)] & (1u << (x & 31))) v = v < 0.f ? v * rp : v / rp;
                    if (P) v = proc_score(v, x, eos, ps, kill + k * kProcWords);
                    v += st.scores[b * K + k];
                }
                val[i] = v;
                key[i] = e < Ng ? f2key(v) : 0u;
            }
            // radix select of the M-th largest key
            uint32_t prefix = 0u, mask = 0u;
            int need = M;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                if (tid < 256) hist[tid] = 0;
                __syncthreads();
#pragma unroll
                for (int i = 0; i < kBeamPer; ++i)
                    if (tid + i * kBeamThreads < Ng && (key[i] & mask) == prefix) atomicAdd(&hist[(key[i] >> shift) & 255], 1);
                __syncthreads();
                if (wv == 0) {
                    // lane l owns digits 255 - 4l .. 252 - 4l; inclusive scan from the top digit down
                    int h[4], own = 0;
                    for (int j = 0; j < 4; ++j) { h[j] = hist[255 - 4 * lane - j]; own += h[j]; }
                    int incl = own;
                    for (int o = 1; o < 64; o <<= 1) {
                        const int y = __shfl_up(incl, o);
                        if (lane >= o) incl += y;
                    }
                    const int excl = incl - own;
                    if (excl < need && incl >= need) {
                        int c = excl;
                        for (int j = 0; j < 4; ++j) {
                            if (c + h[j] >= need) {
                                sh_prefix = prefix | ((uint32_t)(255 - 4 * lane - j) << shift);
                                sh_need = need - c;
                                break;
                            }
                            c += h[j];
                        }
                    }
                }
                __syncthreads();
                prefix = sh_prefix;
                need = sh_need;
                mask |= 255u << shift;
                __syncthreads();
            }
            // survivors: every key above the threshold, and `need` keys equal to it
            if (tid == 0) { cnt_gt = 0; cnt_eq = 0; }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kBeamPer; ++i) {
                const int e = tid + i * kBeamThreads;
                if (e >= Ng) continue;
                if (key[i] > prefix) {
                    const int pos = atomicAdd(&cnt_gt, 1);
                    cv[pos] = val[i]; ci[pos] = e;
                } else if (key[i] == prefix) {
                    const int pos = atomicAdd(&cnt_eq, 1);
                    if (pos < need) { cv[M - need + pos] = val[i]; ci[M - need + pos] = e; }
                }
            }
            __syncthreads();
            if (wv == 0 && lane < M) {
                const float v = cv[lane];
                const int e = ci[lane];
                int r = 0;
                for (int j = 0; j < M; ++j) {
                    const float w = cv[j];
                    r += (w > v) || (w == v && ci[j] < e);
                }
                sv[r] = v; si[r] = e;
            }
            __syncthreads();
            // the scorer walk (BeamSearchScorer.process / BeamHypotheses.add, is_done by the early_stopping mode)
            if (tid == 0) {
                const int lmode = st.length_mode & 0xff, early = (st.length_mode >> 8) & 0xff;
                const int len = lmode == 0 ? st.n0 + t : t + 1;
                const float denom = powf((float)len, st.length_penalty);
                float* hs = st.hyp_score + b * K + r0;
                int32_t* hl = st.hyp_len + b * K + r0;
                int32_t* cnt_p = GRP ? grp->hyp_count + b * G + g : st.hyp_count + b;
                float* worst_p = GRP ? grp->hyp_worst + b * G + g : st.hyp_worst + b;
                int cnt = *cnt_p;
                float worst = *worst_p;
                for (int k = 0; k < S; ++k) pend[r0 + k] = -1;
                int j = 0;
                for (int r = 0; r < M && j < S; ++r) {
                    const int e = si[r], p = e / V, x = e - p * V;
                    if (x == eos) {
                        if (r >= S) continue;
                        const float sc = sv[r] / denom;
                        int dst = -1;
                        if (cnt < S) {
                            dst = cnt++;
                            worst = fminf(sc, worst);
                        } else if (sc > worst) {
                            dst = 0;
                            for (int q = 1; q < S; ++q) if (hs[q] < hs[dst]) dst = q;
                        }
                        if (dst >= 0) {
                            hs[dst] = sc; hl[dst] = t; pend[r0 + dst] = r0 + p;
                            if (cnt == S && dst >= 0) {
                                float w = hs[0];
                                for (int q = 1; q < S; ++q) w = fminf(w, hs[q]);
                                worst = w;
                            }
                        }
                    } else {
                        nx_tok[r0 + j] = x; nx_par[r0 + j] = r0 + p; nx_sc[r0 + j] = sv[r];
                        ++j;
                    }
                }
                int done = 0;
                if (cnt == S) {
                    const float best = lmode == 0 ? sv[0] : nx_sc[r0];
                    if (early == 1) done = 1;
                    else if (early == 2 && st.length_penalty > 0.f)
                        done = worst >= best / powf((float)(lmode == 0 ? st.n0 + st.max_new : st.max_new), st.length_penalty);
                    else done = worst >= best / denom;
                }
                *cnt_p = cnt;
                *worst_p = worst;
                if (GRP) {
                    grp->done[b * G + g] = done;
                    if (G == 1) { st.hyp_count[b] = cnt; st.hyp_worst[b] = worst; }
                }
                all_done &= done;
                // slot permutation: a parent's slot goes to its first child; further children take the slots of childless parents
                int nf = 0;
                for (int k = 0; k < S; ++k) { first[k] = -1; old_slot[k] = slots[b * K + r0 + k]; }
                for (int q = 0; q < S; ++q) if (first[nx_par[r0 + q] - r0] < 0) first[nx_par[r0 + q] - r0] = q;
                for (int k = 0; k < S; ++k) if (first[k] < 0) free_s[nf++] = old_slot[k];
                int taken = 0;
                // (groups start from a fanned-out prefix, gvc_gpt_group_beam_generate: their copies never reach below n0)
                const int lo = t == 0 && G == 1 ? 0 : st.n0;
                for (int q = 0; q < S; ++q) {
                    const int p = nx_par[r0 + q] - r0;
                    if (first[p] == q) {
                        new_slot[r0 + q] = old_slot[p];
                    } else {
                        const int dst = free_s[taken++];
                        new_slot[r0 + q] = dst;
                        int32_t* c = st.copies + ((size_t)b * K + nc) * 3;
                        c[0] = old_slot[p]; c[1] = dst; c[2] = lo;
                        ++nc;
                        if (seq_len) { seq_len[dst] = seq_len[old_slot[p]]; mel_pos[dst] = mel_pos[old_slot[p]]; }
                    }
                }
                for (int q = r0; q < r0 + S; ++q) {
                    slots[b * K + q] = new_slot[q];
                    st.tokens[b * K + q] = nx_tok[q];
                    if (tok_buf) tok_buf[b * K + q] = nx_tok[q];
                    st.parents[b * K + q] = nx_par[q];
                    st.scores[b * K + q] = nx_sc[q];
                    if (GRP) freq[nx_tok[q]] += 1;
                }
            }
            if (GRP) __syncthreads();                            // freq, and the select's LDS, before the next group
        }
        if (tid == 0) {
            st.done[b] = all_done;
            st.n_copies[b] = nc;
        }
    } else if (tid < K) {
        nx_tok[tid] = eos; nx_par[tid] = tid; pend[tid] = -1;
        st.tokens[b * K + tid] = eos;
        if (tok_buf) tok_buf[b * K + tid] = eos;
        st.parents[b * K + tid] = tid;
        if (tid == 0) st.n_copies[b] = 0;
    }
    __syncthreads();
    // hypothesis tokens (the parent's generated tokens, read before any ids row is rewritten) and the ids gather into the other buffer
    for (int k = 0; k < K; ++k) {
        const int p = pend[k];
        if (p < 0) continue;
        const int32_t* src = ids_in + (size_t)(b * K + p) * W + st.n0;
        int32_t* dst = st.hyp_tok + ((size_t)b * K + k) * st.max_new;
        for (int i = tid; i < t; i += kBeamThreads) dst[i] = src[i];
    }
    for (int q = 0; q < K; ++q) {
        const int32_t* src = ids_in + (size_t)(b * K + nx_par[q]) * W;
        int32_t* dst = ids_out + (size_t)(b * K + q) * W;
        for (int i = tid; i < L; i += kBeamThreads) dst[i] = src[i];
        if (tid == 0 && L < W) dst[L] = nx_tok[q];
    }
}

__global__ void __launch_bounds__(kBeamThreads) k_beam_select(gvc_beam_state st_arg, const gvc_logits_processors* proc_arg,
                                                              const BeamCall* call, const float* logits, int32_t* slots, int t_arg,
                                                              int32_t* seq_len, int32_t* mel_pos, int32_t* tok_buf) {
    const gvc_beam_state& st = call ? call->st : st_arg;
    const gvc_logits_processors* P = call ? (call->has_proc ? &call->proc : nullptr) : proc_arg;
    beam_select_body<false>(st, nullptr, P, call ? call->step : t_arg, logits, slots, seq_len, mel_pos, tok_buf);
}

// the group (diverse) select step: k_beam_select's arguments plus the groups (by value, or call->grp on graph replay)
__global__ void __launch_bounds__(kBeamThreads) k_group_beam_select(gvc_beam_state st_arg, gvc_beam_groups grp_arg,
                                                                    const gvc_logits_processors* proc_arg, const BeamCall* call,
                                                                    const float* logits, int32_t* slots, int t_arg, int32_t* seq_len,
                                                                    int32_t* mel_pos, int32_t* tok_buf) {
    const gvc_beam_state& st = call ? call->st : st_arg;
    const gvc_beam_groups* grp = call ? &call->grp : &grp_arg;
    const gvc_logits_processors* P = call ? (call->has_proc ? &call->proc : nullptr) : proc_arg;
    beam_select_body<true>(st, grp, P, call ? call->step : t_arg, logits, slots, seq_len, mel_pos, tok_buf);
}

// one block column per possible copy (blockIdx.y = item * (K-1) + copy), blockIdx.x strides over the (layer, k|v, head) runs; each
// run copies positions [lo, cur) of one head, contiguous, in 16-byte vectors
__global__ void __launch_bounds__(256) k_kv_copy_span(BeamCall* call, int K, char* kv, int runs, int n_head, size_t lw_bytes,
                                                      size_t slot_bytes, size_t head_bytes, int row_bytes, const int32_t* seq_len) {
    const int b = blockIdx.y / (K - 1), q = blockIdx.y - b * (K - 1);
    const int nc = call->st.n_copies[b];
    const int32_t* c = call->st.copies + ((size_t)b * K + q) * 3;
    __syncthreads();                                     // (every thread has read call->step's neighbours before it moves)
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) call->step += 1;
    if (q >= nc) return;
    const int src = c[0], dst = c[1], lo = c[2];
    const int cur = seq_len[src];
    if (cur <= lo) return;
    const size_t off = (size_t)lo * row_bytes, n16 = (size_t)(cur - lo) * row_bytes / 16;
    for (int r = blockIdx.x; r < runs; r += gridDim.x) {
        const int lw = r / n_head, h = r - lw * n_head;
        const char* s = kv + lw * lw_bytes + (size_t)src * slot_bytes + h * head_bytes + off;
        char* d = kv + lw * lw_bytes + (size_t)dst * slot_bytes + h * head_bytes + off;
        const uint4* s4 = reinterpret_cast<const uint4*>(s);
        uint4* d4 = reinterpret_cast<uint4*>(d);
        for (size_t i = threadIdx.x; i < n16; i += blockDim.x) d4[i] = s4[i];
    }
}

// k_kv_copy_span's whole-slot sibling (gvc_gpt_kv_fanout): blockIdx.y = pair, blockIdx.x strides over the (layer, k|v, head) runs; each
// run copies positions [0, seq_len[src]) of one head in 16-byte vectors.  Column 0 of a pair also copies the slot's decode state,
// (the pending token of a deferred decode included), columns 1 and 2 its parked logits / latent.  A pair with a slot outside [0, max_slots) or with src == dst copies nothing
__global__ void __launch_bounds__(256) k_kv_fanout(const int32_t* src_slots, const int32_t* dst_slots, char* kv, int runs, int n_head,
                                                   size_t lw_bytes, size_t slot_bytes, size_t head_bytes, int row_bytes, int max_seq,
                                                   int max_slots, int32_t* seq_len, int32_t* mel_pos, float* slot_logits, int vocab,
                                                   float* slot_latent, int d, int32_t* pending) {
    const int src = src_slots[blockIdx.y], dst = dst_slots[blockIdx.y];
    if (src < 0 || src >= max_slots || dst < 0 || dst >= max_slots || src == dst) return;
    const int cur = min(seq_len[src], max_seq);
    const size_t n16 = (size_t)max(cur, 0) * row_bytes / 16;
    for (int r = blockIdx.x; r < runs; r += gridDim.x) {
        const int lw = r / n_head, h = r - lw * n_head;
        const uint4* s4 = reinterpret_cast<const uint4*>(kv + lw * lw_bytes + (size_t)src * slot_bytes + h * head_bytes);
        uint4* d4 = reinterpret_cast<uint4*>(kv + lw * lw_bytes + (size_t)dst * slot_bytes + h * head_bytes);
        for (size_t i = threadIdx.x; i < n16; i += blockDim.x) d4[i] = s4[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        seq_len[dst] = seq_len[src];
        mel_pos[dst] = mel_pos[src];
        pending[dst] = pending[src];          // a deferred decode travels with the slot (its parked logits / latent are then stale on both)
    }
    if (blockIdx.x == 1 % gridDim.x)
        for (int i = threadIdx.x; i < vocab; i += blockDim.x) slot_logits[(size_t)dst * vocab + i] = slot_logits[(size_t)src * vocab + i];
    if (blockIdx.x == 2 % gridDim.x)
        for (int i = threadIdx.x; i < d; i += blockDim.x) slot_latent[(size_t)dst * d + i] = slot_latent[(size_t)src * d + i];
}

__global__ void k_beam_begin(BeamCall* dst, gvc_beam_state st, int i0, const int32_t* slots_in, int32_t* slot_table, float* logits,
                             const float* slot_logits) {
    const int BK = st.B * st.K, r = blockIdx.x;
    if (r == BK) {
        if (threadIdx.x == 0) { dst->st = st; dst->step = i0; dst->has_proc = 0; }
        if ((int)threadIdx.x < BK) slot_table[threadIdx.x] = slots_in[threadIdx.x];
        return;
    }
    // the first call starts every beam of an item from the logits its prefill parked in slot[b*K]
    const size_t sl = (size_t)(i0 == 0 ? slots_in[(r / st.K) * st.K] : slots_in[r]);
    for (int i = threadIdx.x; i < st.vocab; i += blockDim.x) logits[(size_t)r * st.vocab + i] = slot_logits[sl * st.vocab + i];
}

__global__ void k_beam_end(const int32_t* slot_table, int32_t* slots_out, const float* logits, float* slot_logits, int vocab) {
    const int r = blockIdx.x;
    const size_t sl = (size_t)slot_table[r];
    if (threadIdx.x == 0) slots_out[r] = slot_table[r];
    for (int i = threadIdx.x; i < vocab; i += blockDim.x) slot_logits[sl * vocab + i] = logits[(size_t)r * vocab + i];
}

int beam_check(const gvc_beam_state& st) {
    GVC_REQUIRE(st.B >= 1 && st.K >= 2 && st.K <= kBeamMaxK && st.vocab >= 2 && st.vocab <= 33 * 32 && st.K * st.vocab <= kBeamMaxN &&
                    st.B * st.K <= 64,
                GVC_ERR_ARG, "beam: B=%d K=%d vocab=%d outside the supported range (2 <= K <= 16, K*vocab <= %d, B*K <= 64)", st.B, st.K,
                st.vocab, kBeamMaxN);
    GVC_REQUIRE(st.eos >= 0 && st.eos < st.vocab && st.n0 >= 1 && st.max_new >= 1 && st.ids_stride >= st.n0 + st.max_new &&
                    (st.length_mode & 0xff) <= 1 && (st.length_mode >> 8) >= 0 && (st.length_mode >> 8) <= 2 && st.repetition_penalty > 0.f,
                GVC_ERR_ARG, "beam: bad state (n0 %d, max_new %d, ids_stride %d, length_mode %d)", st.n0, st.max_new, st.ids_stride,
                st.length_mode);
    GVC_REQUIRE(st.ids && st.scores && st.tokens && st.parents && st.done && st.hyp_score && st.hyp_len && st.hyp_tok && st.hyp_count &&
                    st.hyp_worst && st.copies && st.n_copies,
                GVC_ERR_ARG, "beam: null state array");
    return GVC_OK;
}

__global__ void k_beam_proc(BeamCall* dst, gvc_logits_processors proc) {
    if (threadIdx.x == 0) { dst->proc = proc; dst->has_proc = 1; }
}

int launch_beam_select(const gvc_beam_state& st, const gvc_logits_processors* proc, const BeamCall* call, int B, int K,
                       const float* logits, int32_t* slots, int t, int32_t* seq_len, int32_t* mel_pos, int32_t* tok_buf, hipStream_t s) {
    (void)K;
    hipLaunchKernelGGL(k_beam_select, dim3(B), dim3(kBeamThreads), 0, s, st, proc, call, logits, slots, t, seq_len, mel_pos, tok_buf);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int group_beam_check(const gvc_beam_state& st, const gvc_beam_groups& grp) {
    GVC_REQUIRE(grp.G >= 1 && grp.G <= st.K && st.K % grp.G == 0, GVC_ERR_ARG,
                "group beam: %d groups do not divide %d beams (1 <= G <= K, K %% G == 0)", grp.G, st.K);
    GVC_REQUIRE(grp.diversity_penalty >= 0.f && grp.diversity_penalty <= 3.0e38f, GVC_ERR_ARG,
                "group beam: diversity_penalty %g is not a finite value >= 0", (double)grp.diversity_penalty);
    GVC_REQUIRE(grp.done && grp.hyp_count && grp.hyp_worst, GVC_ERR_ARG, "group beam: null group array");
    return GVC_OK;
}

__global__ void k_beam_groups(BeamCall* dst, gvc_beam_groups grp) {
    if (threadIdx.x == 0) dst->grp = grp;
}

int launch_group_beam_select(const gvc_beam_state& st, const gvc_beam_groups& grp, const gvc_logits_processors* proc, const BeamCall* call,
                             int B, const float* logits, int32_t* slots, int t, int32_t* seq_len, int32_t* mel_pos, int32_t* tok_buf,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_group_beam_select, dim3(B), dim3(kBeamThreads), 0, s, st, grp, proc, call, logits, slots, t, seq_len, mel_pos,
                       tok_buf);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

__global__ void k_group_fan_src(const int32_t* slots, int32_t* src, int BK, int K) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < BK) src[r] = slots[(r / K) * K];
}

int launch_group_fan_src(const int32_t* slots, int32_t* src, int BK, int K, hipStream_t s) {
    hipLaunchKernelGGL(k_group_fan_src, dim3((BK + 63) / 64), dim3(64), 0, s, slots, src, BK, K);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_kv_copy_span(BeamCall* call, int B, int K, void* kv, int n_layer, int n_head, int max_seq, int hd, int max_slots, int esz,
                        const int32_t* seq_len, hipStream_t s) {
    GVC_REQUIRE((hd * esz) % 16 == 0, GVC_ERR_UNSUPPORTED, "kv_copy_span: head row of %d bytes is not a multiple of 16", hd * esz);
    const size_t head_bytes = (size_t)max_seq * hd * esz, slot_bytes = head_bytes * n_head, lw_bytes = slot_bytes * max_slots;
    hipLaunchKernelGGL(k_kv_copy_span, dim3(64, B * (K - 1)), dim3(256), 0, s, call, K, (char*)kv, 2 * n_layer * n_head, n_head, lw_bytes,
                       slot_bytes, head_bytes, hd * esz, seq_len);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_kv_fanout(const int32_t* src_slots, const int32_t* dst_slots, int n, void* kv, int n_layer, int n_head, int max_seq, int hd,
                     int max_slots, int esz, int32_t* seq_len, int32_t* mel_pos, float* slot_logits, int vocab, float* slot_latent, int d,
                     int32_t* pending, hipStream_t s) {
    GVC_REQUIRE((hd * esz) % 16 == 0, GVC_ERR_UNSUPPORTED, "kv_fanout: head row of %d bytes is not a multiple of 16", hd * esz);
    const size_t head_bytes = (size_t)max_seq * hd * esz, slot_bytes = head_bytes * n_head, lw_bytes = slot_bytes * max_slots;
    // one workgroup per run (960 at full size; a run is ~12 KB at a 48-row prompt).  With 64 strided workgroups per pair the call took
    // 58-62 us for 1, 3 and 7 pairs alike (profiles/nbest_time_fanout_grid64.json): its time did not follow its bytes
    const int runs = 2 * n_layer * n_head;
    hipLaunchKernelGGL(k_kv_fanout, dim3(runs < 1024 ? runs : 1024, n), dim3(256), 0, s, src_slots, dst_slots, (char*)kv, runs, n_head, lw_bytes,
                       slot_bytes, head_bytes, hd * esz, max_seq, max_slots, seq_len, mel_pos, slot_logits, vocab, slot_latent, d, pending);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_beam_begin(BeamCall* dst, const gvc_beam_state& st, const gvc_logits_processors* proc, const gvc_beam_groups* grp, int i0,
                      const int32_t* slots_in, int32_t* slot_table, float* logits, const float* slot_logits, hipStream_t s) {
    const int BK = st.B * st.K;
    hipLaunchKernelGGL(k_beam_begin, dim3(BK + 1), dim3(256), 0, s, dst, st, i0, slots_in, slot_table, logits, slot_logits);
    GVC_LAUNCH_CHECK();
    if (proc) {
        // (a second tiny launch, stream-ordered behind the begin that cleared has_proc; the struct travels as a kernel argument)
        hipLaunchKernelGGL(k_beam_proc, dim3(1), dim3(64), 0, s, dst, *proc);
        GVC_LAUNCH_CHECK();
    }
    if (grp) {
        hipLaunchKernelGGL(k_beam_groups, dim3(1), dim3(64), 0, s, dst, *grp);
        GVC_LAUNCH_CHECK();
    }
    return GVC_OK;
}

int launch_beam_end(const int32_t* slot_table, int32_t* slots_out, int BK, const float* logits, float* slot_logits, int vocab,
                    hipStream_t s) {
    hipLaunchKernelGGL(k_beam_end, dim3(BK), dim3(256), 0, s, slot_table, slots_out, logits, slot_logits, vocab);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc

extern "C" int gvc_beam_select(const gvc_beam_state* st, const float* logits, int32_t* slots, int32_t t, gvc_stream sv) {
    GVC_REQUIRE(st && logits && slots && t >= 0, GVC_ERR_ARG, "beam_select: bad argument");
    int rc = gvc::beam_check(*st);
    if (rc) return rc;
    GVC_REQUIRE(t < st->max_new && st->n0 + t < st->ids_stride, GVC_ERR_ARG, "beam_select: step %d past max_new %d", t, st->max_new);
    return gvc::launch_beam_select(*st, nullptr, nullptr, st->B, st->K, logits, slots, t, nullptr, nullptr, nullptr, (hipStream_t)sv);
}

extern "C" int gvc_beam_select_proc(const gvc_beam_state* st, const gvc_logits_processors* proc, const float* logits, int32_t* slots,
                                    int32_t t, gvc_stream sv) {
    GVC_REQUIRE(st && proc && logits && slots && t >= 0, GVC_ERR_ARG, "beam_select_proc: bad argument");
    int rc = gvc::beam_check(*st);
    if (rc) return rc;
    if ((rc = gvc::check_procs(*proc, st->vocab))) return rc;
    GVC_REQUIRE(t < st->max_new && st->n0 + t < st->ids_stride, GVC_ERR_ARG, "beam_select: step %d past max_new %d", t, st->max_new);
    hipStream_t s = (hipStream_t)sv;
    // a context-free entry point (tests, callers that decode themselves): the processors are staged for this call only
    gvc::BeamCall* d = nullptr;
    GVC_CHECK_HIP(hipMallocAsync((void**)&d, sizeof(gvc::BeamCall), s));
    hipLaunchKernelGGL(gvc::k_beam_proc, dim3(1), dim3(64), 0, s, d, *proc);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        rc = gvc::launch_beam_select(*st, &d->proc, nullptr, st->B, st->K, logits, slots, t, nullptr, nullptr, nullptr, s);
    else
        gvc::set_error("beam_select_proc: staging launch failed: %s", hipGetErrorString(e));
    const hipError_t e2 = hipFreeAsync(d, s);
    if (e != hipSuccess) return GVC_ERR_HIP;
    if (rc) return rc;
    GVC_CHECK_HIP(e2);
    return GVC_OK;
}

extern "C" int gvc_group_beam_select(const gvc_beam_state* st, const gvc_beam_groups* grp, const gvc_logits_processors* proc,
                                     const float* logits, int32_t* slots, int32_t t, gvc_stream sv) {
    GVC_REQUIRE(st && grp && logits && slots && t >= 0, GVC_ERR_ARG, "group_beam_select: bad argument");
    int rc = gvc::beam_check(*st);
    if (rc) return rc;
    if ((rc = gvc::group_beam_check(*st, *grp))) return rc;
    if (proc && (rc = gvc::check_procs(*proc, st->vocab))) return rc;
    GVC_REQUIRE(t < st->max_new && st->n0 + t < st->ids_stride, GVC_ERR_ARG, "group_beam_select: step %d past max_new %d", t, st->max_new);
    hipStream_t s = (hipStream_t)sv;
    if (!proc) return gvc::launch_group_beam_select(*st, *grp, nullptr, nullptr, st->B, logits, slots, t, nullptr, nullptr, nullptr, s);
    // (as gvc_beam_select_proc: the processors are staged for this call only)
    gvc::BeamCall* d = nullptr;
    GVC_CHECK_HIP(hipMallocAsync((void**)&d, sizeof(gvc::BeamCall), s));
    hipLaunchKernelGGL(gvc::k_beam_proc, dim3(1), dim3(64), 0, s, d, *proc);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        rc = gvc::launch_group_beam_select(*st, *grp, &d->proc, nullptr, st->B, logits, slots, t, nullptr, nullptr, nullptr, s);
    else
        gvc::set_error("group_beam_select: staging launch failed: %s", hipGetErrorString(e));
    const hipError_t e2 = hipFreeAsync(d, s);
    if (e != hipSuccess) return GVC_ERR_HIP;
    if (rc) return rc;
    GVC_CHECK_HIP(e2);
    return GVC_OK;
}
