// GPT context of libgenvc_hip: weight binding/repack, KV cache, prefill, decode step, latent re-pass,
// graph-replayed generation loop.  Reference seams: layers/gpt.py, layers/gpt_inference.py (see
// include/genvc_hip.h for the line-level mapping).
#include <stdlib.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "gemm.h"
#include <algorithm>
#include "gpt_kernels.h"
#include "persist_kernel.h"
#include "persist_rows.h"
#include "persist_rows_b16.h"
#include "gemm_b16.h"
#include "beam.h"
#include "cfg.h"
#include "contrastive.h"
#include "forward_eval.h"
#include "sampler.h"
#include "seqscore.h"
#include "spec.h"
#include "trace.h"

namespace gvc {

// ---------------------------------------------------------------------------------------------
// row kernels
// ---------------------------------------------------------------------------------------------
__global__ void k_ln_rows(const float* src, float* dst, int rows, int d, const float* w1, const float* b1,
                          const float* w2, const float* b2, int dst_fm16) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = src + (size_t)row * d;
    float* y = dst + (size_t)row * d;
    const float inv_d = 1.0f / (float)d;
    for (int pass = 0; pass < (w2 ? 2 : 1); ++pass) {
        const float* in = pass == 0 ? x : y;
        const float* gw = pass == 0 ? w1 : w2;
        const float* gb = pass == 0 ? b1 : b2;
        float s = 0.f;
        for (int k = lane * 4; k < d; k += 256) {
            const float4 v = *reinterpret_cast<const float4*>(in + k);
            s += (v.x + v.y) + (v.z + v.w);
        }
        const float mean = wave_sum(s) * inv_d;
        float q = 0.f;
        for (int k = lane * 4; k < d; k += 256) {
            const float4 v = *reinterpret_cast<const float4*>(in + k);
            const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_d + 1e-5f);
        for (int k = lane * 4; k < d; k += 256) {
            float4 v = *reinterpret_cast<const float4*>(in + k);
            const float4 g = *reinterpret_cast<const float4*>(gw + k);
            const float4 c = *reinterpret_cast<const float4*>(gb + k);
            v.x = (v.x - mean) * rstd * g.x + c.x; v.y = (v.y - mean) * rstd * g.y + c.y;
            v.z = (v.z - mean) * rstd * g.z + c.z; v.w = (v.w - mean) * rstd * g.w + c.w;
            if (dst_fm16 && !w2) *reinterpret_cast<float4*>(dst + fm16_index(row, k, d)) = v;
            else *reinterpret_cast<float4*>(y + k) = v;
        }
    }
}

__global__ void k_embed_rows(float* x, const float* prefix_emb, int B, int T, int P, int d, const float* mel_emb,
                             const float* mel_pos, const int32_t* codes, int n, int start_tok, int stop_tok, int t_off) {
    // rows [t_off, T) of every stream (t_off > 0: the leading rows are already in the KV cache)
    const int row = blockIdx.x;
    const int Tn = T - t_off;
    const int b = row / Tn, t = row - b * Tn + t_off;
    float* dst = x + (size_t)row * d;
    if (t < P) {
        const float* src = prefix_emb + ((size_t)b * P + t) * d;
        for (int k = threadIdx.x * 4; k < d; k += blockDim.x * 4)
            *reinterpret_cast<float4*>(dst + k) = *reinterpret_cast<const float4*>(src + k);
    } else {
        const int i = t - P;
        const int tok = i == 0 ? start_tok : (i <= n ? codes[(size_t)b * n + i - 1] : stop_tok);
        const float* e = mel_emb + (size_t)tok * d;
        const float* p = mel_pos + (size_t)i * d;
        for (int k = threadIdx.x * 4; k < d; k += blockDim.x * 4) {
            const float4 a = *reinterpret_cast<const float4*>(e + k);
            const float4 c = *reinterpret_cast<const float4*>(p + k);
            *reinterpret_cast<float4*>(dst + k) = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
        }
    }
}

__global__ void k_prefix_rows(float* out, const float* cond, int n_cond, const int32_t* codes, int B, int Tc,
                              int d, const float* text_emb, const float* text_pos, int start_text,
                              int stop_text) {
    const int P = n_cond + Tc + 2;
    const int row = blockIdx.x;
    const int b = row / P, t = row - b * P;
    float* dst = out + (size_t)row * d;
    if (t < n_cond) {
        const float* src = cond + ((size_t)b * n_cond + t) * d;
        for (int k = threadIdx.x * 4; k < d; k += blockDim.x * 4)
            *reinterpret_cast<float4*>(dst + k) = *reinterpret_cast<const float4*>(src + k);
    } else {
        const int i = t - n_cond;
        const int id = i == 0 ? start_text : (i <= Tc ? codes[(size_t)b * Tc + i - 1] : stop_text);
        const float* e = text_emb + (size_t)id * d;
        const float* p = text_pos + (size_t)i * d;
        for (int k = threadIdx.x * 4; k < d; k += blockDim.x * 4) {
            const float4 a = *reinterpret_cast<const float4*>(e + k);
            const float4 c = *reinterpret_cast<const float4*>(p + k);
            *reinterpret_cast<float4*>(dst + k) = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
        }
    }
}

// one workgroup per stream: x[b] = mel_embedding[tok[b]] + mel_pos_embedding[mel_pos[slot[b]]]  (gpt_inference.py:92-96)
__global__ void k_embed_decode_rows(float* x, const int32_t* tok, const int32_t* slots, GptState st, const float* mel_emb,
                                    const float* mel_pos, int d, int vocab) {
    const int b = blockIdx.x;
    // (clamped: after a step that produced garbage -- a timed-out hand-off -- the sampler may hand over any id)
    const float* e = mel_emb + (size_t)min(max(tok[b], 0), vocab - 1) * d;
    const float* p = mel_pos + (size_t)st.mel_pos[slots[b]] * d;
    float* dst = x + (size_t)b * d;
    for (int k = threadIdx.x * 4; k < d; k += blockDim.x * 4) {
        const float4 a = *reinterpret_cast<const float4*>(e + k);
        const float4 c = *reinterpret_cast<const float4*>(p + k);
        *reinterpret_cast<float4*>(dst + k) = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
}

// The generation loop's staging buffers (next-step logits and latent) are indexed by the position of a stream in the CALL;
// between calls they are parked per SLOT, so that consecutive calls may batch different sets of streams (streaming.py)
__global__ void k_stage_rows(float* stage, float* store, const int32_t* slots, int n, int to_store) {
    const int b = blockIdx.x;
    float* a = stage + (size_t)b * n;
    float* s = store + (size_t)slots[b] * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (to_store) s[i] = a[i];
        else a[i] = s[i];
    }
}

__global__ void k_set_state(GptState st, const int32_t* slots, int B, int seq_len, int mel_pos) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        st.seq_len[slots[b]] = seq_len;
        st.mel_pos[slots[b]] = mel_pos;
        st.pending[slots[b]] = -1;       // the slot starts over (prefill, reset, latents): a deferred decode of its old stream is dropped
    }
}

__global__ void k_gather_rows(const float* src, float* dst, int B, int T, int off, int n, int d) {
    const int row = blockIdx.x;
    const int b = row / n, i = row - b * n;
    const float* s = src + ((size_t)b * T + off + i) * d;
    float* o = dst + (size_t)row * d;
    for (int k = threadIdx.x * 4; k < d; k += blockDim.x * 4)
        *reinterpret_cast<float4*>(o + k) = *reinterpret_cast<const float4*>(s + k);
}

__global__ void k_round_bf16(float* w, unsigned short* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned u = __float_as_uint(w[i]);
        const unsigned r = u + 0x7fffu + ((u >> 16) & 1u);            // round to nearest even (finite inputs)
        out[i] = (unsigned short)(r >> 16);
        w[i] = __uint_as_float(r & 0xffff0000u);
    }
}

__global__ void k_transpose(const float* src, float* dst, int K, int N) {
    __shared__ float tile[32][33];
    const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int k = k0 + r, n = n0 + threadIdx.x;
        if (k < K && n < N) tile[r][threadIdx.x] = src[(size_t)k * N + n];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int n = n0 + r, k = k0 + threadIdx.x;
        if (k < K && n < N) dst[(size_t)n * K + k] = tile[threadIdx.x][r];
    }
}

// parameters of one gvc_gpt_generate call, resident on the device so the captured step graph
// is independent of them
struct GenCall {
    SampleCall sc;
    int32_t slots[64];
    gvc_row_sampling rows[kMaxSampleRows];   // per-row settings and keys of a gvc_gpt_generate_rows call (sc.rows points here)
    gvc_logits_processors proc;              // processors of a gvc_gpt_generate_proc call (sc.proc points here)
    gvc_logits_processors sets[kMaxSampleRows];   // processor sets of a gvc_gpt_generate_proc_sets call (sc.proc_sets points here)
    int32_t set_of_row[kMaxSampleRows];      // ... and each row's index into them, -1: none (sc.set_of_row points here)
    gvc_logits_warpers warps[kMaxSampleRows];     // warpers of a gvc_gpt_generate_warp call, one per set (sc.warps points here)
    float cfg_scale;                         // guidance scale of a gvc_gpt_generate_cfg call (k_cfg_guide reads it here)
    gvc_logits_bias bias;                    // sequence bias / bad words / forced EOS of a gvc_gpt_generate_bias call (sc.bias points here)
    gvc_logits_ras ras[kMaxSampleRows];      // RAS entries of a gvc_gpt_generate_ras call, one per set (sc.ras points here)
    gvc_logits_penalties pen[kMaxSampleRows];     // penalty entries of a gvc_gpt_generate_pen call, one per set (sc.pen points here)
    gvc_logits_watermark wm[kMaxSampleRows];      // watermark entries of a gvc_gpt_generate_wm call, one per set (sc.wm points here)
};

// Start / end of a gvc_gpt_generate call in ONE launch each (they used to be a memset, k_set_gen_call and two k_stage_rows before the
// step graphs and two k_stage_rows after them: six 4-5 us operations around every group of eight streaming steps).
// begin: workgroup b < B un-parks the next-step logits and latent of stream b; workgroup B resets the step counter and stores the
// call parameters.  end: workgroup b parks them again.
// Deferred decode (one stream on the one-launch step; see the generation loop below): pending is set, and workgroup 0 either hands the
// slot's pending token to the first decode launch (tok = pending, run flag up; the parked logits / latent are stale and stay where they
// are) or, with nothing pending, un-parks as ever and lowers the flag so that the first decode launch of the call leaves at once.
struct DeferRefs {
    const int32_t* pending;      // GptState::pending, or null: the eager order
    int32_t* run;                // run flag of the decode launches
    int32_t* tok;                // their token source (tok_buf)
};

__device__ __forceinline__ void gen_begin(GenCall* dst, const SampleCall& sc, const int32_t* slots, int B, int32_t* step_ctr, float* logits,
                                          const float* slot_logits, int vocab, float* latent, const float* slot_latent, int d,
                                          const DeferRefs& df) {
    const int b = blockIdx.x;
    if (b == B) {
        if (threadIdx.x == 0) { dst->sc = sc; *step_ctr = 0; }
        if (threadIdx.x < B) dst->slots[threadIdx.x] = slots[threadIdx.x];
        return;
    }
    const size_t sl = (size_t)slots[b];
    if (df.pending) {
        const int32_t t = df.pending[sl];
        if (threadIdx.x == 0) {
            *df.run = t >= 0;
            if (t >= 0) df.tok[b] = t;
        }
        if (t >= 0) return;
    }
    for (int i = threadIdx.x; i < vocab; i += blockDim.x) logits[(size_t)b * vocab + i] = slot_logits[sl * vocab + i];
    for (int i = threadIdx.x; i < d; i += blockDim.x) latent[(size_t)b * d + i] = slot_latent[sl * d + i];
}

__global__ void k_gen_begin(GenCall* dst, SampleCall sc, const int32_t* slots, int B, int32_t* step_ctr, float* logits, float* slot_logits,
                            int vocab, float* latent, float* slot_latent, int d, DeferRefs df) {
    gen_begin(dst, sc, slots, B, step_ctr, logits, slot_logits, vocab, latent, slot_latent, d, df);
}

// gvc_gpt_generate_rows: the same, and workgroup B also stores the call's row entries, which travel as a kernel argument (copied by
// the runtime when the launch is enqueued: the caller's host array is free when the call returns, and no staging buffer of the context
// can be overwritten by a later call before this launch has read it -- there is none)
__global__ void k_gen_begin_rows(GenCall* dst, SampleCall sc, const int32_t* slots, int B, int32_t* step_ctr, float* logits,
                                 float* slot_logits, int vocab, float* latent, float* slot_latent, int d, DeferRefs df, SampleRows rows) {
    if ((int)blockIdx.x == B && (int)threadIdx.x < B) dst->rows[threadIdx.x] = rows.r[threadIdx.x];
    gen_begin(dst, sc, slots, B, step_ctr, logits, slot_logits, vocab, latent, slot_latent, d, df);
}

// gvc_gpt_generate_proc: the same, and workgroup B also stores the call's processors (and row entries when ROWS), both kernel arguments
template <bool ROWS>
__global__ void k_gen_begin_proc(GenCall* dst, SampleCall sc, const int32_t* slots, int B, int32_t* step_ctr, float* logits,
                                 float* slot_logits, int vocab, float* latent, float* slot_latent, int d, DeferRefs df,
                                 SampleRows rows, gvc_logits_processors proc) {
    if ((int)blockIdx.x == B) {
        if (ROWS && (int)threadIdx.x < B) dst->rows[threadIdx.x] = rows.r[threadIdx.x];
        if (threadIdx.x == 0) dst->proc = proc;
    }
    gen_begin(dst, sc, slots, B, step_ctr, logits, slot_logits, vocab, latent, slot_latent, d, df);
}

// gvc_gpt_generate_proc_sets: the same, and workgroup B stores each row's set index (and row entries when ROWS), kernel arguments both.
// The sets themselves went ahead on the stream in launches of their own (launch_stage_proc_sets): 64 of them would not fit one argument
template <bool ROWS>
__global__ void k_gen_begin_sets(GenCall* dst, SampleCall sc, const int32_t* slots, int B, int32_t* step_ctr, float* logits,
                                 float* slot_logits, int vocab, float* latent, float* slot_latent, int d, DeferRefs df, SampleRows rows,
                                 SetIndex sor) {
    if ((int)blockIdx.x == B && (int)threadIdx.x < B) {
        if (ROWS) dst->rows[threadIdx.x] = rows.r[threadIdx.x];
        dst->set_of_row[threadIdx.x] = sor.k[threadIdx.x];
    }
    gen_begin(dst, sc, slots, B, step_ctr, logits, slot_logits, vocab, latent, slot_latent, d, df);
}

__global__ void k_gen_end(const int32_t* slots, const float* logits, float* slot_logits, int vocab, const float* latent, float* slot_latent,
                          int d) {
    const int b = blockIdx.x;
    const size_t sl = (size_t)slots[b];
    for (int i = threadIdx.x; i < vocab; i += blockDim.x) slot_logits[sl * vocab + i] = logits[(size_t)b * vocab + i];
    for (int i = threadIdx.x; i < d; i += blockDim.x) slot_latent[sl * d + i] = latent[(size_t)b * d + i];
}

// end of a deferring call: the token of the last sample stays pending for the slot instead of being decoded for nobody.  (A call of
// zero steps hands back what it found: the flag is still as the begin kernel set it, the token as it stored it.)
__global__ void k_gen_end_defer(const int32_t* slots, int32_t* pending, const int32_t* run, const int32_t* tok) {
    if (threadIdx.x == 0) pending[slots[0]] = *run ? tok[0] : -1;
}

// Flush of deferred decodes, ahead of anything that needs a slot's full state (a batched or searching call, an explicit decode step):
// row b's pending token and run flag for the conditional one-stream decode that follows for it, and the slot marked settled.  One thread,
// row after row: a slot listed twice is decoded once.
__global__ void k_flush_begin(const int32_t* slots, int B, int32_t* pending, int32_t* ftok, int32_t* frun) {
    if (threadIdx.x != 0) return;
    for (int b = 0; b < B; ++b) {
        const int sl = slots[b];
        const int32_t t = pending[sl];
        ftok[b] = t;
        frun[b] = t >= 0;
        pending[sl] = -1;
    }
}

}  // namespace gvc

using namespace gvc;

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
struct GptLayer {
    float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *proj_w, *proj_b, *ln2_w, *ln2_b, *fc_w, *fc_b, *p2_w, *p2_b;
    float *qkv_f = nullptr, *proj_f = nullptr, *fc_f = nullptr, *p2_f = nullptr;   // FM16 copies for the skinny prefill GEMM
    unsigned short *qkv_h = nullptr, *proj_h = nullptr, *fc_h = nullptr, *p2_h = nullptr;   // bf16 copies (bf16-weights contexts)
};

// What a captured generation graph bakes into its nodes, and so what tells two graphs of a context apart.
enum GraphKind { kStepGraph, kBeamGraph, kContrastiveGraph, kGroupBeamGraph, kCfgGraph };
struct GraphKey {
    int kind;       // GraphKind
    int rows;       // rows of the decode step: the call's B streams, B * K of a search, 2B of a guided call
    int K;          // beams / candidates per item (0: step graphs)
    int fused;      // GEMV groups with the fused attention + c_proj launch
    int split;      // GenPlan::split
    int unroll;     // steps in the graph
    int greedy;     // step graphs: the sampler kernel (searches carry no sampler: 0)
    int defer;      // step graphs: 1 = [decode the pending token, sample], 0 = [sample, decode]
    bool operator<(const GraphKey& o) const {
        return std::tie(kind, rows, K, fused, split, unroll, greedy, defer) <
               std::tie(o.kind, o.rows, o.K, o.fused, o.split, o.unroll, o.greedy, o.defer);
    }
};

// what the running gvc_gpt_trace call taps between the phases of run_rows (all device pointers, each nullable)
struct TraceCall {
    float* probs;              // [L][B][H][T][T]
    float* hidden;             // [L+1][B][T][d]
    float* align;              // [B][n][Tc]
    float* scratch;            // [B][H][T][T]: a layer's weights when probs is null
    const int32_t* lens;       // [B]
    int P, n, c0, Tc;
    unsigned long long layers; // bit l: layer l counts in align
    int n_chosen, last_chosen;
};

struct gvc_gpt {
    gvc_gpt_dims dm;
    int hd = 0, n_cu = 256;
    float* wbase = nullptr;           // one allocation for all weights
    float* wfm = nullptr;             // FM16 copies of the four per-layer matrices (prefill path)
    unsigned short* wh = nullptr;     // bf16 copies of the streamed matrices (weight_dtype = 1)
    unsigned short* head_h = nullptr;
    int bf16 = 0;
    float *mel_emb, *mel_pos, *text_emb, *text_pos, *lnf_w, *lnf_b, *fn_w, *fn_b, *head_w, *head_b;
    float* thead = nullptr;           // text_head.weight [n_text][d] | text_head.bias [n_text]: optional (gvc_gpt_head_xent, head 0), an allocation of its own
    int thead_bound = 0;              // bit 0: weight, bit 1: bias
    const uint8_t* eval_mask = nullptr;   // key-padding mask [B][eval_mask_stride] of the running gvc_gpt_forward_rows call (null outside it)
    int eval_mask_stride = 0;
    const struct TraceCall* trace = nullptr;   // taps of the running gvc_gpt_trace call (null outside it): run_rows keeps to its launch-per-phase loop
    std::vector<GptLayer> layers;
    std::map<std::string, int> bound;  // name -> 1 once bound
    int n_expected = 0;
    float* kv = nullptr;              // [L][2][slots][H][max_seq][hd], fp32 or (kv_bf16) bf16 elements
    int kv_bf16 = 0;
    int act_bf16 = 0;                 // weight_dtype 3: the one-launch rows step rounds the activations that cross its hand-offs (persist_rows_b16.h)
    // weight_dtype 4: every multi-row pass that is not a one-launch step multiplies on bf16 matrix cores (gemm_b16.h, run_rows_b16)
    int mfma_b16 = 0;
    unsigned short* wb16 = nullptr;   // per layer, FB16: bf16(c_attn g1) [3d][d] | c_proj [d][d] | bf16(c_fc g2) [4d][d] | mlp c_proj [d][4d]
    float* b16_fold = nullptr;        // per layer: S[3d] | C[3d] of LN1 -> c_attn and S[4d] | C[4d] of LN2 -> c_fc (k_rows_ln_fold_b16)
    float* b16_stats = nullptr;       // [rows padded to 16][2] (mean, rstd) of the bf16 rows the folded GEMM consumes
    std::vector<char> b16_dirty;      // per layer: a matrix or LayerNorm parameter was (re)bound -> repack before the next call (b16_prepare)
    int b16_any_dirty = 0;
    long long b16_launches = 0;       // bf16 strip GEMMs issued (gvc_gpt_bf16_gemm_launches; graph replays count once per capture)
    size_t kv_layer_stride = 0;       // floats per (layer, k|v)
    float *x = nullptr, *a = nullptr, *q = nullptr, *h = nullptr, *part = nullptr, *work = nullptr;
    long long work_cap = 0;
    float *x2 = nullptr, *part2 = nullptr;        // fused attention path: second residual buffer, per-head partials
    int fuse_decode = 1;                          // the fused attention + c_proj launch (k_attn_proj) serves short one-stream contexts
    int* seam_err_host = nullptr;                 // pinned, device-visible: a timed-out hand-off of the one-launch step / a full KV cache
    int* seam_err_dev = nullptr;
    int skinny_prefill = 1;                       // fragment-major weight copies + skinny / strip GEMMs (0 only when their allocation failed)
    int strip_prefill = 1;                        // more than 128 rows: strip GEMM
    int fuse_ln_rows = 8;                         // the LayerNorm-prologue GEMM serves up to this many rows (9+: separate launches win)
    int fuse_ln = 1;
    float* xalt = nullptr;                        // second residual buffer of that path [16][d]
    int rows_decode_min = 5;                      // batches of at least this many streams decode on the MFMA rows path (0: never);
                                                  // measured crossover: B=4 925 (GEMV) vs 975 us (rows), B=5 1242 vs 996 us
    float *logits = nullptr, *latent = nullptr;             // staging of the generation loop, indexed by position in the call
    float *slot_logits = nullptr, *slot_latent = nullptr;   // ... parked per slot between calls   // generate(): [slots][V], [slots][d]
    float* guided = nullptr;          // [slots / 2][V] guided scores of a gvc_gpt_generate_cfg step (what its sampler reads as logits)
    int32_t* spec_base = nullptr;     // [slots] cache position of the first row of a slot's verification pass (gvc_gpt_verify)
    int32_t* state = nullptr;         // seq_len[slots], mel_pos[slots], tok[slots], step
    GptState st;
    int32_t *tok_buf = nullptr, *step_ctr = nullptr;
    // deferred decode of a call's last token (one stream on the one-launch step; the generation loop below)
    int defer = 1;                    // GVC_DEFER_DECODE=0: the eager order [sample, decode] everywhere
    int defer_seen = 0;               // a deferring call has run: slots may hold pending tokens, and the entry points that need a slot's
                                      // full state enqueue flush launches first (never before, so other contexts pay nothing)
    int32_t *run_flag = nullptr;      // run flag of the decode launches of the deferring loop
    int32_t *flush_tok = nullptr, *flush_run = nullptr;   // [slots] token and run flag per row of a flush
    int32_t *flush_slot = nullptr;    // [1] slot table of the settling decode after a hand-off time-out
    long long* exec_ctr = nullptr;    // one-stream one-launch steps that ran, early exits not counted (gvc_gpt_one_stream_steps)
    GenCall* gen_call = nullptr;
    BeamCall* beam_call = nullptr;    // parameters of the running gvc_gpt_beam_generate call (device)
    CsCall* cs_call = nullptr;        // ... of the running gvc_gpt_contrastive_generate call (device)
    CsBufs cs = {};                   // contrastive context rows and scratch (gvc_gpt_warmup_contrastive, or the first call)
    hipStream_t cap_stream = nullptr;
    std::map<GraphKey, hipGraphExec_t> graphs;   // captured step, beam and contrastive graphs (get_graph / drop_graphs)
    int prof_only = -1;               // gvc_gpt_time_kernel(): launch only this kernel class
    int prof_skip_one = -1;           // ... or every class except this one
    unsigned long long* dbg = nullptr; // GVC_DEBUG_STAMPS: [launch][8] in-kernel timestamps of the eager decode step
    int dbg_n = 0;
    // one-launch decode step (persist_kernel.h), one stream
    int persist = 1;                  // GVC_PERSIST=0: launch-per-phase decode
    PersistLayer* p_layers = nullptr; // device table of per-layer pointers
    pu64* p_gran = nullptr;           // granule buffers of the in-kernel hand-offs
    unsigned* p_epoch = nullptr;      // [0] step epoch, [1] arrival counter
    unsigned long long* p_dbg = nullptr;   // GVC_PERSIST_STAMPS: wall-clock stamps of workgroup 0
    int p_ring_slots = 0, p_ascr = 0, p_hvec = 0;
    size_t p_lds = 0;
    int last_variant = 0;             // decode variant of the last gvc_gpt_generate call (gvc_gpt_decode_variant)
    int fallbacks = 0;                // hand-off timeouts that switched the one-launch steps off (gvc_gpt_health)
    int persist_cfg = 1;              // what GVC_PERSIST allowed at create (gvc_gpt_rearm restores it)
    // one-launch block stack for 2..16 rows (persist_rows.h): batched decode steps, cached chunk prefills
    int persist_rows = 1;             // GVC_PERSIST_ROWS=0: those calls keep the launch-per-phase rows path
    int persist_rows_min = 2;         // smallest row count the one-launch rows step serves
    long long r_launches = 0;         // one-launch rows steps issued (gvc_gpt_rows_step_launches; graph replays count once per capture)
    int r_ready = 0;                  // 0 not prepared yet, 1 ready, -1 unavailable on this device / for these dims
    RowsLayer* r_layers = nullptr;
    float* r_wpack = nullptr;         // packed weights [layer][256][192 KiB]
    float* r_bufs = nullptr;          // hand-off buffers, two parities
    float* r_lnfold = nullptr;        // per layer: S[3d] | C[3d] of LN1 -> c_attn and S[4d] | C[4d] of LN2 -> c_fc (k_rows_ln_fold)
    unsigned long long* r_dbg = nullptr;   // GVC_PERSIST_STAMPS
    std::vector<char> r_dirty;         // per layer: a matrix was re-bound after the pack was built (gvc_gpt_bind_weight) -> repack before use
    size_t r_lds = 0;
    int rows_keys_hint = 0;           // cached positions the longest stream of the running call reaches (set by the entry points)
    int p_xl = 1;                     // the one-stream step keeps the MLP's hidden units inside their XCD (GVC_PERSIST_XCD=0: never); cleared by
                                      // persist_prepare when the device does not deal a 256-workgroup grid as 8 XCDs x 32
    int arch_xcc = 0;                 // gcnArchName is gfx94x / gfx950: HW_REG_XCC_ID exists and means what the XL layout assumes
    long long lazy_inits = 0;         // allocations / device-wide syncs / graph captures done INSIDE a data-path call (gvc_gpt_lazy_inits)
    int in_warmup = 0;                // ... gvc_gpt_warmup's own do not count
};

static int gemv_init();

static int alloc_f(float** p, size_t n) {
    GVC_CHECK_HIP(hipMalloc((void**)p, n * sizeof(float)));
    return GVC_OK;
}

extern "C" int gvc_gpt_create(const gvc_gpt_dims* dims, gvc_gpt** out) {
    GVC_REQUIRE(dims && out, GVC_ERR_ARG, "gvc_gpt_create: null argument");
    const gvc_gpt_dims& D = *dims;
    GVC_REQUIRE(D.n_layer > 0 && D.n_head > 0 && D.d_model % D.n_head == 0, GVC_ERR_ARG, "bad GPT dims");
    const int hd = D.d_model / D.n_head;
    // the decode GEMVs keep a whole residual row in one wave (d / 256 float4 per lane): d = 256, 512, 768 or 1024
    // widths above 1024 (the reference takes every dimension from the checkpoint's config: inference/model_init.py:11-12,
    // configs/genVC_configs.py:127-139) run on the GEMM paths only -- prefill and decode alike as rows through the skinny / strip / tiled
    // GEMMs with separate LayerNorm launches, the head as a LayerNorm launch + a GEMM; the GEMV decode kernels and the one-launch steps
    // keep a residual row in one wave and stay at <= 1024
    GVC_REQUIRE(D.d_model % 256 == 0 && D.d_model >= 256 && D.d_model <= 2048, GVC_ERR_UNSUPPORTED,
                "d_model %d unsupported (a multiple of 256 up to 2048)", D.d_model);
    GVC_REQUIRE(hd == 64 || hd == 128 || hd == 256, GVC_ERR_UNSUPPORTED, "head_dim %d unsupported (64, 128 or 256)", hd);
    GVC_REQUIRE(D.max_slots >= 1 && D.max_slots <= 64, GVC_ERR_ARG, "max_slots must be in [1,64]");
    GVC_REQUIRE(D.max_rows >= D.max_slots, GVC_ERR_ARG, "max_rows must be >= max_slots");
    auto* c = new gvc_gpt();
    c->dm = D;
    c->hd = hd;
    int dev = 0;
    hipDeviceProp_t prop;
    GVC_CHECK_HIP(hipGetDevice(&dev));
    GVC_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->arch_xcc = strncmp(prop.gcnArchName, "gfx950", 6) == 0 || strncmp(prop.gcnArchName, "gfx94", 5) == 0;
    c->p_xl = getenv("GVC_PERSIST_XCD") ? atoi(getenv("GVC_PERSIST_XCD")) : 1;

    const size_t d = D.d_model, L = D.n_layer, V = D.vocab;
    const size_t per_layer = 2 * d + 3 * d * d + 3 * d + d * d + d + 2 * d + 4 * d * d + 4 * d + 4 * d * d + d;
    const size_t total = V * d + (size_t)D.max_mel_pos * d + (size_t)D.n_text * d + (size_t)D.max_text_pos * d +
                         4 * d + V * d + V + 64 + L * per_layer;
    int rc = alloc_f(&c->wbase, total + 64);
    if (rc) { delete c; return rc; }
    float* p = c->wbase;
    auto take = [&](size_t n) { float* r = p; p += (n + 3) & ~(size_t)3; return r; };
    c->mel_emb = take(V * d); c->mel_pos = take((size_t)D.max_mel_pos * d);
    c->text_emb = take((size_t)D.n_text * d); c->text_pos = take((size_t)D.max_text_pos * d);
    c->lnf_w = take(d); c->lnf_b = take(d); c->fn_w = take(d); c->fn_b = take(d);
    c->head_w = take(V * d); c->head_b = take(V);
    c->layers.resize(L);
    for (auto& ly : c->layers) {
        ly.ln1_w = take(d); ly.ln1_b = take(d); ly.qkv_w = take(3 * d * d); ly.qkv_b = take(3 * d);
        ly.proj_w = take(d * d); ly.proj_b = take(d); ly.ln2_w = take(d); ly.ln2_b = take(d);
        ly.fc_w = take(4 * d * d); ly.fc_b = take(4 * d); ly.p2_w = take(4 * d * d); ly.p2_b = take(d);
    }
    c->n_expected = 10 + 12 * (int)L;
    gemm_init_attributes();
    GVC_CHECK_HIP(hipMalloc((void**)&c->xalt, (size_t)16 * d * sizeof(float)));
    if (getenv("GVC_ROWS_DECODE_MIN")) c->rows_decode_min = atoi(getenv("GVC_ROWS_DECODE_MIN"));
    c->bf16 = D.weight_dtype >= 1;
    c->kv_bf16 = D.weight_dtype >= 2;
    c->act_bf16 = D.weight_dtype >= 3;
    c->mfma_b16 = D.weight_dtype == 4;
    GVC_REQUIRE(D.weight_dtype >= 0 && D.weight_dtype <= 4, GVC_ERR_ARG,
                "weight_dtype must be 0 (fp32), 1 (bf16 weights), 2 (bf16 weights + KV cache), 3 (2 + bf16 activations on the one-launch rows step) "
                "or 4 (3 + bf16 matrix cores on every other multi-row pass)");
    if (c->mfma_b16) {
        if (!(d % 256 == 0 && d <= 2048 && hd % 4 == 0)) {
            gvc_gpt_destroy(c);
            GVC_REQUIRE(false, GVC_ERR_UNSUPPORTED, "weight_dtype 4: the bf16 matrix-core kernels need d_model %% 256 == 0, d_model <= 2048 (got %d)", (int)d);
        }
        gemm_b16_init_attributes();
        if (hipMalloc((void**)&c->wb16, (size_t)L * 12 * d * d * sizeof(unsigned short)) != hipSuccess ||
            hipMalloc((void**)&c->b16_fold, (size_t)L * 14 * d * sizeof(float)) != hipSuccess ||
            hipMalloc((void**)&c->b16_stats, (((size_t)D.max_rows + 15) & ~(size_t)15) * 2 * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            gvc_gpt_destroy(c);
            GVC_REQUIRE(false, GVC_ERR_HIP, "weight_dtype 4: no memory for the bf16 fragment-major weight copies (%.0f MB)", L * 12.0 * d * d * 2 / 1e6);
        }
        c->b16_dirty.assign(L, 1);
        c->b16_any_dirty = 1;
    }
    if (c->bf16) {
        GVC_CHECK_HIP(hipMalloc((void**)&c->wh, (L * 12 * d * d + V * d + 64) * sizeof(unsigned short)));
        unsigned short* hq = c->wh;
        for (auto& ly : c->layers) {
            ly.qkv_h = hq; hq += 3 * d * d; ly.proj_h = hq; hq += d * d; ly.fc_h = hq; hq += 4 * d * d; ly.p2_h = hq; hq += 4 * d * d;
        }
        c->head_h = hq;
    }
    if (c->skinny_prefill) {
        // bf16-weights contexts keep the FM16 copies in bf16 too (half the bytes per pass; widened in registers)
        const size_t es = c->bf16 ? 2 : 4;
        if ((rc = alloc_f(&c->wfm, (L * 12 * d * d * es + 3) / 4))) { gvc_gpt_destroy(c); return rc; }
        char* f = reinterpret_cast<char*>(c->wfm);
        for (auto& ly : c->layers) {
            ly.qkv_f = reinterpret_cast<float*>(f); f += 3 * d * d * es; ly.proj_f = reinterpret_cast<float*>(f); f += d * d * es;
            ly.fc_f = reinterpret_cast<float*>(f); f += 4 * d * d * es; ly.p2_f = reinterpret_cast<float*>(f); f += 4 * d * d * es;
        }
    }

    c->kv_layer_stride = (size_t)D.max_slots * D.n_head * D.max_seq * hd;
    const size_t rows = ((size_t)D.max_rows + 15) & ~(size_t)15;       // fragment-major activations come in 16-row tiles
    c->work_cap = 8ll << 20;
    // weight_dtype 4: the N = d projections of EVERY multi-row pass leave K-split partials (there is no tiled-GEMM path behind the bf16
    // one), so the two halves of the scratch each hold max_rows x d floats whatever max_rows is
    if (c->mfma_b16 && (long long)2 * rows * d > c->work_cap) c->work_cap = (long long)2 * rows * d;
    if ((rc = alloc_f(&c->kv, (c->kv_bf16 ? 1 : 2) * L * c->kv_layer_stride)) || (rc = alloc_f(&c->x, rows * d)) ||
        (rc = alloc_f(&c->a, rows * d)) || (rc = alloc_f(&c->q, rows * d)) || (rc = alloc_f(&c->h, rows * 4 * d)) ||
        (rc = alloc_f(&c->part, (size_t)D.max_slots * D.n_head * kAttnChunks * (hd + 4))) ||
        (rc = alloc_f(&c->work, (size_t)c->work_cap)) || (rc = alloc_f(&c->logits, (size_t)D.max_slots * V)) ||
        (rc = alloc_f(&c->latent, (size_t)D.max_slots * d)) || (rc = alloc_f(&c->x2, (size_t)D.max_slots * d)) ||
        (rc = alloc_f(&c->slot_logits, (size_t)D.max_slots * V)) || (rc = alloc_f(&c->slot_latent, (size_t)D.max_slots * d)) ||
        (rc = alloc_f(&c->part2, (size_t)D.max_slots * D.n_head * d)) || (rc = alloc_f(&c->guided, (size_t)(D.max_slots / 2 + 1) * V))) {
        gvc_gpt_destroy(c);
        return rc;
    }
    const size_t nstate = 6 * (size_t)D.max_slots + 8;
    GVC_CHECK_HIP(hipMalloc((void**)&c->state, nstate * sizeof(int32_t)));
    GVC_CHECK_HIP(hipMemset(c->state, 0, nstate * sizeof(int32_t)));
    c->st.seq_len = c->state;
    c->st.mel_pos = c->state + D.max_slots;
    c->tok_buf = c->state + 2 * D.max_slots;
    c->step_ctr = c->state + 3 * D.max_slots;
    c->st.pending = c->state + 3 * D.max_slots + 4;
    c->flush_tok = c->state + 4 * D.max_slots + 4;
    c->flush_run = c->state + 5 * D.max_slots + 4;
    c->run_flag = c->state + 6 * D.max_slots + 4;
    c->flush_slot = c->state + 6 * D.max_slots + 5;
    GVC_CHECK_HIP(hipMemset(c->st.pending, 0xff, (size_t)D.max_slots * sizeof(int32_t)));      // -1: nothing pending
    GVC_CHECK_HIP(hipMalloc((void**)&c->exec_ctr, sizeof(long long)));
    GVC_CHECK_HIP(hipMalloc((void**)&c->spec_base, (size_t)D.max_slots * sizeof(int32_t)));
    GVC_CHECK_HIP(hipMemset(c->spec_base, 0, (size_t)D.max_slots * sizeof(int32_t)));
    GVC_CHECK_HIP(hipMemset(c->exec_ctr, 0, sizeof(long long)));
    GVC_CHECK_HIP(hipDeviceSynchronize());      // (the memsets went to the legacy default stream; callers may use non-blocking ones)
    if (getenv("GVC_DEFER_DECODE")) c->defer = atoi(getenv("GVC_DEFER_DECODE")) != 0;
    GVC_CHECK_HIP(hipMalloc((void**)&c->gen_call, sizeof(GenCall)));
    GVC_CHECK_HIP(hipMalloc((void**)&c->beam_call, sizeof(BeamCall)));
    GVC_CHECK_HIP(hipMalloc((void**)&c->cs_call, sizeof(CsCall)));
    GVC_CHECK_HIP(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    if ((rc = gemv_init())) { gvc_gpt_destroy(c); return rc; }
    GVC_CHECK_HIP(hipHostMalloc((void**)&c->seam_err_host, sizeof(int), hipHostMallocMapped));
    *c->seam_err_host = 0;
    GVC_CHECK_HIP(hipHostGetDevicePointer((void**)&c->seam_err_dev, c->seam_err_host, 0));
    if (getenv("GVC_PERSIST")) c->persist = atoi(getenv("GVC_PERSIST"));
    c->persist_cfg = c->persist;
    if (getenv("GVC_PERSIST_ROWS")) c->persist_rows = atoi(getenv("GVC_PERSIST_ROWS"));
    if (getenv("GVC_DEBUG_STAMPS")) {
        GVC_CHECK_HIP(hipMalloc((void**)&c->dbg, 4096 * 8 * sizeof(unsigned long long)));
        GVC_CHECK_HIP(hipMemset(c->dbg, 0, 4096 * 8 * sizeof(unsigned long long)));
    }
    *out = c;
    return GVC_OK;
}

// every captured graph of the context, whatever its kind
static void drop_graphs(gvc_gpt* c) {
    for (auto& kvp : c->graphs) (void)hipGraphExecDestroy(kvp.second);
    c->graphs.clear();
}

extern "C" int gvc_gpt_destroy(gvc_gpt* c) {
    if (!c) return GVC_OK;
    drop_graphs(c);
    if (c->cap_stream) hipStreamDestroy(c->cap_stream);
    if (c->xalt) hipFree(c->xalt);
    if (c->thead) hipFree(c->thead);
    if (c->seam_err_host) hipHostFree(c->seam_err_host);
    for (void* p : {(void*)c->p_layers, (void*)c->p_gran, (void*)c->p_epoch, (void*)c->p_dbg, (void*)c->r_layers, (void*)c->r_wpack,
                    (void*)c->r_bufs, (void*)c->r_dbg, (void*)c->r_lnfold, (void*)c->wb16, (void*)c->b16_fold, (void*)c->b16_stats})
        if (p) hipFree(p);
    for (void* p : {(void*)c->wbase, (void*)c->wfm, (void*)c->wh, (void*)c->kv, (void*)c->x, (void*)c->a, (void*)c->q, (void*)c->h,
                    (void*)c->part, (void*)c->work, (void*)c->logits, (void*)c->latent, (void*)c->slot_logits, (void*)c->slot_latent, (void*)c->state, (void*)c->x2, (void*)c->part2,
                    (void*)c->gen_call, (void*)c->beam_call, (void*)c->cs_call, (void*)c->exec_ctr, (void*)c->guided, (void*)c->spec_base})
        if (p) hipFree(p);
    cs_free(&c->cs);
    delete c;
    return GVC_OK;
}

static int copy_w(float* dst, const float* src, int64_t numel, int64_t expect, const char* name, hipStream_t s) {
    GVC_REQUIRE(numel == expect, GVC_ERR_ARG, "%s: expected %lld elements, got %lld", name, (long long)expect,
                (long long)numel);
    GVC_CHECK_HIP(hipMemcpyAsync(dst, src, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    return GVC_OK;
}

// HF Conv1D weight [K][N] -> row-per-output [N][K]
static int transpose_w(float* dst, const float* src, int64_t numel, int K, int N, const char* name, hipStream_t s,
                       float* dst_fm16 = nullptr, unsigned short* dst_bf16 = nullptr) {
    GVC_REQUIRE(numel == (int64_t)K * N, GVC_ERR_ARG, "%s: expected %lld elements, got %lld", name,
                (long long)K * N, (long long)numel);
    hipLaunchKernelGGL(k_transpose, dim3(cdiv(N, 32), cdiv(K, 32)), dim3(32, 8), 0, s, src, dst, K, N);
    GVC_LAUNCH_CHECK();
    if (dst_bf16) {      // bf16-weights context: every path uses the SAME rounded values (fp32 copy rounded in place)
        hipLaunchKernelGGL(k_round_bf16, dim3(1024), dim3(256), 0, s, dst, dst_bf16, (size_t)K * N);
        GVC_LAUNCH_CHECK();
    }
    if (dst_fm16) {      // second copy in MFMA fragment order for the skinny prefill GEMM (bf16 elements in a bf16-weights context)
        if (dst_bf16) hipLaunchKernelGGL(k_to_fm16_bf16, dim3(1024), dim3(256), 0, s, dst, reinterpret_cast<unsigned short*>(dst_fm16), N, K);
        else hipLaunchKernelGGL(k_to_fm16, dim3(1024), dim3(256), 0, s, dst, dst_fm16, N, K);
        GVC_LAUNCH_CHECK();
    }
    return GVC_OK;
}

static void mark_rows_pack_dirty(gvc_gpt* c, int li);
extern "C" int gvc_gpt_bind_weight(gvc_gpt* c, const char* name, const float* src, int64_t numel, gvc_stream sv) {
    GVC_REQUIRE(c && name && src, GVC_ERR_ARG, "gvc_gpt_bind_weight: null argument");
    hipStream_t s = (hipStream_t)sv;
    const int64_t d = c->dm.d_model, V = c->dm.vocab;
    std::string n(name);
    int rc = GVC_OK;
    bool known = true;
    if (n == "mel_embedding.weight") rc = copy_w(c->mel_emb, src, numel, V * d, name, s);
    else if (n == "mel_pos_embedding.emb.weight") rc = copy_w(c->mel_pos, src, numel, c->dm.max_mel_pos * d, name, s);
    else if (n == "text_embedding.weight") rc = copy_w(c->text_emb, src, numel, c->dm.n_text * d, name, s);
    else if (n == "text_pos_embedding.emb.weight") rc = copy_w(c->text_pos, src, numel, c->dm.max_text_pos * d, name, s);
    else if (n == "gpt.ln_f.weight") rc = copy_w(c->lnf_w, src, numel, d, name, s);
    else if (n == "gpt.ln_f.bias") rc = copy_w(c->lnf_b, src, numel, d, name, s);
    else if (n == "final_norm.weight") rc = copy_w(c->fn_w, src, numel, d, name, s);
    else if (n == "final_norm.bias") rc = copy_w(c->fn_b, src, numel, d, name, s);
    else if (n == "mel_head.weight") {
        rc = copy_w(c->head_w, src, numel, V * d, name, s);
        if (rc == GVC_OK && c->bf16) {
            hipLaunchKernelGGL(k_round_bf16, dim3(1024), dim3(256), 0, s, c->head_w, c->head_h, (size_t)(V * d));
            GVC_LAUNCH_CHECK();
        }
    }
    else if (n == "mel_head.bias") rc = copy_w(c->head_b, src, numel, V, name, s);
    else if (n == "text_head.weight" || n == "text_head.bias") {
        // the evaluation pass alone reads it (gvc_gpt_head_xent): not among the expected tensors, so an inference-only bind stays complete
        const int64_t nt = c->dm.n_text, nt4 = (nt * d + 3) & ~(int64_t)3;
        if (!c->thead) GVC_CHECK_HIP(hipMalloc((void**)&c->thead, (size_t)(nt4 + nt) * sizeof(float)));
        const bool w = n == "text_head.weight";
        rc = copy_w(w ? c->thead : c->thead + nt4, src, numel, w ? nt * d : nt, name, s);
        if (rc == GVC_OK) c->thead_bound |= w ? 1 : 2;
        return rc;
    }
    else if (n.rfind("gpt.h.", 0) == 0) {
        const size_t dot = n.find('.', 6);
        GVC_REQUIRE(dot != std::string::npos, GVC_ERR_ARG, "malformed weight name %s", name);
        const int li = atoi(n.substr(6, dot - 6).c_str());
        const std::string rest = n.substr(dot + 1);
        GVC_REQUIRE(li >= 0 && li < c->dm.n_layer, GVC_ERR_ARG, "%s: layer out of range", name);
        GptLayer& ly = c->layers[li];
        if (rest == "ln_1.weight") { rc = copy_w(ly.ln1_w, src, numel, d, name, s); mark_rows_pack_dirty(c, li); }   // (the rows step folds the
        else if (rest == "ln_1.bias") { rc = copy_w(ly.ln1_b, src, numel, d, name, s); mark_rows_pack_dirty(c, li); }    //  LayerNorm into per-row constants)
        else if (rest == "attn.c_attn.weight") { rc = transpose_w(ly.qkv_w, src, numel, d, 3 * d, name, s, ly.qkv_f, ly.qkv_h); mark_rows_pack_dirty(c, li); }
        else if (rest == "attn.c_attn.bias") { rc = copy_w(ly.qkv_b, src, numel, 3 * d, name, s); mark_rows_pack_dirty(c, li); }
        else if (rest == "attn.c_proj.weight") { rc = transpose_w(ly.proj_w, src, numel, d, d, name, s, ly.proj_f, ly.proj_h); mark_rows_pack_dirty(c, li); }
        else if (rest == "attn.c_proj.bias") rc = copy_w(ly.proj_b, src, numel, d, name, s);
        else if (rest == "ln_2.weight") { rc = copy_w(ly.ln2_w, src, numel, d, name, s); mark_rows_pack_dirty(c, li); }
        else if (rest == "ln_2.bias") { rc = copy_w(ly.ln2_b, src, numel, d, name, s); mark_rows_pack_dirty(c, li); }
        else if (rest == "mlp.c_fc.weight") { rc = transpose_w(ly.fc_w, src, numel, d, 4 * d, name, s, ly.fc_f, ly.fc_h); mark_rows_pack_dirty(c, li); }
        else if (rest == "mlp.c_fc.bias") { rc = copy_w(ly.fc_b, src, numel, 4 * d, name, s); mark_rows_pack_dirty(c, li); }
        else if (rest == "mlp.c_proj.weight") { rc = transpose_w(ly.p2_w, src, numel, 4 * d, d, name, s, ly.p2_f, ly.p2_h); mark_rows_pack_dirty(c, li); }
        else if (rest == "mlp.c_proj.bias") rc = copy_w(ly.p2_b, src, numel, d, name, s);
        else known = false;   // attn.bias / attn.masked_bias buffers of 4.33-era checkpoints
    } else {
        known = false;        // text_head.*, conditioning_perceiver.*, gpt.wte.* ... (strict=False)
    }
    if (rc == GVC_OK && known) c->bound[n] = 1;
    return rc;
}

// a block matrix of layer li was (re)bound: the one-launch rows step's packed copy of that layer must be rebuilt before its next use
static void mark_rows_pack_dirty(gvc_gpt* c, int li) {
    if (c->r_ready == 1 && li < (int)c->r_dirty.size()) c->r_dirty[li] = 1;
    if (c->mfma_b16 && li < (int)c->b16_dirty.size()) { c->b16_dirty[li] = 1; c->b16_any_dirty = 1; }     // (the bf16 matrix-core copies too)
}

extern "C" int gvc_gpt_missing_weights(gvc_gpt* c) {
    if (!c) return -1;
    return c->n_expected - (int)c->bound.size();
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
struct GemvGeom { int NI, ksplit, wpb, grid; };

// launch geometry of a decode GEMV over Wt[N][K]: one wave per (row, 1024-input segment); about one
// workgroup per CU, two when that would need more than 12 compute waves
static int gemv_geom(const gvc_gpt* c, int N, int K, GemvGeom* g) {
    // a wave owns a segment of NI * 256 inputs: the whole row when K <= 1024, else the largest NI <= 4 that divides K / 256
    const int k256 = K / 256;
    g->NI = k256 <= 4 ? k256 : (k256 % 4 == 0 ? 4 : (k256 % 3 == 0 ? 3 : (k256 % 2 == 0 ? 2 : 1)));
    GVC_REQUIRE(K % 256 == 0 && g->NI >= 1, GVC_ERR_UNSUPPORTED, "gemv: K=%d unsupported", K);
    g->ksplit = K / (g->NI * 256);
    GVC_REQUIRE(g->ksplit * g->NI * 256 == K && g->ksplit <= 8, GVC_ERR_UNSUPPORTED, "gemv: K=%d unsupported", K);
    const int items = N * g->ksplit;
    constexpr int wpb_split = 12, blocks_per_cu = 1;        // (swept in round 1: profiles/r01_microbench_notes.md)
    int wpb = cdiv(items, blocks_per_cu * c->n_cu);
    if (wpb > wpb_split) wpb = cdiv(items, 2 * blocks_per_cu * c->n_cu);
    if (wpb < 4) wpb = 4;
    wpb = cdiv(wpb, g->ksplit) * g->ksplit;
    if (wpb > 15) wpb = 15 / g->ksplit * g->ksplit;
    g->wpb = wpb;
    g->grid = cdiv(items, wpb);
    return GVC_OK;
}

template <int PRO, int EPI>
static int launch_gemv(gvc_gpt* c, GemvArgs A, int B, hipStream_t s) {
    GemvGeom g;
    int rc = gemv_geom(c, A.N, A.K, &g);
    if (rc) return rc;
    if (PRO == PRO_LN_SUM && g.wpb > 8) {            // this variant is compiled for <= 512 threads
        g.wpb = 8 / g.ksplit * g.ksplit;
        g.grid = cdiv(A.N * g.ksplit, g.wpb);
    }
    const int NI = g.NI;
    A.ksplit = g.ksplit;
    A.wpb = g.wpb;
    A.B = B;
    if (c->dbg && c->dbg_n < 4096) A.dbg = c->dbg + 8 * (size_t)(c->dbg_n++);
    const int BT = B <= 1 ? 1 : (B <= 2 ? 2 : (B <= 4 ? 4 : 8));
    const int grid = g.grid;
    const int wpb = g.wpb;
    const int nthreads = wpb * 64;
    const size_t lds = ((size_t)BT * A.K + (size_t)wpb * BT) * sizeof(float);
#define GVC_GEMV_CASE(bt, ni)                                                    \
    if (BT == bt && NI == ni) {                                                  \
        if (A.Wt16) hipLaunchKernelGGL((k_gemv<bt, ni, PRO, EPI, 1>), dim3(grid), dim3(nthreads), lds, s, A); \
        else hipLaunchKernelGGL((k_gemv<bt, ni, PRO, EPI, 0>), dim3(grid), dim3(nthreads), lds, s, A); \
        GVC_LAUNCH_CHECK();                                                      \
        return GVC_OK;                                                           \
    }
    GVC_GEMV_CASE(1, 1) GVC_GEMV_CASE(1, 2) GVC_GEMV_CASE(1, 3) GVC_GEMV_CASE(1, 4)
    GVC_GEMV_CASE(2, 1) GVC_GEMV_CASE(2, 2) GVC_GEMV_CASE(2, 3) GVC_GEMV_CASE(2, 4)
    GVC_GEMV_CASE(4, 1) GVC_GEMV_CASE(4, 2) GVC_GEMV_CASE(4, 3) GVC_GEMV_CASE(4, 4)
    GVC_GEMV_CASE(8, 1) GVC_GEMV_CASE(8, 2) GVC_GEMV_CASE(8, 3) GVC_GEMV_CASE(8, 4)
#undef GVC_GEMV_CASE
    set_error("gemv: no instantiation for BT=%d NI=%d", BT, NI);
    return GVC_ERR_UNSUPPORTED;
}

// dynamic LDS above 64 KiB needs an opt-in per kernel; done once at context creation (never while a
// stream is capturing)
template <int PRO, int EPI>
static int gemv_allow_big_lds() {
#define GVC_GEMV_ATTR(bt, ni)                                                                              \
    GVC_CHECK_HIP(hipFuncSetAttribute((const void*)k_gemv<bt, ni, PRO, EPI, 0>,                            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));            \
    GVC_CHECK_HIP(hipFuncSetAttribute((const void*)k_gemv<bt, ni, PRO, EPI, 1>,                            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
    GVC_GEMV_ATTR(1, 1) GVC_GEMV_ATTR(1, 2) GVC_GEMV_ATTR(1, 3) GVC_GEMV_ATTR(1, 4)
    GVC_GEMV_ATTR(2, 1) GVC_GEMV_ATTR(2, 2) GVC_GEMV_ATTR(2, 3) GVC_GEMV_ATTR(2, 4)
    GVC_GEMV_ATTR(4, 1) GVC_GEMV_ATTR(4, 2) GVC_GEMV_ATTR(4, 3) GVC_GEMV_ATTR(4, 4)
    GVC_GEMV_ATTR(8, 1) GVC_GEMV_ATTR(8, 2) GVC_GEMV_ATTR(8, 3) GVC_GEMV_ATTR(8, 4)
#undef GVC_GEMV_ATTR
    return GVC_OK;
}

static int gemv_init() {
    int rc;
    if ((rc = gemv_allow_big_lds<PRO_LN, EPI_QKV>())) return rc;
    if ((rc = gemv_allow_big_lds<PRO_MERGE, EPI_RESID>())) return rc;
    if ((rc = gemv_allow_big_lds<PRO_LN, EPI_GELU>())) return rc;
    if ((rc = gemv_allow_big_lds<PRO_LN_SUM, EPI_GELU>())) return rc;
    if ((rc = gemv_allow_big_lds<PRO_COPY, EPI_RESID>())) return rc;
    return gemv_allow_big_lds<PRO_LN2X, EPI_LOGITS>();
}

// K (which = 0) or V (1) cache of a layer; element size follows the context's KV dtype
static float* kv_layer(const gvc_gpt* c, int layer, int which) {
    return reinterpret_cast<float*>(reinterpret_cast<char*>(c->kv) + (size_t)(2 * layer + which) * c->kv_layer_stride * (c->kv_bf16 ? 2 : 4));
}

static GemvArgs base_args(gvc_gpt* c, const int32_t* slots, int row0) {
    GemvArgs A;
    memset(&A, 0, sizeof(A));
    A.d = c->dm.d_model;
    A.x = c->x + (size_t)row0 * A.d;
    A.x_stride = 1;
    A.x_off = 0;
    A.n_head = c->dm.n_head;
    A.head_dim = c->hd;
    A.max_seq = c->dm.max_seq;
    A.max_mel_pos = c->dm.max_mel_pos;
    A.slots = slots;
    A.st = c->st;
    A.mel_emb = c->mel_emb;
    A.mel_pos_tab = c->mel_pos;
    A.kv_bf16 = c->kv_bf16;
    A.err = c->seam_err_dev;
    return A;
}

static int launch_attention(gvc_gpt* c, AttnArgs T, int chunks, int rows, bool direct, hipStream_t s, bool wide = false) {
    // prefill-shaped calls (>= 16 rows per stream): 16-row query tiles on the matrix cores
    int rc = GVC_OK;
    if (c->eval_mask) {            // the evaluation pass: key-padding mask inside the tile kernels, whatever the tile count
        GVC_REQUIRE(direct && chunks == 1 && !wide && !c->kv_bf16 && rows % T.T == 0, GVC_ERR_STATE, "masked attention outside a whole-sequence fp32 pass");
        T.key_mask = c->eval_mask;
        T.mask_stride = c->eval_mask_stride;
        return launch_attention_tile_masked(c->hd, c->dm.n_head, T, rows / T.T, T.T, s);
    }
    if (direct && chunks == 1 && !wide && T.T >= 16 && rows % T.T == 0 &&
        launch_attention_tile(c->hd, c->dm.n_head, T, rows / T.T, T.base_len ? c->dm.max_seq : T.T, s, c->kv_bf16 != 0, &rc))
        return rc;
    return launch_attention_hd(c->hd, c->dm.n_head, T, chunks, rows, direct, s, wide && c->hd == 256, c->kv_bf16 != 0);
}

static AttnArgs gpt_attn_args(gvc_gpt* c, int layer, const int32_t* slots) {
    AttnArgs T;
    memset(&T, 0, sizeof(T));
    T.q_stride = c->dm.d_model;
    T.kbase = kv_layer(c, layer, 0);
    T.vbase = kv_layer(c, layer, 1);
    T.k_batch_stride = (long long)c->dm.n_head * c->dm.max_seq * c->hd;
    T.k_head_stride = (long long)c->dm.max_seq * c->hd;
    T.k_row_stride = c->hd;
    T.slots = slots;
    T.causal = 1;
    T.scale = 1.0f / sqrtf((float)c->hd);
    return T;
}

// one decode step for a group of <= 8 streams whose scratch rows start at row0
// gvc_gpt_time_kernel(): when prof_only >= 0 only that kernel class of the step is launched
static inline bool prof_skip(const gvc_gpt* c, int which) {
    return (c->prof_only >= 0 && c->prof_only != which) || c->prof_skip_one == which;
}

// can the fused attention + c_proj launch serve this call?  one stream, head_dim 256, and the caller
// guarantees at most 8 * kFusedMaxKeys cached positions for the whole run (gvc_gpt_generate: ids_stride)
static bool fused_ok(const gvc_gpt* c, int B, int max_keys) {
    return c->fuse_decode && B == 1 && c->hd == 256 && c->dm.d_model % 16 == 0 && c->dm.d_model <= 1024 && max_keys <= 8 * kFusedMaxKeys;
}

// ---------------------------------------------------------------------------------------------
// one-launch decode step (persist_kernel.h)
// ---------------------------------------------------------------------------------------------
// test hook (tests/test_gpu_gpt.py): GVC_PERSIST_TEST_GRID=255 launches the one-launch steps one workgroup short, which is what a
// non-resident workgroup looks like to the others -- every hand-off times out and the fallback of check_ready must take over
static int persist_test_grid() {
    const char* e = getenv("GVC_PERSIST_TEST_GRID");        // (read per launch: a test sets and clears it inside one process)
    const int g = e ? atoi(e) : kPG;
    return g > 0 && g <= kPG ? g : kPG;
}

// the instantiation that serves this context: d_model / 256, bf16 weight storage, bf16 KV cache (bf16 rows are streamed in whole
// KiB per workgroup and phase, which needs an even d_model / 256)
typedef void (*persist_fn)(const PersistArgs);
// d_model 1024: the stamping variant (STAMPS = true) only when the stamp buffer exists (GVC_PERSIST_STAMPS; persist_prepare allocates
// it for d_model 1024 alone), the production variant otherwise
template <bool STAMPS>
static persist_fn persist_kernel_1024(const gvc_gpt* c) {
    // p_xl = 0 (GVC_PERSIST_XCD=0, or a device that does not deal 8 XCDs x 32 workgroups: persist_prepare's probe): d_model 1024 keeps the
    // device-wide hand-off of the hidden units (the round-3 kernel)
    if (c->p_xl) {
        if (c->kv_bf16) return (persist_fn)k_decode_persist<4, 1, 1, 1, STAMPS>;
        if (c->bf16) return (persist_fn)k_decode_persist<4, 1, 0, 1, STAMPS>;
        return (persist_fn)k_decode_persist<4, 0, 0, 1, STAMPS>;
    }
    if (c->kv_bf16) return (persist_fn)k_decode_persist<4, 1, 1, 0, STAMPS>;
    if (c->bf16) return (persist_fn)k_decode_persist<4, 1, 0, 0, STAMPS>;
    return (persist_fn)k_decode_persist<4, 0, 0, 0, STAMPS>;
}
static persist_fn persist_kernel(const gvc_gpt* c) {
    const int nd = c->dm.d_model / 256;
    if (nd == 4) return c->p_dbg ? persist_kernel_1024<true>(c) : persist_kernel_1024<false>(c);
    if (c->kv_bf16) return (persist_fn)k_decode_persist<2, 1, 1>;
    if (c->bf16) return (persist_fn)k_decode_persist<2, 1, 0>;
    return nd == 3 ? (persist_fn)k_decode_persist<3> : nd == 2 ? (persist_fn)k_decode_persist<2> : (persist_fn)k_decode_persist<1>;
}

// one stream, fp32 weights and cache, a full MI355X (one workgroup per CU)
static bool persist_ok(const gvc_gpt* c, int B) {
    const int d = c->dm.d_model;
    return c->persist && B == 1 && (!c->bf16 || d == 512 || d == 1024) && c->n_cu >= kPG && d % 256 == 0 && d <= 1024 &&
           (c->hd == 64 || c->hd == 128 || c->hd == 256) && c->dm.n_layer < 500;
}

// Topology probe for the XCD-local hand-off (k_decode_persist<4, *, *, 1>): a grid of the one-launch step's own shape (256 workgroups, its
// threads and LDS, so one per CU), all co-resident (they wait for each other, bounded), each adding itself to its XCD's counter.
// hist[0..7]: workgroups per XCC_ID; hist[8]: arrivals; hist[9]: workgroups that gave up waiting.
__global__ __launch_bounds__(gvc::kPThreads) void k_xcd_probe(unsigned* hist) {
    if (threadIdx.x != 0) return;
    unsigned xcc = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    atomicAdd(hist + (xcc & 7u), 1u);
    atomicAdd(hist + 8, 1u);
    for (unsigned i = 0; i < (1u << 16); ++i) {         // (~0.1 s at ~1.5 us per poll; a grid that is dealt one workgroup at a time still ends within half a minute)
        if (__hip_atomic_load(hist + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= gridDim.x) return;
        __builtin_amdgcn_s_sleep(8);
    }
    atomicAdd(hist + 9, 1u);
}

// does this device run a 256-workgroup grid of the one-launch step as 8 XCDs x 32 co-resident workgroups?
static bool xcd_topology_ok(gvc_gpt* c) {
    if (!c->arch_xcc) return false;
    unsigned* hist = nullptr;
    unsigned h[10] = {0};
    bool ok = hipMalloc((void**)&hist, sizeof(h)) == hipSuccess && hipMemsetAsync(hist, 0, sizeof(h), c->cap_stream) == hipSuccess &&
              hipFuncSetAttribute((const void*)k_xcd_probe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->p_lds) == hipSuccess;
    if (ok) {
        // (on the context's own non-blocking stream: a launch on the legacy default stream drags every other stream's pending work in)
        hipLaunchKernelGGL(k_xcd_probe, dim3(kPG), dim3(kPThreads), c->p_lds, c->cap_stream, hist);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(c->cap_stream) == hipSuccess &&
             hipMemcpy(h, hist, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (hist) (void)hipFree(hist);
    (void)hipGetLastError();
    if (!ok || h[9] != 0 || h[8] != (unsigned)kPG) return false;
    for (int x = 0; x < 8; ++x)
        if (h[x] != (unsigned)kPG / 8) return false;
    return true;
}

// a data-path call had to allocate / synchronise the device / capture a graph (first use of a path without gvc_gpt_warmup)
static inline void note_lazy(gvc_gpt* c) { if (!c->in_warmup) c->lazy_inits += 1; }

// buffers and the per-layer pointer table; called outside stream capture (synchronous copies)
static int persist_prepare(gvc_gpt* c) {
    if (c->p_layers || !c->persist) return GVC_OK;
    note_lazy(c);
    const int d = c->dm.d_model, L = c->dm.n_layer, H = c->dm.n_head;
    std::vector<PersistLayer> t(L);
    for (int l = 0; l < L; ++l) {
        const GptLayer& ly = c->layers[l];
        PersistLayer& p = t[l];
        p.ln1_w = ly.ln1_w; p.ln1_b = ly.ln1_b; p.qkv_w = ly.qkv_w; p.qkv_b = ly.qkv_b; p.proj_w = ly.proj_w; p.proj_b = ly.proj_b;
        p.ln2_w = ly.ln2_w; p.ln2_b = ly.ln2_b; p.fc_w = ly.fc_w; p.fc_b = ly.fc_b; p.p2_w = ly.p2_w; p.p2_b = ly.p2_b;
        if (c->bf16) {        // bf16-weights context: the loader streams the row-major bf16 copies (same row order, half the bytes)
            p.qkv_w = reinterpret_cast<const float*>(ly.qkv_h); p.proj_w = reinterpret_cast<const float*>(ly.proj_h);
            p.fc_w = reinterpret_cast<const float*>(ly.fc_h); p.p2_w = reinterpret_cast<const float*>(ly.p2_h);
        }
        p.kcache = kv_layer(c, l, 0); p.vcache = kv_layer(c, l, 1);
    }
    // Anything the device refuses here (memory, the LDS opt-in, residency of one workgroup per CU) switches the one-launch step off
    // for this context -- the launch-per-phase step serves it -- instead of failing the caller's decode / generate call; the
    // buffers are allocated once (a second call after a failure finds the path off and returns before this point).
    auto unavailable = [&]() {
        for (void** p : {(void**)&c->p_gran, (void**)&c->p_epoch, (void**)&c->p_dbg})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        (void)hipGetLastError();
        c->persist = 0;
        return GVC_OK;
    };
    const size_t ngran = persist_granules(d, H);
    if (hipMalloc((void**)&c->p_gran, ngran * sizeof(pu64)) != hipSuccess || hipMemset(c->p_gran, 0, ngran * sizeof(pu64)) != hipSuccess ||
        hipMalloc((void**)&c->p_epoch, 16 * sizeof(unsigned)) != hipSuccess || hipMemset(c->p_epoch, 0, 16 * sizeof(unsigned)) != hipSuccess)
        return unavailable();
    if (getenv("GVC_PERSIST_STAMPS") && d == 1024) {        // (the stamping variant is instantiated for d_model 1024: persist_kernel)
        const size_t nb = (size_t)(20 * (L + 2) + 2 * 5 * kPG + 8 * kPG + 4 * kPG) * sizeof(unsigned long long);
        if (hipMalloc((void**)&c->p_dbg, nb) != hipSuccess || hipMemset(c->p_dbg, 0, nb) != hipSuccess) return unavailable();
    }
    // the memsets above went to the legacy default stream; the caller's stream may be a non-blocking one (no implicit ordering with it): they
    // must have landed before the first launch is enqueued.  (Device-wide sync HERE, before the context's own stream has run anything: under
    // `rocprofv3 --pmc` a device-wide sync behind the probe launch on that stream -- or the probe on the default stream -- never returned.)
    if (hipDeviceSynchronize() != hipSuccess) return unavailable();
    const int ng_hd = kPCW * 256;                       // lane-group states of the attention phase: [kPCW * 64 / (hd / 4)][hd]
    c->p_hvec = 4 * d > d + ng_hd ? 4 * d : d + ng_hd;
    c->p_ascr = 3 * c->hd + 64;
    const size_t other = ((size_t)c->p_hvec + d + c->p_ascr) * sizeof(float) + kCtlWords * sizeof(unsigned) + kPStage * sizeof(float);
    // the ring takes what the device's opt-in LDS limit leaves (160 KiB on gfx950: 8 slots)
    int dev_id = 0, lds_optin = 0;
    if (hipGetDevice(&dev_id) != hipSuccess ||
        hipDeviceGetAttribute(&lds_optin, hipDeviceAttributeSharedMemPerBlockOptin, dev_id) != hipSuccess || lds_optin <= 0)
        lds_optin = 64 * 1024;
    c->p_ring_slots = 8;
    while (c->p_ring_slots > 1 && (size_t)c->p_ring_slots * kPSlot + other > (size_t)lds_optin) c->p_ring_slots >>= 1;
    c->p_lds = (size_t)c->p_ring_slots * kPSlot + other;
    if (c->p_lds > (size_t)lds_optin || c->p_ring_slots < 4) return unavailable();
    // the XCD-local layout assumes 8 XCDs x 32 resident workgroups and HW_REG_XCC_ID: probed once per context, on a grid of the
    // step's own shape; anything else (CU masking, another partition mode, another part) keeps the device-wide hand-off
    if (d == 1024 && c->p_xl && !xcd_topology_ok(c)) c->p_xl = 0;
    if (hipFuncSetAttribute((const void*)persist_kernel(c), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->p_lds) != hipSuccess)
        return unavailable();
    // one workgroup per CU must fit (registers, LDS): otherwise the one-launch step is switched off for this context
    int per_cu = 0;
    hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, persist_kernel(c), kPThreads, c->p_lds);
    if (oe != hipSuccess || per_cu < 1) return unavailable();
    PersistLayer* dev = nullptr;
    if (hipMalloc((void**)&dev, L * sizeof(PersistLayer)) != hipSuccess ||
        hipMemcpy(dev, t.data(), L * sizeof(PersistLayer), hipMemcpyHostToDevice) != hipSuccess) {
        if (dev) (void)hipFree(dev);
        return unavailable();
    }
    c->p_layers = dev;
    return GVC_OK;
}

// run (nullable): device run flag, the grid leaves at once when it is zero; per_slot: the outputs are the per-slot parking tables
static int launch_persist(gvc_gpt* c, const int32_t* slots, const int32_t* tok_in, float* logits_out, float* latent_out,
                          int32_t* step_ctr, hipStream_t s, const int32_t* run = nullptr, int per_slot = 0) {
    GVC_REQUIRE(c->p_layers, GVC_ERR_STATE, "persistent decode step: not prepared");
    PersistArgs A;
    memset(&A, 0, sizeof(A));
    A.layers = c->p_layers; A.n_layer = c->dm.n_layer; A.d = c->dm.d_model; A.n_head = c->dm.n_head; A.head_dim = c->hd;
    A.vocab = c->dm.vocab; A.max_seq = c->dm.max_seq; A.max_mel_pos = c->dm.max_mel_pos;
    A.mel_emb = c->mel_emb; A.mel_pos = c->mel_pos; A.lnf_w = c->lnf_w; A.lnf_b = c->lnf_b; A.fn_w = c->fn_w; A.fn_b = c->fn_b;
    A.head_w = c->head_w; A.head_b = c->head_b; A.slots = slots; A.tok_in = tok_in; A.st = c->st;
    A.logits_out = logits_out; A.latent_out = latent_out; A.step_ctr = step_ctr; A.advance = 1;
    A.gran = c->p_gran; A.epoch = c->p_epoch; A.err = c->seam_err_dev; A.ring_slots = c->p_ring_slots; A.ascr_floats = c->p_ascr; A.hvec_floats = c->p_hvec;
    A.dbg = c->p_dbg;
    A.run = run; A.per_slot = per_slot; A.exec_ctr = c->exec_ctr;
    if (c->bf16) A.head_w = reinterpret_cast<const float*>(c->head_h);
    void* kargs[] = {&A};
    GVC_CHECK_HIP(hipLaunchKernel((const void*)persist_kernel(c), dim3(persist_test_grid()), dim3(kPThreads), kargs, c->p_lds, s));
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}


// ---------------------------------------------------------------------------------------------
// one-launch block stack for 2..16 rows (persist_rows.h)
// ---------------------------------------------------------------------------------------------
static bool rows_persist_ok(const gvc_gpt* c, int rows, const int32_t* base_len) {
    return c->persist && c->persist_rows && c->r_ready >= 0 && base_len && rows >= c->persist_rows_min && rows <= kRMaxRows &&
           c->dm.d_model == kRD && (c->hd == 64 || c->hd == 128 || c->hd == 256) && c->dm.n_head * c->hd == kRD && c->dm.n_layer % 2 == 0 &&
           c->n_cu >= kPG;
}

// key chunks per (row, head) for a call whose longest context reaches `keys` cached positions
static int rows_persist_chunks(const gvc_gpt* c, int rows, int keys) {
    (void)keys;                              // (the kernel picks the split from the contexts it finds; this is the bound)
    int nch = kRMaxChunks;
    const int R = rows <= 8 ? 8 : 16;
    while (nch > 1 && R * (kRD / kRHD) * nch > kPG) nch >>= 1;       // (phase B's workgroups: one per row, 256-dim super-head and key chunk)
    return nch;
}

// the instantiation for this context: padded rows (8 / 16), weight / cache storage, real head_dim
typedef void (*rows_fn)(const RowsArgs);
template <int HDR>
static const void* rows_kernel_hd(const gvc_gpt* c, int R) {
    rows_fn f;
    if (c->act_bf16) f = R == 8 ? (rows_fn)k_rows_persist_b16<8, HDR> : (rows_fn)k_rows_persist_b16<16, HDR>;
    else if (c->kv_bf16) f = R == 8 ? (rows_fn)k_rows_persist<8, 1, 1, HDR> : (rows_fn)k_rows_persist<16, 1, 1, HDR>;
    else if (c->bf16) f = R == 8 ? (rows_fn)k_rows_persist<8, 1, 0, HDR> : (rows_fn)k_rows_persist<16, 1, 0, HDR>;
    else f = R == 8 ? (rows_fn)k_rows_persist<8, 0, 0, HDR> : (rows_fn)k_rows_persist<16, 0, 0, HDR>;
    return (const void*)f;
}
static const void* rows_kernel(const gvc_gpt* c, int R) {
    return c->hd == 64 ? rows_kernel_hd<64>(c, R) : c->hd == 128 ? rows_kernel_hd<128>(c, R) : rows_kernel_hd<256>(c, R);
}

static void rows_persist_release(gvc_gpt* c) {
    for (void** p : {(void**)&c->r_layers, (void**)&c->r_wpack, (void**)&c->r_bufs, (void**)&c->r_dbg, (void**)&c->r_lnfold})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    (void)hipGetLastError();
    c->r_ready = -1;
}

// packed weight copy, per-layer table, hand-off buffers; called outside stream capture (synchronous).  Anything the device
// refuses (memory, LDS opt-in, residency) switches the path off for this context instead of failing the call.
static void rows_pack_layer(gvc_gpt* c, int l) {
    const GptLayer& ly = c->layers[l];
    const int wsh = c->bf16 ? 1 : 0;
    float* dst = reinterpret_cast<float*>(reinterpret_cast<char*>(c->r_wpack) + (size_t)l * kPG * (kRWgLayerBytes >> wsh));
    if (c->act_bf16) {
        // bf16-activation mode: octet-major bf16 groups with the LayerNorm gains folded into c_attn / c_fc, and the constants that go with them
        const int d = kRD;
        float* f = c->r_lnfold + (size_t)l * 14 * d;
        hipLaunchKernelGGL(k_pack_rows_weights_b16, dim3(2048), dim3(256), 0, 0, reinterpret_cast<pu32x4*>(dst), (const float*)ly.qkv_w,
                           (const float*)ly.proj_w, (const float*)ly.fc_w, (const float*)ly.p2_w, (const float*)ly.ln1_w, (const float*)ly.ln2_w);
        hipLaunchKernelGGL(k_rows_ln_fold_b16, dim3(3 * d / 4), dim3(256), 0, 0, f, f + 3 * d, (const float*)ly.qkv_w, (const float*)ly.ln1_w,
                           (const float*)ly.ln1_b, (const float*)ly.qkv_b, 3 * d, d);
        hipLaunchKernelGGL(k_rows_ln_fold_b16, dim3(4 * d / 4), dim3(256), 0, 0, f + 6 * d, f + 10 * d, (const float*)ly.fc_w, (const float*)ly.ln2_w,
                           (const float*)ly.ln2_b, (const float*)ly.fc_b, 4 * d, d);
        return;
    }
    if (wsh) hipLaunchKernelGGL(k_pack_rows_weights<1>, dim3(2048), dim3(256), 0, 0, dst, (const float*)ly.qkv_w, (const float*)ly.proj_w,
                                (const float*)ly.fc_w, (const float*)ly.p2_w);
    else hipLaunchKernelGGL(k_pack_rows_weights<0>, dim3(2048), dim3(256), 0, 0, dst, (const float*)ly.qkv_w, (const float*)ly.proj_w,
                            (const float*)ly.fc_w, (const float*)ly.p2_w);
    // LayerNorm folded into per-output-row constants (persist_rows.h, phases A / D): S_r = sum_k W_rk g_k, C_r = sum_k W_rk b_k + bias_r
    const int d = kRD;
    float* f = c->r_lnfold + (size_t)l * 14 * d;
    hipLaunchKernelGGL(k_rows_ln_fold, dim3(3 * d / 4), dim3(256), 0, 0, f, f + 3 * d, (const float*)ly.qkv_w, (const float*)ly.ln1_w,
                       (const float*)ly.ln1_b, (const float*)ly.qkv_b, 3 * d, d);
    hipLaunchKernelGGL(k_rows_ln_fold, dim3(4 * d / 4), dim3(256), 0, 0, f + 6 * d, f + 10 * d, (const float*)ly.fc_w, (const float*)ly.ln2_w,
                       (const float*)ly.ln2_b, (const float*)ly.fc_b, 4 * d, d);
}

static int rows_persist_prepare(gvc_gpt* c) {
    if (c->r_ready == 1 && !c->r_dirty.empty()) {
        // weights re-bound since the pack was built (a second GptEngine.bind on the same context): the packed copy of those layers is
        // stale.  Rare and outside capture: wait for the bind stream's transposes, repack, wait again.
        bool any = false;
        for (char f : c->r_dirty) any = any || f;
        if (any) {
            note_lazy(c);
            GVC_CHECK_HIP(hipDeviceSynchronize());
            for (int l = 0; l < c->dm.n_layer; ++l)
                if (c->r_dirty[l]) rows_pack_layer(c, l);
            GVC_CHECK_HIP(hipGetLastError());
            GVC_CHECK_HIP(hipDeviceSynchronize());
            std::fill(c->r_dirty.begin(), c->r_dirty.end(), 0);
        }
    }
    if (c->r_ready != 0) return GVC_OK;
    note_lazy(c);
    const int L = c->dm.n_layer;
    c->r_lds = (size_t)8 * kPSlot + ((size_t)kPCW * 4 * kRMaxRows * 4 + 2 * kPCW * 16 + 3 * kRMaxRows * 4 + kPCW * 64 * 4 + 256 + 64 + kPCW * 256) * sizeof(float) +
               kCtlWords * sizeof(unsigned);
    int per_cu = 0;
    const void* kern[2] = {rows_kernel(c, 8), rows_kernel(c, 16)};      // the two instantiations (8 / 16 padded rows) of this context's storage types and head_dim
    const int wsh = c->bf16 ? 1 : 0;
    if (hipFuncSetAttribute(kern[0], hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->r_lds) != hipSuccess ||
        hipFuncSetAttribute(kern[1], hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->r_lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern[1], kPThreads, c->r_lds) != hipSuccess || per_cu < 1 ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern[0], kPThreads, c->r_lds) != hipSuccess || per_cu < 1 ||
        hipMalloc((void**)&c->r_wpack, (size_t)L * kPG * (kRWgLayerBytes >> wsh)) != hipSuccess ||
        hipMalloc((void**)&c->r_bufs, c->act_bf16 ? rows_b16_buf_bytes() : rows_buf_bytes()) != hipSuccess ||
        hipMalloc((void**)&c->r_lnfold, (size_t)L * 14 * kRD * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&c->r_layers, L * sizeof(RowsLayer)) != hipSuccess) {
        rows_persist_release(c);
        return GVC_OK;
    }
    std::vector<RowsLayer> t(L);
    for (int l = 0; l < L; ++l) {
        const GptLayer& ly = c->layers[l];
        RowsLayer& p = t[l];
        p.ln1_w = ly.ln1_w; p.ln1_b = ly.ln1_b; p.qkv_b = ly.qkv_b; p.proj_b = ly.proj_b; p.ln2_w = ly.ln2_w; p.ln2_b = ly.ln2_b;
        p.fc_b = ly.fc_b; p.p2_b = ly.p2_b; p.kcache = kv_layer(c, l, 0); p.vcache = kv_layer(c, l, 1);
        p.lnS_a = c->r_lnfold + (size_t)l * 14 * kRD; p.lnC_a = p.lnS_a + 3 * kRD; p.lnS_d = p.lnS_a + 6 * kRD; p.lnC_d = p.lnS_a + 10 * kRD;
        rows_pack_layer(c, l);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpy(c->r_layers, t.data(), L * sizeof(RowsLayer), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(c->r_bufs, 0xff, c->act_bf16 ? rows_b16_buf_bytes() : rows_buf_bytes()) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        rows_persist_release(c);
        return GVC_OK;
    }
    if (getenv("GVC_PERSIST_STAMPS")) {        // diagnostics only: a failed allocation just leaves the stamps off
        const size_t nb = (size_t)(40 * (L + 2) + 8 * 5 * kPG) * sizeof(unsigned long long);
        if (hipMalloc((void**)&c->r_dbg, nb) != hipSuccess || hipMemset(c->r_dbg, 0, nb) != hipSuccess) {
            if (c->r_dbg) (void)hipFree(c->r_dbg);
            c->r_dbg = nullptr;
            (void)hipGetLastError();
        }
    }
    c->r_dirty.assign(L, 0);
    c->r_ready = 1;
    return GVC_OK;
}

static int launch_rows_persist(gvc_gpt* c, const int32_t* slots, int rows, int T, const int32_t* base_len, int nch, hipStream_t s,
                               const int32_t* tok_in = nullptr) {
    RowsArgs A;
    memset(&A, 0, sizeof(A));
    A.layers = c->r_layers; A.wpack = reinterpret_cast<const char*>(c->r_wpack); A.n_layer = c->dm.n_layer; A.n_head = c->dm.n_head;
    A.max_seq = c->dm.max_seq; A.rows = rows; A.T = T; A.slots = slots; A.base_len = base_len; A.x = c->x; A.bufs = c->r_bufs;
    A.err = c->seam_err_dev; A.ring_slots = 8; A.nchunks = nch; A.dbg = c->r_dbg;
    A.tok_in = tok_in; A.mel_emb = c->mel_emb; A.mel_pos = c->mel_pos; A.mel_pos_idx = c->st.mel_pos; A.vocab = c->dm.vocab;
    // keys of a (row, head) over 2 / 4 workgroups: 8 rows from 80 / 160 cached positions (one 80-key pass per workgroup; 744 vs 766 us
    // per step at 48-112 keys, 815 vs 827 at 110-250), 16 rows from 128 / 288 (their chunk merge gathers 64 KB per chunk: 1068 vs 1104 us)
    A.split1 = rows <= 8 ? 80 : 128;
    A.split2 = rows <= 8 ? 160 : 288;
    void* kargs[] = {&A};
    GVC_CHECK_HIP(hipLaunchKernel(rows_kernel(c, rows <= 8 ? 8 : 16), dim3(persist_test_grid()), dim3(kPThreads), kargs, c->r_lds, s));
    GVC_LAUNCH_CHECK();
    c->r_launches += 1;
    return GVC_OK;
}

static int decode_group(gvc_gpt* c, const int32_t* slots, int B, int row0, const int32_t* tok_in, float* logits_out,
                        float* latent_out, int32_t* step_ctr, hipStream_t s, bool fused = false) {
    const int d = c->dm.d_model;
    int rc;
    float* qb = c->q + (size_t)row0 * d;
    float* hb = c->h + (size_t)row0 * 4 * d;
    float* pb = c->part + (size_t)row0 * c->dm.n_head * kAttnChunks * (c->hd + 4);
    for (int l = 0; l < c->dm.n_layer; ++l) {
        const GptLayer& ly = c->layers[l];
        GemvArgs A = base_args(c, slots, row0);
        A.Wt = ly.qkv_w; A.Wt16 = ly.qkv_h; A.bias = ly.qkv_b; A.N = 3 * d; A.K = d;
        A.ln_w = ly.ln1_w; A.ln_b = ly.ln1_b; A.embed = l == 0; A.tok_in = tok_in;
        A.out = qb;
        A.kcache = kv_layer(c, l, 0);
        A.vcache = kv_layer(c, l, 1);
        if (!prof_skip(c, 0) && (rc = launch_gemv<PRO_LN, EPI_QKV>(c, A, B, s))) return rc;

        if (fused) {
            // attention + head-split c_proj in one launch; c_fc's prologue sums the per-head partials
            AttnProjArgs F;
            memset(&F, 0, sizeof(F));
            F.q = qb; F.kcache = A.kcache; F.vcache = A.vcache; F.slots = slots; F.seq_len = c->st.seq_len;
            F.max_seq = c->dm.max_seq; F.n_head = c->dm.n_head; F.d = d; F.scale = 1.0f / sqrtf((float)c->hd);
            F.Wp = ly.proj_w; F.part2 = c->part2 + (size_t)row0 * c->dm.n_head * d;
            if (!prof_skip(c, 1)) {
                if (c->kv_bf16) hipLaunchKernelGGL((k_attn_proj<256, 1>), dim3(d / 16, c->dm.n_head), dim3(512), 0, s, F);
                else hipLaunchKernelGGL((k_attn_proj<256, 0>), dim3(d / 16, c->dm.n_head), dim3(512), 0, s, F);
                GVC_LAUNCH_CHECK();
            }
            A = base_args(c, slots, row0);
            A.Wt = ly.fc_w; A.Wt16 = ly.fc_h; A.bias = ly.fc_b; A.N = 4 * d; A.K = d; A.ln_w = ly.ln2_w; A.ln_b = ly.ln2_b; A.out = hb;
            A.part2 = F.part2; A.pbias = ly.proj_b; A.x2 = c->x2 + (size_t)row0 * d;
            if (!prof_skip(c, 3) && (rc = launch_gemv<PRO_LN_SUM, EPI_GELU>(c, A, B, s))) return rc;
            A = base_args(c, slots, row0);
            A.Wt = ly.p2_w; A.Wt16 = ly.p2_h; A.bias = ly.p2_b; A.N = d; A.K = 4 * d; A.in = hb; A.xres = c->x2 + (size_t)row0 * d;
            if (!prof_skip(c, 4) && (rc = launch_gemv<PRO_COPY, EPI_RESID>(c, A, B, s))) return rc;
            continue;
        }
        AttnArgs T = gpt_attn_args(c, l, slots);
        T.q = qb; T.T = 1; T.base_len = c->st.seq_len; T.out = pb;
        if (!prof_skip(c, 1) && (rc = launch_attention(c, T, kAttnChunks, B, false, s))) return rc;

        A = base_args(c, slots, row0);
        A.Wt = ly.proj_w; A.Wt16 = ly.proj_h; A.bias = ly.proj_b; A.N = d; A.K = d; A.in = pb;
        if (!prof_skip(c, 2) && (rc = launch_gemv<PRO_MERGE, EPI_RESID>(c, A, B, s))) return rc;

        A = base_args(c, slots, row0);
        A.Wt = ly.fc_w; A.Wt16 = ly.fc_h; A.bias = ly.fc_b; A.N = 4 * d; A.K = d; A.ln_w = ly.ln2_w; A.ln_b = ly.ln2_b; A.out = hb;
        if (!prof_skip(c, 3) && (rc = launch_gemv<PRO_LN, EPI_GELU>(c, A, B, s))) return rc;

        A = base_args(c, slots, row0);
        A.Wt = ly.p2_w; A.Wt16 = ly.p2_h; A.bias = ly.p2_b; A.N = d; A.K = 4 * d; A.in = hb;
        if (!prof_skip(c, 4) && (rc = launch_gemv<PRO_COPY, EPI_RESID>(c, A, B, s))) return rc;
    }
    GemvArgs A = base_args(c, slots, row0);
    A.Wt = c->head_w; A.Wt16 = c->head_h; A.bias = c->head_b; A.N = c->dm.vocab; A.K = d;
    A.ln_w = c->lnf_w; A.ln_b = c->lnf_b; A.ln2_w = c->fn_w; A.ln2_b = c->fn_b;
    A.out = logits_out; A.latent_out = latent_out; A.advance = 1; A.step_ctr = step_ctr;
    if (prof_skip(c, 5)) return GVC_OK;
    return launch_gemv<PRO_LN2X, EPI_LOGITS>(c, A, B, s);
}

static int run_rows(gvc_gpt* c, const int32_t* slots, int B, int T, hipStream_t s, const int32_t* base_len = nullptr, int key_chunks = 1);

// double LayerNorm (ln_f, final_norm) of row (b * stride + off) of x -> latent[b]  (the head of a model wider than the GEMV kernels take)
__global__ void k_head_ln(const float* x, int stride, int off, float* latent, int B, int d, const float* w1, const float* b1, const float* w2,
                          const float* b2) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* in = x + ((size_t)b * stride + off) * d;
    float* y = latent + (size_t)b * d;
    const float inv_d = 1.0f / (float)d;
    for (int pass = 0; pass < 2; ++pass) {
        const float* gw = pass == 0 ? w1 : w2;
        const float* gb = pass == 0 ? b1 : b2;
        float s = 0.f;
        for (int k = lane * 4; k < d; k += 256) { const float4 v = *reinterpret_cast<const float4*>(in + k); s += (v.x + v.y) + (v.z + v.w); }
        const float mean = wave_sum(s) * inv_d;
        float q = 0.f;
        for (int k = lane * 4; k < d; k += 256) {
            const float4 v = *reinterpret_cast<const float4*>(in + k);
            const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_d + 1e-5f);
        for (int k = lane * 4; k < d; k += 256) {
            float4 v = *reinterpret_cast<const float4*>(in + k);
            const float4 g = *reinterpret_cast<const float4*>(gw + k), c = *reinterpret_cast<const float4*>(gb + k);
            v.x = (v.x - mean) * rstd * g.x + c.x; v.y = (v.y - mean) * rstd * g.y + c.y;
            v.z = (v.z - mean) * rstd * g.z + c.z; v.w = (v.w - mean) * rstd * g.w + c.w;
            *reinterpret_cast<float4*>(y + k) = v;
        }
        in = y;
    }
}

// what EPI_LOGITS does behind the logits: the slots' caches grew by one position
__global__ void k_head_advance(GptState st, const int32_t* slots, int B, int max_seq, int max_mel_pos, int32_t* step_ctr, int* err) {
    const int t = threadIdx.x;
    if (t < B) {
        const int slot = slots[t];
        if (st.seq_len[slot] < max_seq - 1) st.seq_len[slot] += 1;
        else if (err) *err = 950;
        if (st.mel_pos[slot] < max_mel_pos - 1) st.mel_pos[slot] += 1;
        else if (err) *err = 951;
    }
    if (step_ctr && t == 0) *step_ctr += 1;
}

// gpt_inference.py:18,111-112 for the rows (b * x_stride + x_off) of x: latent = final_norm(ln_f(h)), logits = mel_head(latent).  Up to
// d_model 1024 ONE GEMV launch with the two LayerNorms in its prologue (8 streams per launch); wider models: a LayerNorm launch + a GEMM
static int launch_head(gvc_gpt* c, const int32_t* slots, int B, int row0, const float* x, int x_stride, int x_off, float* logits_out,
                       float* latent_out, int advance, int32_t* step_ctr, hipStream_t s) {
    const int d = c->dm.d_model;
    int rc;
    if (d <= 1024) {
        for (int g = 0; g < B; g += 8) {
            const int Bg = B - g < 8 ? B - g : 8;
            GemvArgs A = base_args(c, slots + g, row0 + g);
            A.x = const_cast<float*>(x) + (size_t)g * x_stride * d; A.x_stride = x_stride; A.x_off = x_off;
            A.Wt = c->head_w; A.Wt16 = c->head_h; A.bias = c->head_b; A.N = c->dm.vocab; A.K = d;
            A.ln_w = c->lnf_w; A.ln_b = c->lnf_b; A.ln2_w = c->fn_w; A.ln2_b = c->fn_b;
            A.out = logits_out + (size_t)g * c->dm.vocab; A.latent_out = latent_out + (size_t)g * d; A.advance = advance;
            A.step_ctr = g + 8 >= B ? step_ctr : nullptr;
            if ((rc = launch_gemv<PRO_LN2X, EPI_LOGITS>(c, A, Bg, s))) return rc;
        }
        return GVC_OK;
    }
    hipLaunchKernelGGL(k_head_ln, dim3(cdiv(B, 4)), dim3(256), 0, s, x, x_stride, x_off, latent_out, B, d, c->lnf_w, c->lnf_b, c->fn_w, c->fn_b);
    GVC_LAUNCH_CHECK();
    GemmArgs G;
    memset(&G, 0, sizeof(G));
    G.A = latent_out; G.lda = d; G.Wt = c->head_w; G.ldw = d; G.C = logits_out; G.ldc = c->dm.vocab; G.M = B; G.N = c->dm.vocab; G.K = d;
    G.work = c->work; G.e.bias = c->head_b;
    if ((rc = launch_gemm_cap(G, 1, c->work_cap, s))) return rc;
    if (advance || step_ctr) {
        hipLaunchKernelGGL(k_head_advance, dim3(1), dim3(128), 0, s, c->st, slots, advance ? B : 0, c->dm.max_seq, c->dm.max_mel_pos, step_ctr,
                           c->seam_err_dev);
        GVC_LAUNCH_CHECK();
    }
    return GVC_OK;
}

// Batched decode step on the MFMA path: the B new rows go through the skinny fragment-major GEMMs (weights streamed
// once for up to 128 streams) instead of the 8-stream GEMV groups.  Same arithmetic as a prefill of one row per stream
// appended at each slot's cached length.
static bool rows_decode_ok(const gvc_gpt* c, int B) {
    if (c->r_ready >= 0 && rows_persist_ok(c, B, c->st.seq_len)) return true;       // served by the one-launch rows step (from 2 streams)
    if (c->mfma_b16 && B >= 2 && B <= c->dm.max_rows) return true;                   // weight_dtype 4: every multi-row pass, the same rounding points
    const bool wide = c->dm.d_model > 1024;       // no GEMV path above 1024: every batch decodes as rows
    return (wide || (c->rows_decode_min > 0 && B >= c->rows_decode_min)) && B <= 128 && c->skinny_prefill && c->wfm &&
           c->dm.d_model % 256 == 0 && (long long)4 * B * c->dm.d_model <= c->work_cap / 2 && B <= c->dm.max_rows;
}

static int decode_rows(gvc_gpt* c, const int32_t* slots, int B, const int32_t* tok_in, float* logits_out, float* latent_out,
                       int32_t* step_ctr, hipStream_t s, int key_chunks = 1) {
    const int d = c->dm.d_model;
    int rc;
    if (c->r_ready == 1 && rows_persist_ok(c, B, c->st.seq_len)) {        // the one-launch rows step builds its input rows itself
        if ((rc = launch_rows_persist(c, slots, B, 1, c->st.seq_len, rows_persist_chunks(c, B, c->rows_keys_hint), s, tok_in))) return rc;
    } else {
        hipLaunchKernelGGL(k_embed_decode_rows, dim3(B), dim3(256), 0, s, c->x, tok_in, slots, c->st, c->mel_emb, c->mel_pos, d, c->dm.vocab);
        GVC_LAUNCH_CHECK();
        if ((rc = run_rows(c, slots, B, 1, s, c->st.seq_len, key_chunks))) return rc;
    }
    return launch_head(c, slots, B, 0, c->x, 1, 0, logits_out, latent_out, 1, step_ctr, s);
}

// Re-initialises the hand-off buffers of both one-launch steps (the device is idle); the first HIP error, for the caller to judge.
static hipError_t reset_handoffs(gvc_gpt* c) {
    const hipError_t e_bufs = c->r_bufs ? hipMemset(c->r_bufs, 0xff, c->act_bf16 ? rows_b16_buf_bytes() : rows_buf_bytes()) : hipSuccess;
    // (the step epoch p_epoch[0] stays MONOTONIC: granule tags are (epoch + 1, layer, phase) and nothing zeroes the granules, so an epoch
    //  that started over could accept a stale granule of the timed-out call; only the arrival counter and the per-XCD ranks are cleared)
    const hipError_t e_epoch = c->p_epoch ? hipMemset(c->p_epoch + 1, 0, 15 * sizeof(unsigned)) : hipSuccess;
    return e_bufs != hipSuccess ? e_bufs : e_epoch;
}

// Deferred decodes of these slots, now: one conditional one-stream step per row, token from the slot's pending entry, logits and latent
// to the slot's parked rows -- afterwards every slot looks as the eager order leaves it.  Rows with nothing pending cost an early exit.
// Nothing is enqueued in a context where no deferring call has run.
static int flush_pending(gvc_gpt* c, const int32_t* slots, int B, hipStream_t s) {
    if (!c->defer_seen || !c->persist || !c->p_layers) return GVC_OK;
    GVC_REQUIRE(slots && B >= 1 && B <= c->dm.max_slots, GVC_ERR_ARG, "flush of deferred decodes: %d rows outside [1,%d]", B, c->dm.max_slots);
    hipLaunchKernelGGL(k_flush_begin, dim3(1), dim3(64), 0, s, slots, B, c->st.pending, c->flush_tok, c->flush_run);
    GVC_LAUNCH_CHECK();
    int rc = GVC_OK;
    for (int b = 0; b < B && rc == GVC_OK; ++b)
        rc = launch_persist(c, slots + b, c->flush_tok + b, c->slot_logits, c->slot_latent, nullptr, s, c->flush_run + b, 1);
    return rc;
}

static int decode_step(gvc_gpt* c, const int32_t* slots, int B, const int32_t* tok_in, float* logits_out, float* latent_out,
                       int32_t* step_ctr, hipStream_t s, bool fused, int key_chunks);

// The context has just left the one-launch step (hand-off time-out; the device is idle): the pending tokens are decoded once on the
// launch-per-phase path, slot by slot from a synchronous read of the pending table, so that the eager order that serves the context
// from here on finds every slot complete.  Rare; errors are left to the next call's own checks.
static void settle_pending(gvc_gpt* c) {
    if (!c->defer_seen) return;
    c->defer_seen = 0;
    const int S = c->dm.max_slots;
    std::vector<int32_t> pend((size_t)S, -1);
    if (hipMemcpy(pend.data(), c->st.pending, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int32_t slot = 0; slot < S; ++slot) {
        if (pend[slot] < 0) continue;
        if (hipMemcpy(c->flush_slot, &slot, sizeof(slot), hipMemcpyHostToDevice) != hipSuccess) break;
        if (decode_step(c, c->flush_slot, 1, c->st.pending + slot, c->slot_logits + (size_t)slot * c->dm.vocab,
                        c->slot_latent + (size_t)slot * c->dm.d_model, nullptr, nullptr, false, 1) != GVC_OK) break;
        if (hipDeviceSynchronize() != hipSuccess) break;
    }
    (void)hipMemset(c->st.pending, 0xff, (size_t)S * sizeof(int32_t));
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
}

// weight_dtype 4: the FB16 bf16 copies of the four matrices of every layer bound since the last call, with the LayerNorm gains folded
// into c_attn / c_fc, and the fold constants.  Outside stream capture (every entry point passes here before it enqueues anything):
// waits for the bind stream, packs, waits again.  After a bind + gvc_gpt_warmup no data-path call packs, allocates or synchronises.
static unsigned short* b16_w(const gvc_gpt* c, int l, int which) {
    const size_t d = c->dm.d_model, off[4] = {0, 3 * d * d, 4 * d * d, 8 * d * d};
    return c->wb16 + (size_t)l * 12 * d * d + off[which];
}
static int b16_prepare(gvc_gpt* c) {
    if (!c->mfma_b16 || !c->b16_any_dirty) return GVC_OK;
    note_lazy(c);
    const int d = c->dm.d_model;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    int rc;
    for (int l = 0; l < c->dm.n_layer; ++l) {
        if (!c->b16_dirty[l]) continue;
        const GptLayer& ly = c->layers[l];
        float* f = c->b16_fold + (size_t)l * 14 * d;
        if ((rc = launch_to_fb16(ly.qkv_w, b16_w(c, l, 0), 3 * d, d, ly.ln1_w, 0)) || (rc = launch_to_fb16(ly.proj_w, b16_w(c, l, 1), d, d, nullptr, 0)) ||
            (rc = launch_to_fb16(ly.fc_w, b16_w(c, l, 2), 4 * d, d, ly.ln2_w, 0)) || (rc = launch_to_fb16(ly.p2_w, b16_w(c, l, 3), d, 4 * d, nullptr, 0)))
            return rc;
        hipLaunchKernelGGL(k_rows_ln_fold_b16, dim3(3 * d / 4), dim3(256), 0, 0, f, f + 3 * d, (const float*)ly.qkv_w, (const float*)ly.ln1_w,
                           (const float*)ly.ln1_b, (const float*)ly.qkv_b, 3 * d, d);
        hipLaunchKernelGGL(k_rows_ln_fold_b16, dim3(4 * d / 4), dim3(256), 0, 0, f + 6 * d, f + 10 * d, (const float*)ly.fc_w, (const float*)ly.ln2_w,
                           (const float*)ly.ln2_b, (const float*)ly.fc_b, 4 * d, d);
        GVC_LAUNCH_CHECK();
    }
    GVC_CHECK_HIP(hipDeviceSynchronize());
    std::fill(c->b16_dirty.begin(), c->b16_dirty.end(), 0);
    c->b16_any_dirty = 0;
    return GVC_OK;
}

static int check_ready(gvc_gpt* c) {
    GVC_REQUIRE(c, GVC_ERR_ARG, "null context");
    const int dev_err = c->seam_err_host ? *(volatile int*)c->seam_err_host : 0;
    GVC_REQUIRE(dev_err != 950 && dev_err != 951, GVC_ERR_STATE,
                "a decode step ran with a full %s (max_seq %d, max_mel_pos %d): its position was not advanced; reset the slot",
                dev_err == 950 ? "KV cache" : "mel position table", c->dm.max_seq, c->dm.max_mel_pos);
    if (dev_err != 0) {
        // A hand-off of a one-launch step timed out: not all 256 workgroups were resident (another process or stream held CUs).
        // The call that timed out has produced garbage and this call reports it ONCE; the context itself stays usable -- both
        // one-launch steps are switched off, the captured step graphs (which contain them) are dropped, the hand-off buffers are
        // re-initialised -- and every later call runs on the launch-per-phase paths.
        (void)hipDeviceSynchronize();
        c->persist = 0;
        drop_graphs(c);
        (void)reset_handoffs(c);
        *c->seam_err_host = 0;
        settle_pending(c);
        c->fallbacks += 1;
        set_error("an in-kernel hand-off of a one-launch decode step timed out (code %d: were all 256 workgroups resident?); the outputs "
                  "of the previous decode / generate / cached-prefill call are invalid.  The context has switched to the launch-per-phase "
                  "paths and stays usable: reset the affected slots and repeat the call", dev_err);
        return GVC_ERR_TIMEOUT;
    }
    GVC_REQUIRE(gvc_gpt_missing_weights(c) == 0, GVC_ERR_STATE, "%d GPT weight tensors are not bound",
                gvc_gpt_missing_weights(c));
    return b16_prepare(c);
}

// One decode step over the B rows of a slot table, eager or under capture: the one-stream one-launch step, else the rows path, else
// GEMV groups of 8 streams (the nullable step counter goes to the last group only).  The one-launch steps are prepared by the caller.
static int decode_step(gvc_gpt* c, const int32_t* slots, int B, const int32_t* tok_in, float* logits_out, float* latent_out,
                       int32_t* step_ctr, hipStream_t s, bool fused, int key_chunks) {
    if (persist_ok(c, B)) return launch_persist(c, slots, tok_in, logits_out, latent_out, step_ctr, s);
    if (rows_decode_ok(c, B)) return decode_rows(c, slots, B, tok_in, logits_out, latent_out, step_ctr, s, key_chunks);
    int rc = GVC_OK;
    for (int g = 0; g < B && rc == GVC_OK; g += 8) {
        const int Bg = B - g < 8 ? B - g : 8;
        const bool last = g + 8 >= B;
        rc = decode_group(c, slots + g, Bg, g, tok_in + g, logits_out + (size_t)g * c->dm.vocab, latent_out + (size_t)g * c->dm.d_model,
                          last ? step_ctr : nullptr, s, fused);
    }
    return rc;
}

extern "C" int gvc_gpt_decode_step(gvc_gpt* c, const int32_t* slots, int32_t B, const int32_t* tok_in,
                                   float* logits_out, float* latent_out, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots, GVC_ERR_ARG, "decode_step: B=%d outside [1,%d]", B, c->dm.max_slots);
    hipStream_t s = (hipStream_t)sv;
    if (persist_ok(c, B) && (rc = persist_prepare(c))) return rc;
    if (!persist_ok(c, B)) {
        if (rows_persist_ok(c, B, c->st.seq_len) && (rc = rows_persist_prepare(c))) return rc;
        c->rows_keys_hint = c->dm.max_seq;            // (no bound from the caller: the key split for the longest possible context)
    }
    if ((rc = flush_pending(c, slots, B, s))) return rc;
    return decode_step(c, slots, B, tok_in, logits_out, latent_out, nullptr, s, false, 1);
}

extern "C" int gvc_gpt_reset_slots(gvc_gpt* c, const int32_t* slots, int32_t B, gvc_stream sv) {
    GVC_REQUIRE(c && slots && B >= 1, GVC_ERR_ARG, "reset_slots: bad argument");
    if (c->seam_err_host && (*c->seam_err_host == 950 || *c->seam_err_host == 951)) *c->seam_err_host = 0;     // overflow acknowledged
    hipLaunchKernelGGL(k_set_state, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)sv, c->st, slots, B, 0, 0);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

extern "C" int gvc_gpt_kv_fanout(gvc_gpt* c, const int32_t* src_slots, const int32_t* dst_slots, int32_t n, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(src_slots && dst_slots && n >= 1 && n <= c->dm.max_slots, GVC_ERR_ARG, "kv_fanout: n=%d outside [1,%d] or a null slot list",
                n, c->dm.max_slots);
    return launch_kv_fanout(src_slots, dst_slots, n, c->kv, c->dm.n_layer, c->dm.n_head, c->dm.max_seq, c->hd, c->dm.max_slots,
                            c->kv_bf16 ? 2 : 4, c->st.seq_len, c->st.mel_pos, c->slot_logits, c->dm.vocab, c->slot_latent, c->dm.d_model,
                            c->st.pending, (hipStream_t)sv);
}

extern "C" int gvc_gpt_sequence_logprobs(gvc_gpt* c, const int32_t* tokens, int32_t tokens_stride, const float* latents, int32_t R, int32_t n,
                                         int32_t stop_tok, double* logprob_out, int32_t* length_out, float* token_logprobs_out,
                                         gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(tokens && latents && logprob_out && length_out && R >= 1 && n >= 1 && tokens_stride >= n, GVC_ERR_ARG,
                "sequence_logprobs: bad argument (R %d, n %d, tokens_stride %d)", R, n, tokens_stride);
    return launch_sequence_logprobs(latents, tokens, tokens_stride, R, n, c->dm.d_model, c->dm.vocab, stop_tok, c->head_w, c->head_b, c->work,
                                    c->work_cap, logprob_out, length_out, token_logprobs_out, (hipStream_t)sv);
}

extern "C" int gvc_gpt_prefix_embeddings(gvc_gpt* c, const float* cond, int32_t n_cond, const int32_t* codes,
                                         int32_t B, int32_t Tc, int32_t start_text, int32_t stop_text, float* out,
                                         gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(Tc + 2 <= c->dm.max_text_pos, GVC_ERR_ARG, "prefix: %d content codes exceed text positions", Tc);
    const int P = n_cond + Tc + 2;
    hipLaunchKernelGGL(k_prefix_rows, dim3(B * P), dim3(256), 0, (hipStream_t)sv, out, cond, n_cond, codes, B, Tc,
                       c->dm.d_model, c->text_emb, c->text_pos, start_text, stop_text);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// block stack over B*T rows already in c->x; K/V of every row go to the slots' cache (positions 0..T-1, or
// base_len[slot] + 0..T-1 when the rows continue cached sequences: the batched decode step is T = 1).
// rows <= 128 (a streaming prefill): skinny MFMA GEMMs; the N = d projections are K-split over 4 workgroup
// rows and their raw partial sums are folded into the NEXT LayerNorm launch (k_ln_sum_rows), so a layer is
// 7 launches.  Larger row counts (batched offline prefill, latent re-pass) use the tiled GEMM.
// weight_dtype 4: the block stack of run_rows with the four projections of every layer on bf16 matrix cores and the rounding points of
// the one-launch bf16 rows step (oracle: gpt_blocks(act_bf16, kv_bf16)): the residual stream stays fp32 in c->x; the row kernel
// completes it and publishes x~ = bf16(x) (FB16, in c->a) with the (mean, rstd) of x~; c_attn / c_fc consume x~ against bf16(W g) and
// apply the folded LayerNorm in their epilogue; the attention output (fp32 rows, in c->h) is rounded into c->a by a convert launch;
// c_fc stores bf16(gelu_new(.)) in FB16 (in c->h); the N = d projections leave raw K-split partials for the next row kernel.
// 8 launches per layer (the fp32 path: 7).  The attention runs with ONE key chunk per (row, head): run_rows' 2 / 4-way key split of a batched decode
// step over long contexts merges its partials inside the fp32 skinny c_proj GEMM, which this path does not use.
static int run_rows_b16(gvc_gpt* c, const int32_t* slots, int B, int T, hipStream_t s, const int32_t* base_len) {
    const int d = c->dm.d_model, rows = B * T, L = c->dm.n_layer;
    GVC_REQUIRE((long long)rows * d <= c->work_cap / 2, GVC_ERR_STATE, "weight_dtype 4: %d rows exceed the split-K scratch", rows);   // (sized for max_rows at create)
    int rc;
    float* part_proj = c->work;
    float* part_p2 = c->work + c->work_cap / 2;
    unsigned short* a16 = reinterpret_cast<unsigned short*>(c->a);
    unsigned short* h16 = reinterpret_cast<unsigned short*>(c->h);
    int sk_p2 = 0, sk_proj = 0;
    for (int l = 0; l < L; ++l) {
        const GptLayer& ly = c->layers[l];
        const float* f = c->b16_fold + (size_t)l * 14 * d;
        if ((rc = launch_ln_sum_rows_b16(c->x, c->x, a16, c->b16_stats, l > 0 ? part_p2 : nullptr, sk_p2, l > 0 ? c->layers[l - 1].p2_b : nullptr,
                                         rows, d, s)))
            return rc;
        GemmArgs G;
        B16Epi F;
        memset(&G, 0, sizeof(G));
        memset(&F, 0, sizeof(F));
        G.A = c->a; G.lda = d; G.Wt = reinterpret_cast<const float*>(b16_w(c, l, 0)); G.ldw = d; G.C = c->q; G.ldc = d; G.M = rows; G.N = 3 * d; G.K = d;
        G.e.qkv = 1; G.e.d = d; G.e.n_head = c->dm.n_head; G.e.head_dim = c->hd; G.e.max_seq = c->dm.max_seq; G.e.T = T; G.e.slots = slots;
        G.e.base_len = base_len; G.e.kcache = kv_layer(c, l, 0); G.e.vcache = kv_layer(c, l, 1); G.e.kv_bf16 = c->kv_bf16;
        F.stats = c->b16_stats; F.S = f; F.Cc = f + 3 * d;
        if ((rc = launch_gemm_strip_b16(G, F, 1, c->work_cap, 0, nullptr, s))) return rc;

        AttnArgs At = gpt_attn_args(c, l, slots);
        At.q = c->q; At.T = T; At.base_len = base_len;
        At.out = c->h; At.out_stride = d; At.out_fm16 = 0;
        if ((rc = launch_attention(c, At, 1, rows, true, s, base_len && T == 1))) return rc;
        if ((rc = launch_to_fb16(c->h, a16, rows, d, nullptr, s))) return rc;

        memset(&G, 0, sizeof(G));
        memset(&F, 0, sizeof(F));
        G.A = c->a; G.lda = d; G.Wt = reinterpret_cast<const float*>(b16_w(c, l, 1)); G.ldw = d; G.C = c->x; G.ldc = d; G.M = rows; G.N = d; G.K = d;
        G.work = part_proj;
        if ((rc = launch_gemm_strip_b16(G, F, 8, c->work_cap / 2, 1, &sk_proj, s))) return rc;
        if ((rc = launch_ln_sum_rows_b16(c->x, c->x, a16, c->b16_stats, part_proj, sk_proj, ly.proj_b, rows, d, s))) return rc;

        memset(&G, 0, sizeof(G));
        G.A = c->a; G.lda = d; G.Wt = reinterpret_cast<const float*>(b16_w(c, l, 2)); G.ldw = d; G.C = c->h; G.ldc = 4 * d; G.M = rows; G.N = 4 * d; G.K = d;
        G.e.act = ACT_GELU_NEW;
        F.stats = c->b16_stats; F.S = f + 6 * d; F.Cc = f + 10 * d; F.c_b16 = h16;
        if ((rc = launch_gemm_strip_b16(G, F, 1, c->work_cap, 0, nullptr, s))) return rc;

        memset(&G, 0, sizeof(G));
        memset(&F, 0, sizeof(F));
        G.A = c->h; G.lda = 4 * d; G.Wt = reinterpret_cast<const float*>(b16_w(c, l, 3)); G.ldw = 4 * d; G.C = c->x; G.ldc = d; G.M = rows; G.N = d; G.K = 4 * d;
        G.work = part_p2;
        if ((rc = launch_gemm_strip_b16(G, F, 8, c->work_cap / 2, 1, &sk_p2, s))) return rc;
        c->b16_launches += 4;
    }
    // fold the last layer's mlp partials into the residual stream (what the head reads)
    return launch_ln_sum_rows_b16(c->x, c->x, nullptr, nullptr, part_p2, sk_p2, c->layers[L - 1].p2_b, rows, d, s);
}

// The taps of a gvc_gpt_trace call in front of layer l's attention launch: hidden plane l (the embedded rows for l = 0, else the residual
// after layer l - 1), the layer's attention weights (trace.h) and its share of the alignment map.
static int trace_layer(gvc_gpt* c, int l, const AttnArgs& At, int B, hipStream_t s) {
    const TraceCall& tr = *c->trace;
    const int d = c->dm.d_model, T = At.T, H = c->dm.n_head;
    int rc;
    if (tr.hidden) {
        hipLaunchKernelGGL(k_trace_hidden, dim3(cdiv(B * T, 4)), dim3(256), 0, s, c->x, tr.hidden + (size_t)l * B * T * d, B, T, d, tr.lens, tr.P,
                           (const float*)nullptr, (const float*)nullptr);
        GVC_LAUNCH_CHECK();
    }
    const bool chosen = tr.align && ((tr.layers >> l) & 1ull);
    if (!tr.probs && !chosen) return GVC_OK;
    float* pl = tr.probs ? tr.probs + (size_t)l * B * H * T * T : tr.scratch;
    if ((rc = launch_attention_probs(c->hd, H, At, B, tr.lens, tr.P, pl, s))) return rc;
    if (chosen) {
        const int total = B * tr.n * tr.Tc;
        int first = 1;
        for (int k = 0; k < l; ++k) first &= !((tr.layers >> k) & 1ull);
        hipLaunchKernelGGL(k_trace_align, dim3(cdiv(total, 256)), dim3(256), 0, s, pl, tr.align, B, H, T, tr.P, tr.n, tr.c0, tr.Tc, first,
                           l == tr.last_chosen ? 1.0f / (float)(H * tr.n_chosen) : 0.f);
        GVC_LAUNCH_CHECK();
    }
    return GVC_OK;
}

static int run_rows(gvc_gpt* c, const int32_t* slots, int B, int T, hipStream_t s, const int32_t* base_len, int key_chunks) {
    const int d = c->dm.d_model, rows = B * T;
    int rc;
    // 2..16 rows that continue cached sequences (a batched decode step, the uncached rows of a streaming chunk): ONE launch
    if (c->r_ready == 1 && rows_persist_ok(c, rows, base_len))
        return launch_rows_persist(c, slots, rows, T, base_len, rows_persist_chunks(c, rows, c->rows_keys_hint), s);
    if (c->mfma_b16 && rows > 1) return run_rows_b16(c, slots, B, T, s, base_len);
    const bool skinny = c->skinny_prefill && c->wfm && rows <= 128 && d % 256 == 0 && (long long)4 * rows * d <= c->work_cap / 2;
    const int SKP = 4;
    float* part_proj = c->work;                                    // [SKP][rows][d]
    float* part_p2 = c->work + c->work_cap / 2;                    // [SKP][rows][d]
    int ln_rc = GVC_OK;          // (a lambda cannot return through GVC_REQUIRE: the first failure is kept and returned below)
    // batched decode over long contexts (key_chunks > 1, from the caller's key bound): the keys of a (stream, head) are split over
    // 2 or 4 workgroups of k_attention and the chunk partials are merged while the attn c_proj GEMM loads its A fragments
    const int att_nc = (skinny && base_len && T == 1 && rows <= 32 && c->hd == 256 && (key_chunks == 2 || key_chunks == 4) &&
                        rows <= c->dm.max_slots) ? key_chunks : 1;
    // <= fuse_ln_rows rows (8: a batched decode step of <= 8 streams; beyond, the prologue's L2 traffic -- rows x 6 planes in every
    // workgroup -- costs more than the two launches it saves): the row completion + LayerNorm runs
    // in the prologue of the QKV / c_fc GEMMs (5 launches per layer instead of 7); the residual stream ping-pongs between
    // c->x and c->xalt because only workgroup 0 of a launch writes the completed rows while the others still read them
    if (skinny && rows <= c->fuse_ln_rows && c->fuse_ln && d <= 1024 && !c->trace) {
        float* X[2] = {c->x, c->xalt};
        int cur = 0;
        for (int l = 0; l < c->dm.n_layer; ++l) {
            const GptLayer& ly = c->layers[l];
            GemmArgs G;
            LnFuse P;
            memset(&G, 0, sizeof(G));
            memset(&P, 0, sizeof(P));
            P.x_in = X[cur]; P.ln_w = ly.ln1_w; P.ln_b = ly.ln1_b; P.rows = rows;
            if (l > 0) { P.part = part_p2; P.SK = SKP; P.pbias = c->layers[l - 1].p2_b; P.x_out = X[cur ^ 1]; }
            G.Wt = ly.qkv_f; G.w_bf16 = c->bf16; G.ldw = d; G.C = c->q; G.ldc = d; G.M = rows; G.N = 3 * d; G.K = d;
            G.e.bias = ly.qkv_b; G.e.qkv = 1; G.e.d = d; G.e.n_head = c->dm.n_head;
            G.e.head_dim = c->hd; G.e.max_seq = c->dm.max_seq; G.e.T = T; G.e.slots = slots; G.e.base_len = base_len;
            G.e.kcache = kv_layer(c, l, 0);
            G.e.vcache = kv_layer(c, l, 1);
            G.e.kv_bf16 = c->kv_bf16;
            if ((rc = launch_gemm_skinny_ln(G, P, s))) return rc;
            if (l > 0) cur ^= 1;

            AttnArgs At = gpt_attn_args(c, l, slots);
            At.q = c->q; At.T = T; At.base_len = base_len;
            At.out = c->a; At.out_stride = d; At.out_fm16 = 1;
            if (att_nc > 1) {
                At.out = c->part;
                if ((rc = launch_attention(c, At, att_nc, rows, false, s, true))) return rc;
            } else if ((rc = launch_attention(c, At, 1, rows, true, s, base_len && T == 1))) return rc;

            memset(&G, 0, sizeof(G));
            G.A = c->a; G.lda = d; G.Wt = ly.proj_f; G.w_bf16 = c->bf16; G.ldw = d; G.C = c->x; G.ldc = d; G.M = rows; G.N = d; G.K = d; G.work = part_proj;
            if (att_nc > 1) { G.att_part = c->part; G.att_nc = att_nc; G.att_heads = c->dm.n_head; G.att_hd = c->hd; }
            if ((rc = launch_gemm_skinny(G, SKP, c->work_cap / 2, s))) return rc;

            memset(&G, 0, sizeof(G));
            memset(&P, 0, sizeof(P));
            P.x_in = X[cur]; P.x_out = X[cur ^ 1]; P.part = part_proj; P.SK = SKP; P.pbias = ly.proj_b;
            P.ln_w = ly.ln2_w; P.ln_b = ly.ln2_b; P.rows = rows;
            G.Wt = ly.fc_f; G.w_bf16 = c->bf16; G.ldw = d; G.C = c->h; G.ldc = 4 * d; G.M = rows; G.N = 4 * d; G.K = d;
            G.e.bias = ly.fc_b; G.e.act = ACT_GELU_NEW; G.e.c_fm16 = 1;
            if ((rc = launch_gemm_skinny_ln(G, P, s))) return rc;
            cur ^= 1;

            memset(&G, 0, sizeof(G));
            G.A = c->h; G.lda = 4 * d; G.Wt = ly.p2_f; G.w_bf16 = c->bf16; G.ldw = 4 * d; G.C = c->x; G.ldc = d; G.M = rows; G.N = d; G.K = 4 * d; G.work = part_p2;
            if ((rc = launch_gemm_skinny(G, SKP, c->work_cap / 2, s))) return rc;
        }
        // fold the last layer's mlp partials into the residual stream, landing in c->x (what the head reads)
        return launch_ln_sum_rows(X[cur], c->x, c->a, part_p2, SKP, c->layers[c->dm.n_layer - 1].p2_b, rows, d, nullptr, nullptr, 1, s);
    }
    // more rows than the skinny kernels take: the strip GEMM (gemm.hip) on the same fragment-major operands; the N = d projections
    // leave raw K-split partials for the next LayerNorm launch exactly as the skinny path does (the split is the launcher's choice)
    const bool strip = !skinny && c->strip_prefill && c->skinny_prefill && c->wfm && d % 256 == 0 && d <= 1024 &&
                       (long long)rows * d <= c->work_cap / 2;
    const bool fm = skinny || strip;
    auto gemm_fm = [&](GemmArgs& G, int sk_max, int raw, int* sk_used) -> int {
        if (strip) return launch_gemm_strip(G, sk_max, sk_max > 1 ? c->work_cap / 2 : c->work_cap, raw, sk_used, s);
        if (sk_used) *sk_used = sk_max;
        return launch_gemm_skinny(G, sk_max, sk_max > 1 ? c->work_cap / 2 : c->work_cap, s);
    };
    auto ln_fm = [&](const float* w, const float* b) {
        hipLaunchKernelGGL(k_ln_rows, dim3(cdiv(rows, 4)), dim3(256), 0, s, c->x, c->a, rows, d, w, b, (const float*)nullptr,
                           (const float*)nullptr, fm ? 1 : 0);
    };
    auto ln_sum_sk = [&](const float* part, int SK, const float* bias, const float* w, const float* b) {
        const int r = launch_ln_sum_rows(c->x, c->x, c->a, part, SK, bias, rows, d, w, b, 1, s);
        if (ln_rc == GVC_OK) ln_rc = r;
    };
    int sk_p2 = SKP, sk_proj = SKP;
    for (int l = 0; l < c->dm.n_layer; ++l) {
        const GptLayer& ly = c->layers[l];
        if (fm && l > 0) ln_sum_sk(part_p2, sk_p2, c->layers[l - 1].p2_b, ly.ln1_w, ly.ln1_b);
        else ln_fm(ly.ln1_w, ly.ln1_b);
        GVC_LAUNCH_CHECK();
        GemmArgs G;
        memset(&G, 0, sizeof(G));
        G.A = c->a; G.lda = d; G.Wt = fm ? ly.qkv_f : ly.qkv_w; G.w_bf16 = fm && c->bf16; G.ldw = d; G.C = c->q; G.ldc = d; G.M = rows; G.N = 3 * d; G.K = d;
        G.work = c->work; G.e.bias = ly.qkv_b; G.e.qkv = 1; G.e.d = d; G.e.n_head = c->dm.n_head;
        G.e.head_dim = c->hd; G.e.max_seq = c->dm.max_seq; G.e.T = T; G.e.slots = slots; G.e.base_len = base_len;
        G.e.kcache = kv_layer(c, l, 0);
        G.e.vcache = kv_layer(c, l, 1);
        G.e.kv_bf16 = c->kv_bf16;
        if ((rc = fm ? gemm_fm(G, 1, 0, nullptr) : launch_gemm_cap(G, 1, c->work_cap, s))) return rc;

        AttnArgs At = gpt_attn_args(c, l, slots);
        At.q = c->q; At.T = T; At.base_len = base_len;
        At.out = c->a; At.out_stride = d; At.out_fm16 = fm ? 1 : 0;
        if (c->trace && (rc = trace_layer(c, l, At, B, s))) return rc;      // c->x: the residual in front of layer l; q and the K rows are in place
        // one new row per cached stream (batched decode): 16 waves share the keys of a (row, head)
        if (att_nc > 1) {
            At.out = c->part;
            if ((rc = launch_attention(c, At, att_nc, rows, false, s, true))) return rc;
        } else if ((rc = launch_attention(c, At, 1, rows, true, s, base_len && T == 1))) return rc;

        memset(&G, 0, sizeof(G));
        G.A = c->a; G.lda = d; G.Wt = fm ? ly.proj_f : ly.proj_w; G.w_bf16 = fm && c->bf16; G.ldw = d; G.C = c->x; G.ldc = d; G.M = rows; G.N = d; G.K = d;
        if (fm) {
            G.work = part_proj;
            if (att_nc > 1) { G.att_part = c->part; G.att_nc = att_nc; G.att_heads = c->dm.n_head; G.att_hd = c->hd; }
            if ((rc = gemm_fm(G, strip ? 8 : SKP, 1, &sk_proj))) return rc;
            ln_sum_sk(part_proj, sk_proj, ly.proj_b, ly.ln2_w, ly.ln2_b);
        } else {
            G.work = c->work; G.e.bias = ly.proj_b; G.e.resid = c->x; G.e.ldr = d;
            if ((rc = launch_gemm_cap(G, 1, c->work_cap, s))) return rc;
            ln_fm(ly.ln2_w, ly.ln2_b);
        }
        GVC_LAUNCH_CHECK();
        memset(&G, 0, sizeof(G));
        G.A = c->a; G.lda = d; G.Wt = fm ? ly.fc_f : ly.fc_w; G.w_bf16 = fm && c->bf16; G.ldw = d; G.C = c->h; G.ldc = 4 * d; G.M = rows; G.N = 4 * d; G.K = d;
        G.work = c->work; G.e.bias = ly.fc_b; G.e.act = ACT_GELU_NEW; G.e.c_fm16 = fm ? 1 : 0;
        if ((rc = fm ? gemm_fm(G, 1, 0, nullptr) : launch_gemm_cap(G, 1, c->work_cap, s))) return rc;

        memset(&G, 0, sizeof(G));
        G.A = c->h; G.lda = 4 * d; G.Wt = fm ? ly.p2_f : ly.p2_w; G.w_bf16 = fm && c->bf16; G.ldw = 4 * d; G.C = c->x; G.ldc = d; G.M = rows; G.N = d; G.K = 4 * d;
        if (fm) {
            G.work = part_p2;
            if ((rc = gemm_fm(G, strip ? 8 : SKP, 1, &sk_p2))) return rc;
        } else {
            G.work = c->work; G.e.bias = ly.p2_b; G.e.resid = c->x; G.e.ldr = d;
            if ((rc = launch_gemm_cap(G, 1, c->work_cap, s))) return rc;
        }
    }
    if (fm) {       // fold the last layer's mlp partials into the residual stream
        ln_sum_sk(part_p2, sk_p2, c->layers[c->dm.n_layer - 1].p2_b, nullptr, nullptr);
        GVC_LAUNCH_CHECK();
    }
    if (c->trace && c->trace->hidden && ln_rc == GVC_OK) {      // the last plane: ln_f of the last residual
        hipLaunchKernelGGL(k_trace_hidden, dim3(cdiv(rows, 4)), dim3(256), 0, s, c->x, c->trace->hidden + (size_t)c->dm.n_layer * rows * d, B, T, d,
                           c->trace->lens, c->trace->P, (const float*)c->lnf_w, (const float*)c->lnf_b);
        GVC_LAUNCH_CHECK();
    }
    return ln_rc;
}

extern "C" int gvc_gpt_prefill(gvc_gpt* c, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P,
                               int32_t start_tok, float* logits_out, float* latent_out, gvc_stream sv) {
    return gvc_gpt_prefill_cached(c, slots, B, prefix_emb, P, 0, start_tok, logits_out, latent_out, sv);
}

// hidden_out (nullable, n_cached == 0): ln_f of every computed row [B][P+1][d] (gvc_gpt_prefill_hidden)
static int prefill_impl(gvc_gpt* c, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P, int32_t n_cached,
                        int32_t start_tok, float* logits_out, float* latent_out, float* hidden_out, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    const int T = P + 1, d = c->dm.d_model;
    GVC_REQUIRE(n_cached >= 0 && n_cached <= P, GVC_ERR_ARG, "prefill: n_cached=%d outside [0,%d]", n_cached, P);
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots, GVC_ERR_ARG, "prefill: B=%d outside [1,%d]", B, c->dm.max_slots);
    GVC_REQUIRE(P >= 0 && B * T <= c->dm.max_rows, GVC_ERR_ARG, "prefill: %d rows exceed max_rows %d", B * T, c->dm.max_rows);
    GVC_REQUIRE(T < c->dm.max_seq, GVC_ERR_ARG, "prefill: %d rows exceed max_seq %d", T, c->dm.max_seq);
    hipStream_t s = (hipStream_t)sv;
    if (!logits_out) logits_out = c->logits;      // staging of the generation loop
    if (!latent_out) latent_out = c->latent;
    hipLaunchKernelGGL(k_embed_rows, dim3(B * (T - n_cached)), dim3(256), 0, s, c->x, prefix_emb, B, T, P, d, c->mel_emb, c->mel_pos,
                       (const int32_t*)nullptr, 0, start_tok, start_tok, n_cached);
    GVC_LAUNCH_CHECK();
    const int Tn = T - n_cached;
    if (n_cached > 0 && rows_persist_ok(c, B * Tn, c->st.seq_len) && (rc = rows_persist_prepare(c))) return rc;
    c->rows_keys_hint = T;
    if (n_cached > 0) {
        // the rows continue the cached prefix: K/V go to positions n_cached.., attention sees [0, n_cached + t]
        hipLaunchKernelGGL(k_set_state, dim3(cdiv(B, 64)), dim3(64), 0, s, c->st, slots, B, n_cached, 0);
        GVC_LAUNCH_CHECK();
        if ((rc = run_rows(c, slots, B, Tn, s, c->st.seq_len))) return rc;
    } else if ((rc = run_rows(c, slots, B, T, s))) return rc;
    if (hidden_out) {
        hipLaunchKernelGGL(k_ln_rows, dim3(cdiv(B * Tn, 4)), dim3(256), 0, s, c->x, hidden_out, B * Tn, d, c->lnf_w, c->lnf_b,
                           (const float*)nullptr, (const float*)nullptr, 0);
        GVC_LAUNCH_CHECK();
    }
    if ((rc = launch_head(c, slots, B, 0, c->x, Tn, Tn - 1, logits_out, latent_out, 0, nullptr, s))) return rc;
    hipLaunchKernelGGL(k_set_state, dim3(cdiv(B, 64)), dim3(64), 0, s, c->st, slots, B, T, 1);
    GVC_LAUNCH_CHECK();
    // park the next-step logits / latent per slot: gvc_gpt_generate continues every slot from here, whoever received them
    hipLaunchKernelGGL(k_stage_rows, dim3(B), dim3(256), 0, s, logits_out, c->slot_logits, slots, c->dm.vocab, 1);
    hipLaunchKernelGGL(k_stage_rows, dim3(B), dim3(256), 0, s, latent_out, c->slot_latent, slots, d, 1);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

extern "C" int gvc_gpt_prefill_cached(gvc_gpt* c, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P,
                                      int32_t n_cached, int32_t start_tok, float* logits_out, float* latent_out, gvc_stream sv) {
    return prefill_impl(c, slots, B, prefix_emb, P, n_cached, start_tok, logits_out, latent_out, nullptr, sv);
}

extern "C" int gvc_gpt_prefill_hidden(gvc_gpt* c, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P, int32_t start_tok,
                                      float* hidden_out, gvc_stream sv) {
    GVC_REQUIRE(hidden_out, GVC_ERR_ARG, "prefill_hidden: null hidden_out");
    return prefill_impl(c, slots, B, prefix_emb, P, 0, start_tok, nullptr, nullptr, hidden_out, sv);
}

// The conditioning rows alone (no text rows, no start token, no head): K/V of rows 0..n_cond-1 into the slots' caches, length n_cond.
// For callers that know the target speaker before the first source segment arrives (a streaming session: the reference recomputes these
// rows inside every segment's prefill, inference_utils.py:43-66): every segment, the first one too, then takes gvc_gpt_prefill_cached with
// n_cached = n_cond.  Same kernels and per-row arithmetic as the rows of a full prefill (each row's projections depend on that row only,
// its attention on the rows in front of it).
extern "C" int gvc_gpt_prefill_cond(gvc_gpt* c, const int32_t* slots, int32_t B, const float* cond_latents, int32_t n_cond, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    const int d = c->dm.d_model;
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots && n_cond >= 1 && B * n_cond <= c->dm.max_rows && n_cond < c->dm.max_seq, GVC_ERR_ARG,
                "prefill_cond: bad B=%d n_cond=%d", B, n_cond);
    hipStream_t s = (hipStream_t)sv;
    hipLaunchKernelGGL(k_embed_rows, dim3(B * n_cond), dim3(256), 0, s, c->x, cond_latents, B, n_cond, n_cond, d, c->mel_emb, c->mel_pos,
                       (const int32_t*)nullptr, 0, 0, 0, 0);
    GVC_LAUNCH_CHECK();
    c->rows_keys_hint = n_cond;
    if ((rc = run_rows(c, slots, B, n_cond, s))) return rc;
    hipLaunchKernelGGL(k_set_state, dim3(cdiv(B, 64)), dim3(64), 0, s, c->st, slots, B, n_cond, 0);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

extern "C" int gvc_gpt_latents(gvc_gpt* c, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P,
                               const int32_t* gen_codes, int32_t n, int32_t start_tok, int32_t stop_tok, float* out,
                               gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    const int T = P + n + 5, d = c->dm.d_model;
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots && n >= 1, GVC_ERR_ARG, "latents: bad B=%d n=%d", B, n);
    GVC_REQUIRE(B * T <= c->dm.max_rows, GVC_ERR_ARG, "latents: %d rows exceed max_rows %d", B * T, c->dm.max_rows);
    GVC_REQUIRE(T < c->dm.max_seq && n + 5 <= c->dm.max_mel_pos, GVC_ERR_ARG, "latents: sequence too long");
    hipStream_t s = (hipStream_t)sv;
    hipLaunchKernelGGL(k_embed_rows, dim3(B * T), dim3(256), 0, s, c->x, prefix_emb, B, T, P, d, c->mel_emb, c->mel_pos,
                       gen_codes, n, start_tok, stop_tok, 0);
    GVC_LAUNCH_CHECK();
    if ((rc = run_rows(c, slots, B, T, s))) return rc;
    hipLaunchKernelGGL(k_ln_rows, dim3(cdiv(B * T, 4)), dim3(256), 0, s, c->x, c->a, B * T, d, c->lnf_w, c->lnf_b,
                       c->fn_w, c->fn_b, 0);
    GVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gather_rows, dim3(B * n), dim3(256), 0, s, c->a, out, B, T, P, n, d);
    GVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_set_state, dim3(cdiv(B, 64)), dim3(64), 0, s, c->st, slots, B, 0, 0);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// Teacher-forced trace pass (include/genvc_hip.h): the rows of gvc_gpt_latents without its four trailing stop rows, through run_rows'
// launch-per-phase loop with the taps of trace_layer between the phases.
extern "C" int gvc_gpt_trace(gvc_gpt* c, const int32_t* slots, int32_t B, const float* prefix_emb, int32_t P, const int32_t* gen_codes,
                             int32_t n, const int32_t* lengths, const int32_t* lengths_host, const gvc_trace_options* opt, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(c->dm.weight_dtype == 0, GVC_ERR_UNSUPPORTED,
                "trace: the trace pass is a reference-numerics pass: fp32 contexts only (weight_dtype %d)", c->dm.weight_dtype);
    GVC_REQUIRE(slots && prefix_emb && gen_codes && lengths && lengths_host && opt, GVC_ERR_ARG, "trace: null argument");
    GVC_REQUIRE(opt->probs || opt->hidden || opt->align, GVC_ERR_ARG, "trace: no output asked for (probs, hidden and align are all null)");
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots && n >= 1 && P >= 1, GVC_ERR_ARG, "trace: bad B=%d n=%d P=%d", B, n, P);
    const long long T = (long long)P + n;
    const int d = c->dm.d_model, L = c->dm.n_layer;
    GVC_REQUIRE(B * T <= c->dm.max_rows, GVC_ERR_ARG, "trace: %lld rows exceed max_rows %d", B * T, c->dm.max_rows);
    GVC_REQUIRE(T < c->dm.max_seq, GVC_ERR_ARG, "trace: %lld rows per item exceed max_seq %d", T, c->dm.max_seq);
    GVC_REQUIRE(n <= c->dm.max_mel_pos - 5, GVC_ERR_ARG, "trace: %d codes exceed the position table (%d - 5)", n, c->dm.max_mel_pos);
    for (int b = 0; b < B; ++b)
        GVC_REQUIRE(lengths_host[b] >= 1 && lengths_host[b] <= n, GVC_ERR_ARG, "trace: length %d of item %d outside [1,%d]", lengths_host[b], b, n);
    GVC_REQUIRE(L <= 64, GVC_ERR_ARG, "trace: %d layers exceed the 64 bits of the layer mask", L);
    TraceCall tr;
    memset(&tr, 0, sizeof(tr));
    tr.probs = opt->probs; tr.hidden = opt->hidden; tr.align = opt->align; tr.lens = lengths; tr.P = P; tr.n = n;
    if (opt->align) {
        GVC_REQUIRE(opt->n_content >= 1 && opt->content_off >= 0 && opt->content_off + opt->n_content <= P, GVC_ERR_ARG,
                    "trace: content rows [%d, %d) outside the %d prefix rows", opt->content_off, opt->content_off + opt->n_content, P);
        GVC_REQUIRE(opt->probs || opt->scratch, GVC_ERR_ARG, "trace: align without probs needs the [B][H][T][T] scratch");
        const unsigned long long all = L == 64 ? ~0ull : (1ull << L) - 1;
        tr.layers = opt->layer_mask ? opt->layer_mask : all;
        GVC_REQUIRE((tr.layers & ~all) == 0, GVC_ERR_ARG, "trace: layer mask 0x%llx names layers past the %d of the model", tr.layers, L);
        for (int l = 0; l < L; ++l)
            if ((tr.layers >> l) & 1ull) { tr.n_chosen += 1; tr.last_chosen = l; }
        tr.scratch = opt->scratch; tr.c0 = opt->content_off; tr.Tc = opt->n_content;
    }
    hipStream_t s = (hipStream_t)sv;
    hipLaunchKernelGGL(k_embed_rows, dim3(B * (int)T), dim3(256), 0, s, c->x, prefix_emb, B, (int)T, P, d, c->mel_emb, c->mel_pos,
                       gen_codes, n, opt->start_tok, opt->stop_tok, 0);
    GVC_LAUNCH_CHECK();
    c->rows_keys_hint = (int)T;
    c->trace = &tr;
    rc = run_rows(c, slots, B, (int)T, s);
    c->trace = nullptr;
    if (rc) return rc;
    hipLaunchKernelGGL(k_set_state, dim3(cdiv(B, 64)), dim3(64), 0, s, c->st, slots, B, 0, 0);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// The block stack over a padded batch with all its text and code rows (GPT.forward's default call, gpt.py:476-506 and get_logits
// :275-304): rows = [cond (n_cond) | text rows (Lt) | code rows (Lm)] per item, causal attention with the nullable key-padding mask,
// final_norm(ln_f(h)) of the Lt + Lm rows behind the conditioning ones.  Reference numerics only (weight_dtype 0).
extern "C" int gvc_gpt_forward_rows(gvc_gpt* c, const int32_t* slots, int32_t B, const float* cond, int32_t n_cond, const int32_t* text_ids,
                                    int32_t Lt, const int32_t* code_ids, int32_t Lm, const uint8_t* key_mask, float* latents_out,
                                    gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(c->dm.weight_dtype == 0, GVC_ERR_UNSUPPORTED,
                "forward_rows: the evaluation pass is a reference-numerics pass: fp32 contexts only (weight_dtype %d)", c->dm.weight_dtype);
    GVC_REQUIRE(slots && cond && text_ids && code_ids && latents_out, GVC_ERR_ARG, "forward_rows: null argument");
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots, GVC_ERR_ARG, "forward_rows: B=%d outside [1,%d]", B, c->dm.max_slots);
    GVC_REQUIRE(n_cond >= 0 && Lt >= 1 && Lm >= 1, GVC_ERR_ARG, "forward_rows: bad row counts (n_cond %d, Lt %d, Lm %d)", n_cond, Lt, Lm);
    GVC_REQUIRE(Lt <= c->dm.max_text_pos && Lm <= c->dm.max_mel_pos, GVC_ERR_ARG,
                "forward_rows: %d text rows / %d code rows exceed the position tables (%d, %d)", Lt, Lm, c->dm.max_text_pos, c->dm.max_mel_pos);
    const long long T = (long long)n_cond + Lt + Lm;
    const int d = c->dm.d_model;
    GVC_REQUIRE(T <= c->dm.max_seq, GVC_ERR_ARG, "forward_rows: %lld rows per item exceed max_seq %d", T, c->dm.max_seq);
    GVC_REQUIRE(B * T <= c->dm.max_rows, GVC_ERR_ARG, "forward_rows: %lld rows exceed max_rows %d", B * T, c->dm.max_rows);
    hipStream_t s = (hipStream_t)sv;
    if ((rc = launch_eval_embed(c->x, cond, n_cond, text_ids, Lt, code_ids, Lm, B, d, c->text_emb, c->text_pos, c->dm.n_text, c->mel_emb,
                                c->mel_pos, c->dm.vocab, s)))
        return rc;
    c->rows_keys_hint = (int)T;
    c->eval_mask = key_mask;
    c->eval_mask_stride = (int)T;
    rc = run_rows(c, slots, B, (int)T, s);
    c->eval_mask = nullptr;
    if (rc) return rc;
    hipLaunchKernelGGL(k_ln_rows, dim3(cdiv(B * (int)T, 4)), dim3(256), 0, s, c->x, c->a, B * (int)T, d, c->lnf_w, c->lnf_b, c->fn_w, c->fn_b, 0);
    GVC_LAUNCH_CHECK();
    if ((rc = launch_eval_gather(c->a, latents_out, B, (int)T, n_cond, Lt + Lm, d, s))) return rc;
    hipLaunchKernelGGL(k_set_state, dim3(cdiv(B, 64)), dim3(64), 0, s, c->st, slots, B, 0, 0);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// One head over R latent rows and its loss terms (gpt.py:306-312, 526-535): logits_out [R][V] = head(latents), then launch_head_xent
// (forward_eval.h).  head 0: text_head (V = n_text), 1: mel_head (V = vocab)
extern "C" int gvc_gpt_head_xent(gvc_gpt* c, const float* latents, int32_t R, int32_t head, const int32_t* targets, float label_smoothing,
                                 int32_t top_k, float* logits_out, float* row_terms, double* sums, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(c->dm.weight_dtype == 0, GVC_ERR_UNSUPPORTED,
                "head_xent: the evaluation pass is a reference-numerics pass: fp32 contexts only (weight_dtype %d)", c->dm.weight_dtype);
    GVC_REQUIRE(latents && targets && logits_out && row_terms && sums, GVC_ERR_ARG, "head_xent: null argument");
    GVC_REQUIRE(head == 0 || head == 1, GVC_ERR_ARG, "head_xent: head %d (0 text_head, 1 mel_head)", head);
    GVC_REQUIRE(R >= 1 && R <= c->dm.max_rows, GVC_ERR_ARG, "head_xent: %d rows outside [1, max_rows %d]", R, c->dm.max_rows);
    GVC_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f && top_k >= 1, GVC_ERR_ARG, "head_xent: label_smoothing %g outside [0,1] or top_k %d < 1",
                (double)label_smoothing, top_k);
    GVC_REQUIRE(head == 1 || c->thead_bound == 3, GVC_ERR_STATE, "head_xent: text_head.weight / text_head.bias are not bound");
    const int d = c->dm.d_model, V = head ? c->dm.vocab : c->dm.n_text;
    const long long nt4 = ((long long)c->dm.n_text * d + 3) & ~3ll;
    hipStream_t s = (hipStream_t)sv;
    GemmArgs G;
    memset(&G, 0, sizeof(G));
    G.A = latents; G.lda = d; G.Wt = head ? c->head_w : c->thead; G.ldw = d; G.C = logits_out; G.ldc = V; G.M = R; G.N = V; G.K = d;
    G.work = c->work; G.e.bias = head ? c->head_b : c->thead + nt4;
    if ((rc = launch_gemm_cap(G, 1, c->work_cap, s))) return rc;
    return launch_head_xent(logits_out, V, targets, R, V, label_smoothing, top_k, row_terms, sums, s);
}

// ---------------------------------------------------------------------------------------------
// generation loop: one captured graph = [sample -> decode step] for a fixed B, replayed n_steps times
// ---------------------------------------------------------------------------------------------
// What a gvc_gpt_generate call over B streams that reaches `key_bound` cached positions replays: the step variant, its key split and what
// keys its captured graphs (GraphKey).  Runs the one-time preparation of the one-launch steps first (they may switch a path off for this
// context -- r_ready / persist -- so nothing is derived from rows_decode_ok / persist_ok before).
struct GenPlan {
    bool fused, greedy;
    bool defer;     // the deferring order [decode the pending token, sample]: one stream on the one-launch step
    int key_chunks, variant;
    int split;      // GraphKey::split: key_chunks, or 8 + the key split of the one-launch rows step
};

static int step_unroll() {
    // the steps of a call run as graphs of this many consecutive steps, the remainder one by one
    return 8;
}

static int plan_generate(gvc_gpt* c, int B, int key_bound, int top_k, GenPlan* pl) {
    int rc;
    pl->fused = fused_ok(c, B, key_bound);
    // rows mode splits the keys of long contexts over 2 / 4 attention workgroups per (stream, head): two from key_split cached
    // positions on (0: never), four beyond 320
    constexpr int key_split = 144;
    if (persist_ok(c, B) && (rc = persist_prepare(c))) return rc;
    if (!persist_ok(c, B) && rows_persist_ok(c, B, c->st.seq_len) && (rc = rows_persist_prepare(c))) return rc;
    pl->key_chunks = (key_split > 0 && rows_decode_ok(c, B) && !persist_ok(c, B) && B <= 32)
                         ? (key_bound > 320 ? 4 : (key_bound > key_split ? 2 : 1)) : 1;
    const bool rows1 = !persist_ok(c, B) && c->r_ready == 1 && rows_persist_ok(c, B, c->st.seq_len);      // one-launch rows step
    c->rows_keys_hint = key_bound;
    pl->split = rows1 ? 8 + rows_persist_chunks(c, B, key_bound) : pl->key_chunks;   // (the one-launch steps are pure functions of B [and the key split])
    pl->variant = persist_ok(c, B) ? 3 : (rows1 ? 5 : (rows_decode_ok(c, B) ? 4 : (pl->fused ? 2 : 1)));
    // (the sampler kernel is chosen at capture time: a graph serves top_k = 1 or everything else)
    pl->greedy = sample_greedy_ok(top_k, c->dm.d_model);
    pl->defer = c->defer && persist_ok(c, B);
    return GVC_OK;
}

// The context's graph for `key`, captured on first use (a lazy init outside warm-up) from key.unroll repetitions of `step`, which
// enqueues one step of the loop on the capture stream it is given and returns a GVC_* code.
template <class Step>
static int get_graph(gvc_gpt* c, const GraphKey& key, hipGraphExec_t* ge, Step&& step) {
    auto it = c->graphs.find(key);
    if (it == c->graphs.end()) {
        hipGraphExec_t g1;
        note_lazy(c);
        // key.unroll consecutive steps in ONE graph: the boundary between two graph launches costs several times the boundary between
        // two kernels of a graph, and the host looks at the finished flags once per group of steps anyway
        int r = capture_graph(c->cap_stream, &g1, [&] {
            int rc = GVC_OK;
            for (int u = 0; u < key.unroll && rc == GVC_OK; ++u) rc = step(c->cap_stream);
            return rc;
        });
        if (r) return r;
        it = c->graphs.emplace(key, g1).first;
    }
    *ge = it->second;
    return GVC_OK;
}

static int step_graph(gvc_gpt* c, int B, const GenPlan& pl, int unroll, hipGraphExec_t* ge) {
    return get_graph(c, GraphKey{kStepGraph, B, 0, pl.fused, pl.split, unroll, pl.greedy, pl.defer}, ge, [&](hipStream_t cs) {
        if (pl.defer) {
            // the decode of the token sampled one step (or one call) ago, if there is one, then this step's sample; the sampler raises the
            // run flag and advances the step counter
            const int rc = launch_persist(c, c->gen_call->slots, c->tok_buf, c->logits, c->latent, nullptr, cs, c->run_flag, 0);
            return rc ? rc : launch_sample_indirect(&c->gen_call->sc, B, pl.greedy, cs);
        }
        const int rc = launch_sample_indirect(&c->gen_call->sc, B, pl.greedy, cs);
        return rc ? rc : decode_step(c, c->gen_call->slots, B, c->tok_buf, c->logits, c->latent, c->step_ctr, cs, pl.fused, pl.key_chunks);
    });
}

// Classifier-free guidance (gvc_gpt_generate_cfg): rows 0..B-1 of the slot table are the items' conditional slots, rows B..2B-1 their
// unconditional ones.  One step = [k_cfg_guide over the logits rows (b, B + b) -> guided; the sampler over B rows, reading guided as its
// logits; token b mirrored to row B + b; the decode step plan_generate picks for 2B rows].  The graphs live in the context's graph map
// under kind kCfgGraph, so every path that drops the step graphs (time-out fallback, rearm, destroy) drops them too.
static int cfg_graph(gvc_gpt* c, int B, const GenPlan& pl, int unroll, hipGraphExec_t* ge) {
    const int V = c->dm.vocab;
    return get_graph(c, GraphKey{kCfgGraph, 2 * B, 0, pl.fused, pl.split, unroll, pl.greedy, 0}, ge, [&](hipStream_t cs) {
        int rc = launch_cfg_guide(c->logits, c->logits + (size_t)B * V, B, V, 1.f, &c->gen_call->cfg_scale, c->guided, cs);
        if (rc == GVC_OK) rc = launch_sample_indirect(&c->gen_call->sc, B, pl.greedy, cs);
        if (rc == GVC_OK) rc = launch_cfg_mirror(c->tok_buf, B, cs);
        if (rc == GVC_OK)
            rc = decode_step(c, c->gen_call->slots, 2 * B, c->tok_buf, c->logits, c->latent, c->step_ctr, cs, pl.fused, pl.key_chunks);
        return rc;
    });
}

// Replays n_steps steps on s: groups of step_unroll() steps, then the remainder one by one.  graph(unroll, &ge) hands out the graph of
// that many steps; each of the two is asked for only when the call needs it.
template <class Graph>
static int replay_steps(int n_steps, hipStream_t s, Graph&& graph) {
    const int unroll = step_unroll();
    int rc, left = n_steps;
    if (unroll > 1 && left >= unroll) {
        hipGraphExec_t ge;
        if ((rc = graph(unroll, &ge))) return rc;
        for (; left >= unroll; left -= unroll) GVC_CHECK_HIP(hipGraphLaunch(ge, s));
    }
    if (left > 0) {
        hipGraphExec_t ge;
        if ((rc = graph(1, &ge))) return rc;
        for (; left > 0; --left) GVC_CHECK_HIP(hipGraphLaunch(ge, s));
    }
    return GVC_OK;
}

// in_warmup for a scope: what a warm-up call allocates, synchronises and captures is no lazy init (note_lazy)
struct WarmupScope {
    gvc_gpt* c;
    explicit WarmupScope(gvc_gpt* c_) : c(c_) { c->in_warmup = 1; }
    ~WarmupScope() { c->in_warmup = 0; }
};

// Captures the unrolled and the single-step graph of every plan the key bounds lo..hi lead to (runs of bounds share one plan):
// plan(bound, &pl) is the loop's plan function, graph(pl, unroll, &ge) its graph getter.
template <class Plan, class Graph>
static int warmup_sweep(int lo, int hi, Plan&& plan, Graph&& graph) {
    int rc, last_fused = -1, last_split = -1;
    for (int mk = lo; mk <= hi; ++mk) {
        GenPlan pl;
        if ((rc = plan(mk, &pl))) return rc;
        if (pl.fused == last_fused && pl.split == last_split) continue;
        last_fused = pl.fused;
        last_split = pl.split;
        hipGraphExec_t ge;
        if (step_unroll() > 1 && (rc = graph(pl, step_unroll(), &ge))) return rc;
        if ((rc = graph(pl, 1, &ge))) return rc;
    }
    return GVC_OK;
}

// Everything a later gvc_gpt_generate / gvc_gpt_decode_step / gvc_gpt_prefill_cached call of this shape would otherwise do on first use:
// the one-launch steps' buffers, weight pack, topology probe and LDS opt-in, and the captured step graphs (eight steps and one step) for
// B streams reaching `max_keys` cached positions with this top_k.  Synchronous; call it after the weights are bound, once per shape a
// deployment uses.  After it, data-path calls of that shape neither allocate nor synchronise the device (gvc_gpt_lazy_inits stays put).
extern "C" int gvc_gpt_warmup(gvc_gpt* c, int32_t B, int32_t max_keys, int32_t top_k) {
    int rc;
    if (c && c->mfma_b16 && gvc_gpt_missing_weights(c) == 0) {       // (the pack is warm-up work, not a lazy initialisation)
        WarmupScope warm(c);
        if ((rc = b16_prepare(c))) return rc;
    }
    if ((rc = check_ready(c))) return rc;
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots && max_keys >= 0 && max_keys < c->dm.max_seq, GVC_ERR_ARG, "warmup: bad argument");
    WarmupScope warm(c);
    // the rows step also serves the <= 16 uncached rows of a cached chunk prefill, whatever B
    if (rows_persist_ok(c, 16, c->st.seq_len) && (rc = rows_persist_prepare(c))) return rc;
    GenPlan pl;
    if ((rc = plan_generate(c, B, max_keys > 0 ? max_keys : c->dm.max_seq - 1, top_k, &pl))) return rc;
    hipGraphExec_t ge;
    if (step_unroll() > 1 && (rc = step_graph(c, B, pl, step_unroll(), &ge))) return rc;
    if ((rc = step_graph(c, B, pl, 1, &ge))) return rc;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    return GVC_OK;
}

extern "C" int gvc_gpt_warmup_range(gvc_gpt* c, int32_t B, int32_t min_keys, int32_t max_keys, int32_t top_k) {
    GVC_REQUIRE(c, GVC_ERR_ARG, "null context");
    GVC_REQUIRE(min_keys >= 1 && min_keys <= max_keys && max_keys < c->dm.max_seq, GVC_ERR_ARG, "warmup_range: bad key range [%d, %d]", min_keys, max_keys);
    int rc = gvc_gpt_warmup(c, B, min_keys, top_k);          // (also prepares the one-launch steps: the plans below are then pure look-ups)
    if (rc) return rc;
    WarmupScope warm(c);
    rc = warmup_sweep(min_keys, max_keys, [&](int mk, GenPlan* pl) { return plan_generate(c, B, mk, top_k, pl); },
                      [&](const GenPlan& pl, int unroll, hipGraphExec_t* ge) { return step_graph(c, B, pl, unroll, ge); });
    if (rc) return rc;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    return GVC_OK;
}

extern "C" long long gvc_gpt_lazy_inits(gvc_gpt* c) { return c ? c->lazy_inits : 0; }

// After a hand-off time-out the context runs on the launch-per-phase paths.  That is the right answer while another context holds CUs, and
// the wrong one for the rest of a server's life: when the caller knows the GPU is its own again (a quiet moment, the other process gone) it
// re-arms the one-launch steps here.  Synchronises the device, drops the captured step graphs (they hold the fallback launches) and resets
// the hand-off state; a later time-out simply falls back again.  Pending errors are reported first, exactly as by gvc_gpt_health.
extern "C" int gvc_gpt_rearm(gvc_gpt* c) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (c->persist == c->persist_cfg) return GVC_OK;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    drop_graphs(c);
    GVC_CHECK_HIP(reset_handoffs(c));
    GVC_CHECK_HIP(hipDeviceSynchronize());
    c->persist = c->persist_cfg;
    return GVC_OK;
}

// What a generation call may carry beyond gvc_gpt_generate's arguments; everything null: that plain call.  Each gvc_gpt_generate* entry
// fills the members its signature has and generate_impl does the rest, so an option is handled in exactly one place.
struct GenOptions {
    const gvc_row_sampling* rows = nullptr;        // B host entries (gvc_gpt_generate_rows): the rows' own settings and keys, else p's for all
    const gvc_logits_processors* proc = nullptr;   // the call's one processor set (gvc_gpt_generate_proc)
    const gvc_logits_processors* sets = nullptr;   // n_sets host processor sets (gvc_gpt_generate_proc_sets) ...
    const gvc_logits_warpers* warps = nullptr;     // ... and / or n_sets host warpers (gvc_gpt_generate_warp), both indexed through
    int n_sets = 0;
    const int32_t* set_of_row = nullptr;           // B host indices (null: every row uses entry 0); ignored without sets and warps
    const int32_t* uslots = nullptr;               // the B unconditional slots of a guided call (gvc_gpt_generate_cfg) ...
    float scale = 1.f;                             // ... and its guidance scale
    float* scores_out = nullptr;                   // per-step score / logit buffers (gvc_gpt_generate_scores, SampleCall::scores_out)
    float* logits_out = nullptr;
    int out_stride = 0;
    int do_sample = 1;
    const gvc_logits_bias* bias = nullptr;         // the call's sequence bias (gvc_gpt_generate_bias)
    const gvc_logits_ras* ras = nullptr;           // n_sets host RAS entries (gvc_gpt_generate_ras), indexed through set_of_row ...
    int32_t* ras_redraws = nullptr;                // ... and the rows' redraw counters (device, nullable)
    const gvc_logits_penalties* pen = nullptr;     // n_sets host penalty entries (gvc_gpt_generate_pen), indexed through set_of_row
    const gvc_logits_watermark* wm = nullptr;      // n_sets host watermark entries (gvc_gpt_generate_wm), indexed through set_of_row
};

// the guards gvc_gpt_generate_cfg / _scores / _bias share, under the entry's name (a guided entry counts items, the others rows)
static int check_guided(const char* name, const gvc_gpt* c, const int32_t* slots, int B, bool need_uslots, const GenOptions& o) {
    const int per = o.uslots ? 2 : 1;
    GVC_REQUIRE(c && slots && (o.uslots || !need_uslots), GVC_ERR_ARG, "%s: null argument", name);
    GVC_REQUIRE(B >= 1 && per * B <= kMaxSampleRows, GVC_ERR_ARG, "%s: need 1..%d %s, got %d", name, kMaxSampleRows / per,
                need_uslots ? "items" : "rows", B);
    GVC_REQUIRE(!o.uslots || (o.scale == o.scale && fabsf(o.scale) <= 3.0e38f), GVC_ERR_ARG, "%s: the guidance scale is not finite", name);
    GVC_REQUIRE(!o.uslots || c->dm.vocab <= kCfgMaxVocab, GVC_ERR_UNSUPPORTED, "%s: vocab %d above %d", name, c->dm.vocab, kCfgMaxVocab);
    GVC_REQUIRE((!o.scores_out && !o.logits_out) || o.out_stride >= 1, GVC_ERR_ARG, "%s: output buffers without a stride", name);
    return GVC_OK;
}

static int generate_impl(gvc_gpt* c, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len, int32_t* finished,
                         const gvc_sample_params* p, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out,
                         int32_t tok_stride, float* latents_out, int32_t lat_stride, gvc_stream sv, const GenOptions& o = GenOptions()) {
    const gvc_row_sampling* rows = o.rows;
    const gvc_logits_processors* proc = o.proc;
    const gvc_logits_bias* bias = o.bias;
    const int32_t* uslots = o.uslots;
    // without sets and warpers there is nothing to index; with either, a null index means entry 0 for every row (the entries that allow
    // a null index have bounded B by kMaxSampleRows)
    const bool any = o.sets || o.warps || o.ras || o.pen || o.wm;
    const gvc_logits_processors* sets = o.sets;
    const gvc_logits_warpers* warps = o.warps;
    const int n_sets = any ? o.n_sets : 0;
    static const int32_t zeros[kMaxSampleRows] = {};
    const int32_t* set_of_row = any ? (o.set_of_row ? o.set_of_row : zeros) : nullptr;
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots && p && n_steps >= 0 && max_keys >= 0, GVC_ERR_ARG, "generate: bad argument");
    GVC_REQUIRE((!o.scores_out && !o.logits_out) || (i0 >= 0 && i0 + n_steps <= o.out_stride), GVC_ERR_ARG,
                "generate_scores: steps [%d, %d) do not fit the %d steps of a row of the output buffers", i0, i0 + n_steps, o.out_stride);
    GVC_REQUIRE(!uslots || 2 * B <= c->dm.max_slots, GVC_ERR_ARG, "generate_cfg: 2 * %d rows exceed the context's %d KV slots", B,
                c->dm.max_slots);
    const int Brows = uslots ? 2 * B : B;      // rows of the decode step
    bool rows_greedy = false;
    if (rows && (rc = check_sample_rows(rows, B, c->dm.vocab, &rows_greedy))) return rc;
    if (proc && (rc = check_procs(*proc, c->dm.vocab))) return rc;
    if (bias && (rc = check_bias(*bias, c->dm.vocab))) return rc;
    if (o.ras && (rc = check_ras(o.ras, n_sets))) return rc;
    if (o.pen && (rc = check_pen(o.pen, n_sets))) return rc;
    if (o.wm && (rc = check_wm(o.wm, n_sets, c->dm.vocab))) return rc;
    if (warps || o.ras || o.pen || o.wm) {
        if ((rc = check_warp_sets(sets, warps, n_sets, set_of_row, B, c->dm.vocab))) return rc;
    } else if (set_of_row && (rc = check_proc_sets(sets, n_sets, set_of_row, B, c->dm.vocab))) {
        return rc;
    }
    // cached positions of the longest stream once this call has run: the caller's bound, else the whole ids row
    const int key_bound = max_keys > 0 ? max_keys : ids_stride;
    GVC_REQUIRE(max_keys == 0 || max_keys < c->dm.max_seq, GVC_ERR_STATE,
                "generate: %d cached positions would overflow the KV cache (max_seq %d)", max_keys, c->dm.max_seq);
    GVC_REQUIRE(p->vocab == c->dm.vocab, GVC_ERR_ARG, "generate: vocab mismatch");
    hipStream_t s = (hipStream_t)sv;
    GenPlan pl;
    // (a keyed call replays the greedy graphs when every row is greedy, the sampling ones otherwise: the step graphs are the same)
    // (a call with a RAS table replays the sampling graphs whatever its top_k: the redraw lives in the full kernel; a penalties
    // table or a watermark table changes nothing here: both sampler kernels apply them)
    if ((rc = plan_generate(c, Brows, key_bound, o.ras ? 0 : (rows ? (rows_greedy ? 1 : 0) : p->top_k), &pl))) return rc;
    GVC_REQUIRE(!uslots || !pl.defer, GVC_ERR_STATE, "generate_cfg: the one-stream step cannot serve %d rows", Brows);
    c->last_variant = pl.variant;
    // One stream on the one-launch step: each step is [decode the pending token, if any; sample], the call ends after its last sample and
    // that token stays pending for the slot -- its decode opens the next call that continues the slot and never runs when the slot is
    // prefilled or reset instead (the end of every chunk).  Every other call settles its slots first and keeps [sample, decode].
    DeferRefs df = {nullptr, nullptr, nullptr};
    if (pl.defer) {
        df.pending = c->st.pending; df.run = c->run_flag; df.tok = c->tok_buf;
        c->defer_seen = 1;
    } else if ((rc = flush_pending(c, slots, B, s)) || (uslots && (rc = flush_pending(c, uslots, B, s)))) {
        return rc;
    }
    SampleCall sc;
    memset(&sc, 0, sizeof(sc));
    sc.run_flag = pl.defer ? c->run_flag : nullptr;
    sc.logits = uslots ? c->guided : c->logits; sc.B = B; sc.ids = ids; sc.ids_stride = ids_stride; sc.ids_len = ids_len;
    sc.finished = finished; sc.p = *p; sc.step = 0; sc.step_ptr = c->step_ctr; sc.tok_out = c->tok_buf;
    sc.tokens_out = tokens_out; sc.tok_stride = tok_stride; sc.i0 = i0; sc.latent_src = c->latent;
    sc.latents_out = latents_out; sc.lat_stride = lat_stride; sc.d = c->dm.d_model;
    // per-step outputs (gvc_gpt_generate_scores): they travel in the call state the step graphs read, so the graphs are the same.  The
    // sampler of a guided call reads the guided scores as its logits: its raw rows are the conditional rows of the decode step
    sc.scores_out = o.scores_out; sc.logits_out = o.logits_out; sc.out_stride = o.out_stride; sc.scores_warped = o.do_sample;
    sc.logits_src = uslots && o.logits_out ? c->logits : nullptr;
    if (bias) {
        // gvc_gpt_generate_bias: the struct travels by value into the device-resident call state in a launch of its own, ahead of the
        // begin launch (as the warpers do): nothing to allocate, and the caller's struct is free on return
        if ((rc = launch_stage_bias(&c->gen_call->bias, bias, s))) return rc;
        sc.bias = &c->gen_call->bias;
    }
    if (set_of_row) {
        // each set some row uses travels by value into the device-resident call state, ahead of the begin launch, which carries the
        // rows' indices (and row entries): nothing to allocate, no staging buffer, and the caller's arrays are free on return
        // (the warpers likewise, all n_sets of them in one launch)
        if (sets && (rc = launch_stage_proc_sets(c->gen_call->sets, sets, n_sets, set_of_row, B, s))) return rc;
        if (warps && (rc = launch_stage_warps(c->gen_call->warps, warps, n_sets, s))) return rc;
        if (o.ras && (rc = launch_stage_ras(c->gen_call->ras, o.ras, n_sets, s))) return rc;
        if (o.pen && (rc = launch_stage_pen(c->gen_call->pen, o.pen, n_sets, s))) return rc;
        if (o.wm && (rc = launch_stage_wm(c->gen_call->wm, o.wm, n_sets, s))) return rc;
        SampleRows sr;
        memset(&sr, 0, sizeof(sr));
        SetIndex si;
        memset(&si, 0, sizeof(si));
        memcpy(si.k, set_of_row, (size_t)B * sizeof(int32_t));
        sc.proc_sets = sets ? c->gen_call->sets : nullptr;
        sc.set_of_row = c->gen_call->set_of_row;
        sc.warps = warps ? c->gen_call->warps : nullptr;
        sc.ras = o.ras ? c->gen_call->ras : nullptr;
        sc.ras_redraws = o.ras ? o.ras_redraws : nullptr;
        sc.pen = o.pen ? c->gen_call->pen : nullptr;
        sc.wm = o.wm ? c->gen_call->wm : nullptr;
        if (rows) {
            memcpy(sr.r, rows, (size_t)B * sizeof(gvc_row_sampling));
            sc.rows = c->gen_call->rows;
            hipLaunchKernelGGL(k_gen_begin_sets<true>, dim3(B + 1), dim3(256), 0, s, c->gen_call, sc, slots, B, c->step_ctr, c->logits,
                               c->slot_logits, c->dm.vocab, c->latent, c->slot_latent, c->dm.d_model, df, sr, si);
        } else {
            hipLaunchKernelGGL(k_gen_begin_sets<false>, dim3(B + 1), dim3(256), 0, s, c->gen_call, sc, slots, B, c->step_ctr, c->logits,
                               c->slot_logits, c->dm.vocab, c->latent, c->slot_latent, c->dm.d_model, df, sr, si);
        }
    } else if (proc) {
        // (the processors travel as a kernel argument, as the rows do: nothing to allocate, and the caller's struct is free on return)
        SampleRows sr;
        memset(&sr, 0, sizeof(sr));
        if (rows) {
            memcpy(sr.r, rows, (size_t)B * sizeof(gvc_row_sampling));
            sc.rows = c->gen_call->rows;
        }
        sc.proc = &c->gen_call->proc;
        if (rows)
            hipLaunchKernelGGL(k_gen_begin_proc<true>, dim3(B + 1), dim3(256), 0, s, c->gen_call, sc, slots, B, c->step_ctr, c->logits,
                               c->slot_logits, c->dm.vocab, c->latent, c->slot_latent, c->dm.d_model, df, sr, *proc);
        else
            hipLaunchKernelGGL(k_gen_begin_proc<false>, dim3(B + 1), dim3(256), 0, s, c->gen_call, sc, slots, B, c->step_ctr, c->logits,
                               c->slot_logits, c->dm.vocab, c->latent, c->slot_latent, c->dm.d_model, df, sr, *proc);
    } else if (rows) {
        SampleRows sr;
        memset(&sr, 0, sizeof(sr));
        memcpy(sr.r, rows, (size_t)B * sizeof(gvc_row_sampling));
        sc.rows = c->gen_call->rows;          // (device address: GenCall lives in device memory)
        hipLaunchKernelGGL(k_gen_begin_rows, dim3(B + 1), dim3(256), 0, s, c->gen_call, sc, slots, B, c->step_ctr, c->logits,
                           c->slot_logits, c->dm.vocab, c->latent, c->slot_latent, c->dm.d_model, df, sr);
    } else {
        hipLaunchKernelGGL(k_gen_begin, dim3(B + 1), dim3(256), 0, s, c->gen_call, sc, slots, B, c->step_ctr, c->logits, c->slot_logits,
                           c->dm.vocab, c->latent, c->slot_latent, c->dm.d_model, df);
    }
    GVC_LAUNCH_CHECK();
    if (uslots) {
        // the unconditional rows behind the conditional ones: slot table, parked logits and latents, and the scale
        const int V = c->dm.vocab, d = c->dm.d_model;
        if ((rc = launch_cfg_begin(c->gen_call->slots, uslots, B, o.scale, &c->gen_call->cfg_scale, c->logits, c->slot_logits, V, c->latent,
                                   c->slot_latent, d, s)))
            return rc;
        if ((rc = replay_steps(n_steps, s, [&](int unroll, hipGraphExec_t* ge) { return cfg_graph(c, B, pl, unroll, ge); }))) return rc;
        hipLaunchKernelGGL(k_gen_end, dim3(B), dim3(256), 0, s, slots, c->logits, c->slot_logits, V, c->latent, c->slot_latent, d);
        hipLaunchKernelGGL(k_gen_end, dim3(B), dim3(256), 0, s, uslots, c->logits + (size_t)B * V, c->slot_logits, V,
                           c->latent + (size_t)B * d, c->slot_latent, d);
        GVC_LAUNCH_CHECK();
        return GVC_OK;
    }
    if ((rc = replay_steps(n_steps, s, [&](int unroll, hipGraphExec_t* ge) { return step_graph(c, B, pl, unroll, ge); }))) return rc;
    if (pl.defer)
        hipLaunchKernelGGL(k_gen_end_defer, dim3(1), dim3(64), 0, s, slots, c->st.pending, c->run_flag, c->tok_buf);
    else
        hipLaunchKernelGGL(k_gen_end, dim3(B), dim3(256), 0, s, slots, c->logits, c->slot_logits, c->dm.vocab, c->latent, c->slot_latent,
                           c->dm.d_model);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

extern "C" int gvc_gpt_generate(gvc_gpt* c, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride,
                                int32_t* ids_len, int32_t* finished, const gvc_sample_params* p, int32_t i0,
                                int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out,
                                int32_t lat_stride, gvc_stream sv) {
    return generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride, latents_out,
                         lat_stride, sv);
}

extern "C" int gvc_gpt_generate_rows(gvc_gpt* c, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                                     int32_t* finished, const gvc_sample_params* common, const gvc_row_sampling* rows, int32_t i0,
                                     int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out,
                                     int32_t lat_stride, gvc_stream sv) {
    GVC_REQUIRE(rows, GVC_ERR_ARG, "generate_rows: null rows");
    GenOptions o;
    o.rows = rows;
    return generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, common, i0, n_steps, max_keys, tokens_out, tok_stride,
                         latents_out, lat_stride, sv, o);
}

extern "C" int gvc_gpt_generate_proc(gvc_gpt* c, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                                     int32_t* finished, const gvc_sample_params* p, const gvc_row_sampling* rows,
                                     const gvc_logits_processors* proc, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out,
                                     int32_t tok_stride, float* latents_out, int32_t lat_stride, gvc_stream sv) {
    GenOptions o;
    o.rows = rows; o.proc = proc;
    return generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride, latents_out,
                         lat_stride, sv, o);
}

extern "C" int gvc_gpt_generate_proc_sets(gvc_gpt* c, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                                          int32_t* finished, const gvc_sample_params* p, const gvc_row_sampling* rows,
                                          const gvc_logits_processors* sets, int32_t n_sets, const int32_t* set_of_row, int32_t i0,
                                          int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out,
                                          int32_t lat_stride, gvc_stream sv) {
    GVC_REQUIRE(sets && set_of_row, GVC_ERR_ARG, "generate_proc_sets: null sets or set_of_row");
    GenOptions o;
    o.rows = rows; o.sets = sets; o.n_sets = n_sets; o.set_of_row = set_of_row;
    return generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride, latents_out,
                         lat_stride, sv, o);
}

// (neither sets nor warpers: the call without processors)
extern "C" int gvc_gpt_generate_warp(gvc_gpt* c, const int32_t* slots, int32_t B, int32_t* ids, int32_t ids_stride, int32_t* ids_len,
                                     int32_t* finished, const gvc_sample_params* p, const gvc_row_sampling* rows,
                                     const gvc_logits_processors* sets, const gvc_logits_warpers* warps, int32_t n_sets,
                                     const int32_t* set_of_row, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out,
                                     int32_t tok_stride, float* latents_out, int32_t lat_stride, gvc_stream sv) {
    GVC_REQUIRE(B >= 1 && B <= kMaxSampleRows, GVC_ERR_ARG, "generate_warp: need 1..%d rows, got %d", kMaxSampleRows, B);
    GenOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row;
    return generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride, latents_out,
                         lat_stride, sv, o);
}

// Guided generation (classifier-free guidance, HF guidance_scale): gvc_gpt_generate_warp's call over B items of two KV slots each
extern "C" int gvc_gpt_generate_cfg(gvc_gpt* c, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                                    int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                                    const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                                    int32_t n_sets, const int32_t* set_of_row, int32_t i0, int32_t n_steps, int32_t max_keys,
                                    int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride, gvc_stream sv) {
    GenOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row;
    o.uslots = uncond_slots; o.scale = scale;
    const int rc = check_guided("generate_cfg", c, slots, B, true, o);
    return rc ? rc : generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride,
                                   latents_out, lat_stride, sv, o);
}

// gvc_gpt_generate_scores (bias null; uncond_slots null: gvc_gpt_generate_warp's call, else gvc_gpt_generate_cfg's) also stores, per row
// and step, the scores the draw was taken from and / or the raw logits ([B][out_stride][vocab] fp32, either nullable).  do_sample: HF's
// flag, which only decides what the scores hold (SampleCall::scores_warped); the tokens are those of the call without the buffers, bit
// for bit.  gvc_gpt_generate_bias adds the call's sequence bias / bad words / forced EOS / renormalised scores (include/genvc_hip.h:
// gvc_logits_bias, HOST, nullable: null is exactly gvc_gpt_generate_scores, under its name)
extern "C" int gvc_gpt_generate_bias(gvc_gpt* c, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                                     int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                                     const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                                     int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, int32_t i0, int32_t n_steps,
                                     int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride,
                                     float* scores_out, float* logits_out, int32_t out_stride, int32_t do_sample, gvc_stream sv) {
    GenOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row;
    o.uslots = uncond_slots; o.scale = scale; o.bias = bias;
    o.scores_out = scores_out; o.logits_out = logits_out; o.out_stride = out_stride; o.do_sample = do_sample != 0;
    const int rc = check_guided(bias ? "generate_bias" : "generate_scores", c, slots, B, false, o);
    return rc ? rc : generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride,
                                   latents_out, lat_stride, sv, o);
}

extern "C" int gvc_gpt_generate_ras(gvc_gpt* c, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                                    int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                                    const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                                    int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, const gvc_logits_ras* ras,
                                    int32_t* ras_redraws, int32_t i0, int32_t n_steps, int32_t max_keys, int32_t* tokens_out,
                                    int32_t tok_stride, float* latents_out, int32_t lat_stride, float* scores_out, float* logits_out,
                                    int32_t out_stride, int32_t do_sample, gvc_stream sv) {
    GenOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row;
    o.uslots = uncond_slots; o.scale = scale; o.bias = bias; o.ras = ras; o.ras_redraws = ras_redraws;
    o.scores_out = scores_out; o.logits_out = logits_out; o.out_stride = out_stride; o.do_sample = do_sample != 0;
    const int rc = check_guided("generate_ras", c, slots, B, false, o);
    return rc ? rc : generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride,
                                   latents_out, lat_stride, sv, o);
}

extern "C" int gvc_gpt_generate_pen(gvc_gpt* c, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                                    int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                                    const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                                    int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, const gvc_logits_ras* ras,
                                    int32_t* ras_redraws, const gvc_logits_penalties* pen, int32_t i0, int32_t n_steps, int32_t max_keys,
                                    int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride, float* scores_out,
                                    float* logits_out, int32_t out_stride, int32_t do_sample, gvc_stream sv) {
    GenOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row;
    o.uslots = uncond_slots; o.scale = scale; o.bias = bias; o.ras = ras; o.ras_redraws = ras_redraws; o.pen = pen;
    o.scores_out = scores_out; o.logits_out = logits_out; o.out_stride = out_stride; o.do_sample = do_sample != 0;
    const int rc = check_guided("generate_pen", c, slots, B, false, o);
    return rc ? rc : generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride,
                                   latents_out, lat_stride, sv, o);
}

extern "C" int gvc_gpt_generate_wm(gvc_gpt* c, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                                   int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                                   const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                                   int32_t n_sets, const int32_t* set_of_row, const gvc_logits_bias* bias, const gvc_logits_ras* ras,
                                   int32_t* ras_redraws, const gvc_logits_penalties* pen, const gvc_logits_watermark* wm, int32_t i0,
                                   int32_t n_steps, int32_t max_keys, int32_t* tokens_out, int32_t tok_stride, float* latents_out,
                                   int32_t lat_stride, float* scores_out, float* logits_out, int32_t out_stride, int32_t do_sample,
                                   gvc_stream sv) {
    GenOptions o;
    o.rows = rows; o.sets = sets; o.warps = warps; o.n_sets = n_sets; o.set_of_row = set_of_row;
    o.uslots = uncond_slots; o.scale = scale; o.bias = bias; o.ras = ras; o.ras_redraws = ras_redraws; o.pen = pen; o.wm = wm;
    o.scores_out = scores_out; o.logits_out = logits_out; o.out_stride = out_stride; o.do_sample = do_sample != 0;
    const int rc = check_guided("generate_wm", c, slots, B, false, o);
    return rc ? rc : generate_impl(c, slots, B, ids, ids_stride, ids_len, finished, p, i0, n_steps, max_keys, tokens_out, tok_stride,
                                   latents_out, lat_stride, sv, o);
}

extern "C" int gvc_gpt_generate_scores(gvc_gpt* c, const int32_t* slots, const int32_t* uncond_slots, int32_t B, float scale, int32_t* ids,
                                       int32_t ids_stride, int32_t* ids_len, int32_t* finished, const gvc_sample_params* p,
                                       const gvc_row_sampling* rows, const gvc_logits_processors* sets, const gvc_logits_warpers* warps,
                                       int32_t n_sets, const int32_t* set_of_row, int32_t i0, int32_t n_steps, int32_t max_keys,
                                       int32_t* tokens_out, int32_t tok_stride, float* latents_out, int32_t lat_stride, float* scores_out,
                                       float* logits_out, int32_t out_stride, int32_t do_sample, gvc_stream sv) {
    return gvc_gpt_generate_bias(c, slots, uncond_slots, B, scale, ids, ids_stride, ids_len, finished, p, rows, sets, warps, n_sets,
                                 set_of_row, nullptr, i0, n_steps, max_keys, tokens_out, tok_stride, latents_out, lat_stride, scores_out,
                                 logits_out, out_stride, do_sample, sv);
}

// gvc_gpt_warmup for gvc_gpt_generate_cfg over B items: everything gvc_gpt_warmup(2B) prepares, and the guided step graphs of every
// context class up to max_keys cached positions
extern "C" int gvc_gpt_warmup_cfg(gvc_gpt* c, int32_t B, int32_t max_keys, int32_t top_k) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(B >= 1 && 2 * B <= c->dm.max_slots, GVC_ERR_ARG, "warmup_cfg: 2 * %d rows outside [2, %d]", B, c->dm.max_slots);
    if ((rc = gvc_gpt_warmup(c, 2 * B, max_keys, top_k))) return rc;
    WarmupScope warm(c);
    // every context class a guided generation reaching max_keys passes through (the calls' bounds grow with the generation)
    const int hi = max_keys > 0 ? max_keys : c->dm.max_seq - 1;
    rc = warmup_sweep(1, hi, [&](int mk, GenPlan* pl) { return plan_generate(c, 2 * B, mk, top_k, pl); },
                      [&](const GenPlan& pl, int unroll, hipGraphExec_t* ge) { return cfg_graph(c, B, pl, unroll, ge); });
    if (rc) return rc;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    return GVC_OK;
}

// ---------------------------------------------------------------------------------------------
// assisted (speculative) greedy decoding (include/genvc_hip.h; kernels in spec.hip)
// ---------------------------------------------------------------------------------------------
// One verification pass over the T new rows of each of B slots, enqueued on s: input rows, the block stack through run_rows at the
// slots' cached lengths (the one-launch rows step for <= 16 rows where it applies, else the skinny path), the head over all B * T
// rows, and the lengths.  The caller has checked the arguments, prepared the rows step and settled deferred tokens.
static int verify_rows(gvc_gpt* c, const int32_t* slots, int B, const int32_t* toks, int T, float* logits_out, float* latent_out,
                       hipStream_t s) {
    const int d = c->dm.d_model, V = c->dm.vocab, rows = B * T;
    int rc;
    if ((rc = launch_spec_embed(c->x, toks, slots, B, T, c->st.seq_len, c->st.mel_pos, c->mel_emb, c->mel_pos, d, V, c->dm.max_seq,
                                c->dm.max_mel_pos, c->spec_base, c->seam_err_dev, s)))
        return rc;
    c->last_variant = c->r_ready == 1 && rows_persist_ok(c, rows, c->spec_base) ? 5 : 4;
    if ((rc = run_rows(c, slots, B, T, s, c->spec_base))) return rc;
    if (d <= 1024) {
        // the GEMV head takes 8 rows per launch and reads no slot when it does not advance them
        for (int g = 0; g < rows && rc == GVC_OK; g += 8)
            rc = launch_head(c, slots, rows - g < 8 ? rows - g : 8, 0, c->x + (size_t)g * d, 1, 0, logits_out + (size_t)g * V,
                             latent_out + (size_t)g * d, 0, nullptr, s);
    } else {
        rc = launch_head(c, slots, rows, 0, c->x, 1, 0, logits_out, latent_out, 0, nullptr, s);
    }
    if (rc) return rc;
    return launch_spec_advance(c->st.seq_len, c->st.mel_pos, slots, B, T, c->dm.max_seq, c->dm.max_mel_pos, s);
}

static int check_verify(const gvc_gpt* c, int B, int T) {
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_slots && T >= 1, GVC_ERR_ARG, "verify: B=%d outside [1,%d] or T=%d below 1", B, c->dm.max_slots, T);
    GVC_REQUIRE(B * T <= kSpecMaxRows && B * T <= c->dm.max_rows, GVC_ERR_ARG, "verify: %d x %d rows exceed %d rows (max_rows %d)", B, T,
                kSpecMaxRows, c->dm.max_rows);
    GVC_REQUIRE(T < c->dm.max_seq - 1 && T < c->dm.max_mel_pos - 1, GVC_ERR_ARG, "verify: T=%d does not fit max_seq %d / max_mel_pos %d", T,
                c->dm.max_seq, c->dm.max_mel_pos);
    // the skinny path is the only other one that takes rows at per-slot lengths
    GVC_REQUIRE(rows_persist_ok(c, B * T, c->st.seq_len) ||
                    (c->skinny_prefill && c->wfm && (long long)4 * B * T * c->dm.d_model <= c->work_cap / 2),
                GVC_ERR_UNSUPPORTED, "verify: no rows path for %d rows of d_model %d", B * T, c->dm.d_model);
    return GVC_OK;
}

extern "C" int gvc_gpt_verify(gvc_gpt* c, const int32_t* slots, int32_t B, const int32_t* toks, int32_t T, float* logits_out,
                              float* latent_out, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(slots && toks && logits_out && latent_out, GVC_ERR_ARG, "verify: null argument");
    if ((rc = check_verify(c, B, T))) return rc;
    hipStream_t s = (hipStream_t)sv;
    if (rows_persist_ok(c, B * T, c->st.seq_len) && (rc = rows_persist_prepare(c))) return rc;
    c->rows_keys_hint = c->dm.max_seq;            // (no bound from the caller: the key split for the longest possible context)
    if ((rc = flush_pending(c, slots, B, s))) return rc;
    return verify_rows(c, slots, B, toks, T, logits_out, latent_out, s);
}

extern "C" int gvc_gpt_truncate(gvc_gpt* c, const int32_t* slots, int32_t B, const int32_t* drop, gvc_stream sv) {
    GVC_REQUIRE(c && slots && drop && B >= 1 && B <= c->dm.max_slots, GVC_ERR_ARG, "truncate: bad argument");
    hipStream_t s = (hipStream_t)sv;
    // (a deferred token sits behind the slot's length: it is decoded before the length moves)
    int rc = flush_pending(c, slots, B, s);
    if (rc) return rc;
    return launch_spec_truncate(c->st.seq_len, c->st.mel_pos, slots, B, drop, s);
}

// where a round's drafts come from when there is no assistant: prompt lookup in the row's own history (spec.h: launch_spec_lookup)
struct LookupDrafts {
    int max_ngram, from;
    int32_t* draft_len;
};

// The round loop behind gvc_gpt_generate_assisted (ss null: greedy), gvc_gpt_generate_assisted_sample (ss: the workspaces of
// speculative sampling; the draft steps run the full sampler on keyed rows and store their warped rows, the accept step is
// launch_spec_accept_sample) and gvc_gpt_generate_lookup (lk: no assistant -- a is null -- and the draft side of a round is one
// launch_spec_lookup, which hands the accept step a draft count per row and, when ss is given, the drafts' one-hot rows)
static int assisted_rounds(gvc_gpt* c, gvc_gpt* a, const int32_t* slots, const int32_t* aslots, const gvc_spec_state* st,
                           const gvc_spec_sampling* ss, const gvc_sample_params* p, const gvc_logits_processors* proc, int32_t first,
                           int32_t n_rounds, int32_t k, int32_t max_keys, int32_t a_max_keys, const LookupDrafts* lk, gvc_stream sv) {
    const char* who = lk ? "generate_lookup" : "generate_assisted";
    int rc = check_ready(c);
    if (rc) return rc;
    if (lk) {
        GVC_REQUIRE(slots, GVC_ERR_ARG, "%s: null slot list", who);
    } else {
        if ((rc = check_ready(a))) return rc;
        GVC_REQUIRE(c != a && slots && aslots, GVC_ERR_ARG, "%s: the target and the assistant are two contexts with a slot list each", who);
    }
    if ((rc = check_spec_state(st, k, p, proc, true))) return rc;
    if (ss && (rc = check_spec_sampling(ss->q_scores, ss->p_scores, ss->rows, !lk, p))) return rc;
    const gvc_spec_state& S = *st;
    const int B = S.B, V = c->dm.vocab, d = c->dm.d_model;
    GVC_REQUIRE(k >= 1 && n_rounds >= 0, GVC_ERR_ARG, "%s: k=%d below 1 or n_rounds=%d below 0", who, k, n_rounds);
    GVC_REQUIRE(p->vocab == V && (lk || a->dm.vocab == V), GVC_ERR_ARG, "%s: vocab mismatch (call %d, target %d, assistant %d)", who,
                p->vocab, V, lk ? V : a->dm.vocab);
    GVC_REQUIRE((lk || B <= a->dm.max_slots) && (!S.lats || S.d == d), GVC_ERR_ARG, "%s: %d streams / latent width %d do not fit", who, B, S.d);
    if (lk && (rc = check_spec_lookup(st, k, lk->max_ngram, lk->from, lk->draft_len, V))) return rc;
    if ((rc = check_verify(c, B, k + 1))) return rc;
    GVC_REQUIRE(max_keys > 0 && max_keys < c->dm.max_seq - 1 && (lk || (a_max_keys > 0 && a_max_keys < a->dm.max_seq - 1)), GVC_ERR_STATE,
                "%s: %d / %d cached positions would overflow a KV cache (max_seq %d / %d)", who, max_keys, a_max_keys, c->dm.max_seq,
                lk ? 0 : a->dm.max_seq);
    hipStream_t s = (hipStream_t)sv;
    if (rows_persist_ok(c, B * (k + 1), c->st.seq_len) && (rc = rows_persist_prepare(c))) return rc;
    c->rows_keys_hint = max_keys;
    GenPlan apl = {};
    if (!lk) {
        if ((rc = plan_generate(a, B, a_max_keys, ss ? p->top_k : 1, &apl))) return rc;
        a->last_variant = apl.variant;
    }
    if ((rc = flush_pending(c, slots, B, s)) || (!lk && (rc = flush_pending(a, aslots, B, s)))) return rc;
    gvc_sample_params gp = *p;
    if (!ss) gp.top_k = 1;
    if (first) {
        // token 0 of every row: the target's choice (greedy, or drawn with u_res(0)) from the logits and latent its prefill parked
        hipLaunchKernelGGL(k_stage_rows, dim3(B), dim3(256), 0, s, S.v_logits, c->slot_logits, slots, V, 0);
        hipLaunchKernelGGL(k_stage_rows, dim3(B), dim3(256), 0, s, S.v_latents, c->slot_latent, slots, d, 0);
        GVC_LAUNCH_CHECK();
        if (ss) rc = launch_spec_accept_sample(S, 0, 0, S.v_logits, S.v_latents, nullptr, 0, nullptr, false, nullptr, ss->p_scores, gp, proc, s);
        else rc = launch_spec_accept(S, 0, 0, S.v_logits, S.v_latents, nullptr, 0, nullptr, gp, proc, s);
        if (rc) return rc;
    }
    // the draft sampler: the sampler's greedy kernel on the assistant's logits, with the call's settings, on the rows' own ids (it
    // writes d_j where the accept step writes it again) but lengths and finished flags of its own; d_j lands in row j of v_toks
    SampleCall dsc;
    memset(&dsc, 0, sizeof(dsc));
    if (!lk) {
        dsc.logits = a->logits; dsc.B = B; dsc.ids = S.ids; dsc.ids_stride = S.ids_stride; dsc.ids_len = S.d_ids_len;
        dsc.finished = S.d_finished; dsc.p = gp; dsc.step_ptr = a->step_ctr; dsc.tok_out = a->tok_buf;
        dsc.tokens_out = S.v_toks; dsc.tok_stride = k + 1; dsc.i0 = 1; dsc.d = a->dm.d_model;
        if (ss) {
            // the full sampler on device-resident keyed rows (the round-begin launch writes them); the row d_j is drawn from lands in
            // row j of q_scores, as d_j lands in column j of v_toks
            dsc.rows = ss->rows; dsc.scores_out = ss->q_scores; dsc.scores_warped = 1; dsc.out_stride = k + 1;
        }
        if (proc) {
            static const int32_t zeros[kMaxSampleRows] = {};
            GVC_REQUIRE(B <= kMaxSampleRows, GVC_ERR_ARG, "%s: processors serve up to %d streams", who, kMaxSampleRows);
            if ((rc = launch_stage_proc_sets(&a->gen_call->proc, proc, 1, zeros, B, s))) return rc;
            dsc.proc = &a->gen_call->proc;
        }
    }
    const int32_t* dlen = lk ? lk->draft_len : nullptr;
    for (int r = 0; r < n_rounds; ++r) {
        if (lk) {
            // 1. the drafts of every row from its own history: one launch, which is the round's begin as well
            if ((rc = launch_spec_lookup(S, k, lk->max_ngram, lk->from, lk->draft_len, ss ? ss->q_scores : nullptr, V, s))) return rc;
        } else {
            // 1. k + 1 decode steps of the assistant: the pending token, then [sample d_j, decode d_j] for j = 1..k
            if ((rc = launch_spec_round_begin(S, k + 1, a->step_ctr, ss ? ss->rows : nullptr, gp, s))) return rc;
            if ((rc = decode_step(a, aslots, B, S.pending, a->logits, a->latent, nullptr, s, apl.fused, apl.key_chunks))) return rc;
            for (int j = 0; j < k; ++j) {
                if ((rc = launch_sample(dsc, s))) return rc;
                if ((rc = decode_step(a, aslots, B, a->tok_buf, a->logits, a->latent, a->step_ctr, s, apl.fused, apl.key_chunks))) return rc;
            }
        }
        // 2. - 4. one pass of the target over [pending, d_1..d_k], the accept step, and the caches rolled back (the looked-up drafts
        // are in no ids row yet: the sampled accept step puts them there before it warps)
        if ((rc = verify_rows(c, slots, B, S.v_toks, k + 1, S.v_logits, S.v_latents, s))) return rc;
        if (ss) rc = launch_spec_accept_sample(S, k, k + 1, S.v_logits, S.v_latents, S.v_toks + 1, k + 1, dlen, lk != nullptr, ss->q_scores,
                                               ss->p_scores, gp, proc, s);
        else rc = launch_spec_accept(S, k, k + 1, S.v_logits, S.v_latents, S.v_toks + 1, k + 1, dlen, gp, proc, s);
        if (rc) return rc;
        if ((rc = launch_spec_truncate(c->st.seq_len, c->st.mel_pos, slots, B, S.drop_target, s))) return rc;
        if (!lk && (rc = launch_spec_truncate(a->st.seq_len, a->st.mel_pos, aslots, B, S.drop_assistant, s))) return rc;
    }
    return GVC_OK;
}

extern "C" int gvc_gpt_generate_assisted(gvc_gpt* c, gvc_gpt* a, const int32_t* slots, const int32_t* aslots, const gvc_spec_state* st,
                                         const gvc_sample_params* p, const gvc_logits_processors* proc, int32_t first, int32_t n_rounds,
                                         int32_t k, int32_t max_keys, int32_t a_max_keys, gvc_stream sv) {
    return assisted_rounds(c, a, slots, aslots, st, nullptr, p, proc, first, n_rounds, k, max_keys, a_max_keys, nullptr, sv);
}

extern "C" int gvc_gpt_generate_assisted_sample(gvc_gpt* c, gvc_gpt* a, const int32_t* slots, const int32_t* aslots,
                                                const gvc_spec_state* st, const gvc_spec_sampling* ss, const gvc_sample_params* p,
                                                const gvc_logits_processors* proc, int32_t first, int32_t n_rounds, int32_t k,
                                                int32_t max_keys, int32_t a_max_keys, gvc_stream sv) {
    GVC_REQUIRE(ss, GVC_ERR_ARG, "generate_assisted_sample: null sampling workspaces");
    GVC_REQUIRE(p && p->top_k != 1, GVC_ERR_ARG, "generate_assisted_sample: top_k == 1 is the greedy call (gvc_gpt_generate_assisted)");
    return assisted_rounds(c, a, slots, aslots, st, ss, p, proc, first, n_rounds, k, max_keys, a_max_keys, nullptr, sv);
}

extern "C" int gvc_gpt_generate_lookup(gvc_gpt* c, const int32_t* slots, const gvc_spec_state* st, const gvc_spec_sampling* ss,
                                       const gvc_sample_params* p, const gvc_logits_processors* proc, int32_t first, int32_t n_rounds,
                                       int32_t k, int32_t max_ngram, int32_t from, int32_t* draft_len, int32_t max_keys, gvc_stream sv) {
    GVC_REQUIRE(!ss || (p && p->top_k != 1), GVC_ERR_ARG, "generate_lookup: top_k == 1 is the greedy call (pass no sampling workspaces)");
    const LookupDrafts lk = {max_ngram, from, draft_len};
    return assisted_rounds(c, nullptr, slots, nullptr, st, ss, p, proc, first, n_rounds, k, max_keys, 0, &lk, sv);
}

// ---------------------------------------------------------------------------------------------
// beam search: one captured graph = [k_beam_select -> k_kv_copy_span -> decode step over B*K rows], replayed n_steps times.  The
// decode step is the one plan_generate picks for B*K rows (the one-launch rows step for 2..16 rows where it applies); it addresses the
// KV cache through the device-resident slot table gen_call->slots, which the select step permutes (beam.h).  The graphs live in the
// context's graph map under kind kBeamGraph, so every path that drops the step graphs (time-out fallback, rearm, destroy) drops them too.
// ---------------------------------------------------------------------------------------------
static int beam_graph(gvc_gpt* c, int B, int K, const GenPlan& pl, int unroll, hipGraphExec_t* ge) {
    int32_t* table = c->gen_call->slots;
    gvc_beam_state dummy;
    memset(&dummy, 0, sizeof(dummy));
    return get_graph(c, GraphKey{kBeamGraph, B * K, K, pl.fused, pl.split, unroll, 0, 0}, ge, [&](hipStream_t cs) {
        int rc = launch_beam_select(dummy, nullptr, c->beam_call, B, K, c->logits, table, 0, c->st.seq_len, c->st.mel_pos, c->tok_buf, cs);
        if (rc == GVC_OK)
            rc = launch_kv_copy_span(c->beam_call, B, K, c->kv, c->dm.n_layer, c->dm.n_head, c->dm.max_seq, c->hd, c->dm.max_slots,
                                     c->kv_bf16 ? 2 : 4, c->st.seq_len, cs);
        if (rc == GVC_OK) rc = decode_step(c, table, B * K, c->tok_buf, c->logits, c->latent, nullptr, cs, pl.fused, pl.key_chunks);
        return rc;
    });
}

static int beam_plan(gvc_gpt* c, int B, int K, int key_bound, GenPlan* pl) {
    GVC_REQUIRE(B >= 1 && K >= 2 && K <= kBeamMaxK && B * K <= c->dm.max_slots, GVC_ERR_ARG,
                "beam: B*K = %d*%d rows exceed the context's %d KV slots", B, K, c->dm.max_slots);
    GVC_REQUIRE(!persist_ok(c, B * K), GVC_ERR_STATE, "beam: the one-stream step cannot serve %d rows", B * K);
    return plan_generate(c, B * K, key_bound, 1, pl);
}

extern "C" int gvc_gpt_warmup_beam(gvc_gpt* c, int32_t B, int32_t K, int32_t max_keys) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(max_keys >= 0 && max_keys < c->dm.max_seq, GVC_ERR_ARG, "warmup_beam: bad max_keys %d", max_keys);
    GVC_REQUIRE(B >= 1 && K >= 2 && B * K <= c->dm.max_slots, GVC_ERR_ARG, "warmup_beam: B*K = %d*%d outside [2, %d]", B, K, c->dm.max_slots);
    if ((rc = gvc_gpt_warmup(c, B * K, max_keys, 1))) return rc;
    WarmupScope warm(c);
    // every context class a search reaching max_keys passes through (the calls' bounds grow with the search)
    const int hi = max_keys > 0 ? max_keys : c->dm.max_seq - 1;
    rc = warmup_sweep(1, hi, [&](int mk, GenPlan* pl) { return beam_plan(c, B, K, mk, pl); },
                      [&](const GenPlan& pl, int unroll, hipGraphExec_t* ge) { return beam_graph(c, B, K, pl, unroll, ge); });
    if (rc) return rc;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    return GVC_OK;
}

static int beam_generate_impl(gvc_gpt* c, int32_t* slots, const gvc_beam_state* st, const gvc_logits_processors* proc, int32_t i0,
                              int32_t n_steps, int32_t max_keys, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(slots && st && i0 >= 0 && n_steps >= 0 && max_keys >= 0, GVC_ERR_ARG, "beam_generate: bad argument");
    if ((rc = beam_check(*st))) return rc;
    if (proc && (rc = check_procs(*proc, st->vocab))) return rc;
    GVC_REQUIRE(st->vocab == c->dm.vocab, GVC_ERR_ARG, "beam_generate: vocab mismatch");
    GVC_REQUIRE(i0 + n_steps <= st->max_new, GVC_ERR_ARG, "beam_generate: steps %d..%d past max_new %d", i0, i0 + n_steps, st->max_new);
    const int key_bound = max_keys > 0 ? max_keys : st->n0 + i0 + n_steps;
    GVC_REQUIRE(key_bound < c->dm.max_seq, GVC_ERR_STATE, "beam_generate: %d cached positions would overflow the KV cache (max_seq %d)",
                key_bound, c->dm.max_seq);
    hipStream_t s = (hipStream_t)sv;
    const int B = st->B, K = st->K, BK = B * K;
    GenPlan pl;
    if ((rc = beam_plan(c, B, K, key_bound, &pl))) return rc;
    if ((rc = flush_pending(c, slots, BK, s))) return rc;
    if ((rc = launch_beam_begin(c->beam_call, *st, proc, nullptr, i0, slots, c->gen_call->slots, c->logits, c->slot_logits, s))) return rc;
    c->last_variant = pl.variant;
    if ((rc = replay_steps(n_steps, s, [&](int unroll, hipGraphExec_t* ge) { return beam_graph(c, B, K, pl, unroll, ge); }))) return rc;
    return launch_beam_end(c->gen_call->slots, slots, BK, c->logits, c->slot_logits, c->dm.vocab, s);
}

extern "C" int gvc_gpt_beam_generate(gvc_gpt* c, int32_t* slots, const gvc_beam_state* st, int32_t i0, int32_t n_steps, int32_t max_keys,
                                     gvc_stream sv) {
    return beam_generate_impl(c, slots, st, nullptr, i0, n_steps, max_keys, sv);
}

extern "C" int gvc_gpt_beam_generate_proc(gvc_gpt* c, int32_t* slots, const gvc_beam_state* st, const gvc_logits_processors* proc,
                                          int32_t i0, int32_t n_steps, int32_t max_keys, gvc_stream sv) {
    return beam_generate_impl(c, slots, st, proc, i0, n_steps, max_keys, sv);
}

// ---------------------------------------------------------------------------------------------
// group (diverse) beam search: the beam graph with k_group_beam_select in k_beam_select's place, under kind kGroupBeamGraph.  The
// select reads G and lambda from the device-resident call, so one graph serves every G of a (B, K).
// ---------------------------------------------------------------------------------------------
static int group_beam_graph(gvc_gpt* c, int B, int K, const GenPlan& pl, int unroll, hipGraphExec_t* ge) {
    int32_t* table = c->gen_call->slots;
    gvc_beam_state dummy;
    gvc_beam_groups dummy_grp;
    memset(&dummy, 0, sizeof(dummy));
    memset(&dummy_grp, 0, sizeof(dummy_grp));
    return get_graph(c, GraphKey{kGroupBeamGraph, B * K, K, pl.fused, pl.split, unroll, 0, 0}, ge, [&](hipStream_t cs) {
        int rc = launch_group_beam_select(dummy, dummy_grp, nullptr, c->beam_call, B, c->logits, table, 0, c->st.seq_len, c->st.mel_pos,
                                          c->tok_buf, cs);
        if (rc == GVC_OK)
            rc = launch_kv_copy_span(c->beam_call, B, K, c->kv, c->dm.n_layer, c->dm.n_head, c->dm.max_seq, c->hd, c->dm.max_slots,
                                     c->kv_bf16 ? 2 : 4, c->st.seq_len, cs);
        if (rc == GVC_OK) rc = decode_step(c, table, B * K, c->tok_buf, c->logits, c->latent, nullptr, cs, pl.fused, pl.key_chunks);
        return rc;
    });
}

extern "C" int gvc_gpt_warmup_group_beam(gvc_gpt* c, int32_t B, int32_t K, int32_t G, int32_t max_keys) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(max_keys >= 0 && max_keys < c->dm.max_seq, GVC_ERR_ARG, "warmup_group_beam: bad max_keys %d", max_keys);
    GVC_REQUIRE(B >= 1 && K >= 2 && K <= kBeamMaxK && B * K <= c->dm.max_slots, GVC_ERR_ARG,
                "warmup_group_beam: B*K = %d*%d outside [2, %d] or K above %d", B, K, c->dm.max_slots, kBeamMaxK);
    GVC_REQUIRE(G >= 1 && G <= K && K % G == 0, GVC_ERR_ARG, "warmup_group_beam: %d groups do not divide %d beams", G, K);
    if ((rc = gvc_gpt_warmup(c, B * K, max_keys, 1))) return rc;
    WarmupScope warm(c);
    const int hi = max_keys > 0 ? max_keys : c->dm.max_seq - 1;
    rc = warmup_sweep(1, hi, [&](int mk, GenPlan* pl) { return beam_plan(c, B, K, mk, pl); },
                      [&](const GenPlan& pl, int unroll, hipGraphExec_t* ge) { return group_beam_graph(c, B, K, pl, unroll, ge); });
    if (rc) return rc;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    return GVC_OK;
}

extern "C" int gvc_gpt_group_beam_generate(gvc_gpt* c, int32_t* slots, const gvc_beam_state* st, const gvc_beam_groups* grp,
                                           const gvc_logits_processors* proc, int32_t i0, int32_t n_steps, int32_t max_keys,
                                           gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(slots && st && grp && i0 >= 0 && n_steps >= 0 && max_keys >= 0, GVC_ERR_ARG, "group_beam_generate: bad argument");
    if ((rc = beam_check(*st))) return rc;
    if ((rc = group_beam_check(*st, *grp))) return rc;
    if (proc && (rc = check_procs(*proc, st->vocab))) return rc;
    GVC_REQUIRE(st->vocab == c->dm.vocab, GVC_ERR_ARG, "group_beam_generate: vocab mismatch");
    GVC_REQUIRE(i0 + n_steps <= st->max_new, GVC_ERR_ARG, "group_beam_generate: steps %d..%d past max_new %d", i0, i0 + n_steps,
                st->max_new);
    const int key_bound = max_keys > 0 ? max_keys : st->n0 + i0 + n_steps;
    GVC_REQUIRE(key_bound < c->dm.max_seq, GVC_ERR_STATE,
                "group_beam_generate: %d cached positions would overflow the KV cache (max_seq %d)", key_bound, c->dm.max_seq);
    hipStream_t s = (hipStream_t)sv;
    const int B = st->B, K = st->K, BK = B * K;
    GenPlan pl;
    if ((rc = beam_plan(c, B, K, key_bound, &pl))) return rc;
    if ((rc = flush_pending(c, slots, BK, s))) return rc;
    if (i0 == 0 && grp->G > 1) {
        // group g starts from beam g*S, but only slot b*K is prefilled: the whole prefix goes to the item's other slots first (tok_buf
        // holds the source of every row until the first select rewrites it; a pair with src == dst copies nothing)
        if ((rc = launch_group_fan_src(slots, c->tok_buf, BK, K, s))) return rc;
        rc = launch_kv_fanout(c->tok_buf, slots, BK, c->kv, c->dm.n_layer, c->dm.n_head, c->dm.max_seq, c->hd, c->dm.max_slots,
                              c->kv_bf16 ? 2 : 4, c->st.seq_len, c->st.mel_pos, c->slot_logits, c->dm.vocab, c->slot_latent, c->dm.d_model,
                              c->st.pending, s);
        if (rc) return rc;
    }
    if ((rc = launch_beam_begin(c->beam_call, *st, proc, grp, i0, slots, c->gen_call->slots, c->logits, c->slot_logits, s))) return rc;
    c->last_variant = pl.variant;
    if ((rc = replay_steps(n_steps, s, [&](int unroll, hipGraphExec_t* ge) { return group_beam_graph(c, B, K, pl, unroll, ge); })))
        return rc;
    return launch_beam_end(c->gen_call->slots, slots, BK, c->logits, c->slot_logits, c->dm.vocab, s);
}

// ---------------------------------------------------------------------------------------------
// contrastive search: one captured graph = [k_cs_recall -> decode step over B*K rows -> k_cs_hidden -> k_cs_sim -> k_cs_select ->
// k_kv_copy_span], replayed n_steps times.  The decode step is the one beam_plan picks for B*K rows; it reads the candidates from tok_buf
// and leaves every row's residual in c->x (all decode variants do: launch_head reads it there), which k_cs_hidden turns into ln_f rows.
// The graphs live in the context's graph map under kind kContrastiveGraph, so time-out fallback, rearm and destroy drop them too.
// ---------------------------------------------------------------------------------------------
static int cs_prepare(gvc_gpt* c) {
    if (c->cs.ctx) return GVC_OK;
    note_lazy(c);
    const int items = c->dm.max_slots / 2 > 0 ? c->dm.max_slots / 2 : 1;
    return cs_alloc(&c->cs, items, c->dm.max_slots, c->dm.max_seq, c->dm.d_model);
}

static int cs_graph(gvc_gpt* c, int B, int K, const GenPlan& pl, int unroll, hipGraphExec_t* ge) {
    int32_t* table = c->gen_call->slots;
    return get_graph(c, GraphKey{kContrastiveGraph, B * K, K, pl.fused, pl.split, unroll, 0, 0}, ge, [&](hipStream_t cs) {
        int rc = launch_cs_recall(c->cs_call, c->cs, B, c->logits, c->latent, c->tok_buf, cs);
        if (rc == GVC_OK) rc = decode_step(c, table, B * K, c->tok_buf, c->logits, c->latent, nullptr, cs, pl.fused, pl.key_chunks);
        if (rc == GVC_OK) rc = launch_cs_hidden(c->x, c->cs, B * K, c->lnf_w, c->lnf_b, cs);
        if (rc == GVC_OK) rc = launch_cs_sim(c->cs_call, c->cs, B, cs);
        if (rc == GVC_OK) rc = launch_cs_select(c->cs_call, c->cs, B, c->tok_buf, table, c->st.seq_len, cs);
        if (rc == GVC_OK)
            rc = launch_kv_copy_span(&c->cs_call->bc, B, K, c->kv, c->dm.n_layer, c->dm.n_head, c->dm.max_seq, c->hd, c->dm.max_slots,
                                     c->kv_bf16 ? 2 : 4, c->st.seq_len, cs);
        return rc;
    });
}

extern "C" int gvc_gpt_warmup_contrastive(gvc_gpt* c, int32_t B, int32_t K, int32_t max_keys) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(max_keys >= 0 && max_keys < c->dm.max_seq, GVC_ERR_ARG, "warmup_contrastive: bad max_keys %d", max_keys);
    GVC_REQUIRE(B >= 1 && K >= 2 && K <= kCsMaxK && B * K <= c->dm.max_slots, GVC_ERR_ARG,
                "warmup_contrastive: B*K = %d*%d outside [2, %d] (K <= %d)", B, K, c->dm.max_slots, kCsMaxK);
    if ((rc = cs_check_shape(B, K, c->dm.vocab, c->dm.d_model))) return rc;      // (what every call checks: no graph the calls refuse)
    if ((rc = gvc_gpt_warmup(c, B * K, max_keys, 1))) return rc;
    WarmupScope warm(c);
    if ((rc = cs_prepare(c))) return rc;
    const int hi = max_keys > 0 ? max_keys : c->dm.max_seq - 1;
    rc = warmup_sweep(1, hi, [&](int mk, GenPlan* pl) { return beam_plan(c, B, K, mk, pl); },
                      [&](const GenPlan& pl, int unroll, hipGraphExec_t* ge) { return cs_graph(c, B, K, pl, unroll, ge); });
    if (rc) return rc;
    GVC_CHECK_HIP(hipDeviceSynchronize());
    return GVC_OK;
}

static int cs_generate_impl(gvc_gpt* c, const int32_t* slots, const gvc_contrastive_state* st, const gvc_logits_processors* proc, int32_t i0,
                            int32_t n_steps, int32_t max_keys, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    GVC_REQUIRE(slots && st && i0 >= 0 && n_steps >= 0 && max_keys >= 0, GVC_ERR_ARG, "contrastive_generate: bad argument");
    if ((rc = cs_check(*st, c->dm.d_model))) return rc;
    if (proc && (rc = check_procs(*proc, st->vocab))) return rc;
    GVC_REQUIRE(st->vocab == c->dm.vocab, GVC_ERR_ARG, "contrastive_generate: vocab mismatch");
    GVC_REQUIRE(i0 + n_steps <= st->max_new, GVC_ERR_ARG, "contrastive_generate: steps %d..%d past max_new %d", i0, i0 + n_steps,
                st->max_new);
    const int key_bound = max_keys > 0 ? max_keys : st->n0 + i0 + n_steps;
    GVC_REQUIRE(key_bound < c->dm.max_seq && st->n0 + i0 + n_steps < c->dm.max_seq, GVC_ERR_STATE,
                "contrastive_generate: %d cached positions would overflow the KV cache (max_seq %d)", st->n0 + i0 + n_steps, c->dm.max_seq);
    hipStream_t s = (hipStream_t)sv;
    const int B = st->B, K = st->K;
    GenPlan pl;
    if ((rc = beam_plan(c, B, K, key_bound, &pl))) return rc;
    if ((rc = cs_prepare(c))) return rc;
    if ((rc = flush_pending(c, slots, B * K, s))) return rc;
    if ((rc = launch_cs_begin(c->cs_call, c->cs, *st, proc, i0, slots, c->gen_call->slots, c->logits, c->slot_logits, c->latent,
                              c->slot_latent, c->st.seq_len, c->st.mel_pos, c->kv, c->dm.n_layer, c->dm.n_head, c->dm.max_seq, c->hd, c->dm.max_slots, c->kv_bf16 ? 2 : 4,
                              s)))
        return rc;
    c->last_variant = pl.variant;
    if ((rc = replay_steps(n_steps, s, [&](int unroll, hipGraphExec_t* ge) { return cs_graph(c, B, K, pl, unroll, ge); }))) return rc;
    return launch_cs_end(c->cs, slots, B, K, c->logits, c->slot_logits, c->dm.vocab, c->latent, c->slot_latent, s);
}

extern "C" int gvc_gpt_contrastive_generate(gvc_gpt* c, const int32_t* slots, const gvc_contrastive_state* st, int32_t i0, int32_t n_steps,
                                            int32_t max_keys, gvc_stream sv) {
    return cs_generate_impl(c, slots, st, nullptr, i0, n_steps, max_keys, sv);
}

extern "C" int gvc_gpt_contrastive_generate_proc(gvc_gpt* c, const int32_t* slots, const gvc_contrastive_state* st,
                                                 const gvc_logits_processors* proc, int32_t i0, int32_t n_steps, int32_t max_keys,
                                                 gvc_stream sv) {
    return cs_generate_impl(c, slots, st, proc, i0, n_steps, max_keys, sv);
}

// ---------------------------------------------------------------------------------------------
// measurement hook (bench.py roofline): launch ONLY one kernel class of the decode step (0 qkv, 1 attention,
// 2 attn c_proj, 3 mlp c_fc, 4 mlp c_proj, 5 head), layer after layer as the step does (so every launch
// streams different weights, 1.5 GB apart in total: no cache reuse), n_steps times back to back on the
// caller's stream between two hipEvents; returns the mean microseconds per launch.  HIP events resolve
// single ~5 us kernels poorly (an empty event pair already measures ~4.7 us), so the mean over a long
// back-to-back run is used; it includes the same-stream launch boundary, as rocprofv3's per-kernel
// durations summed over a decode step do.  Synchronises the stream.
// ---------------------------------------------------------------------------------------------
extern "C" int gvc_gpt_time_kernel(gvc_gpt* c, int32_t which, const int32_t* slots, int32_t B, const int32_t* tok_in,
                                   int32_t n_steps, float* avg_us, int32_t* n_launches, gvc_stream sv) {
    int rc = check_ready(c);
    if (rc) return rc;
    // which 0..5: that class alone; 6: the whole step; 16 + X: the whole step WITHOUT class X (in-situ cost of X =
    // (whole - without) / launches: the class then runs behind its real predecessor, whose output it has to fetch from
    // the other XCDs, instead of re-reading its own stale inputs from L2)
    const bool whole = which == 6 || which == 7 || (which >= 16 && which <= 21);
    GVC_REQUIRE(((which >= 0 && which <= 5) || whole) && B >= 1 && B <= 8 && n_steps >= 1 && avg_us, GVC_ERR_ARG,
                "time_kernel: bad argument");
    const bool one_launch = which == 7;
    GVC_REQUIRE(!one_launch || persist_ok(c, B), GVC_ERR_UNSUPPORTED, "time_kernel: the one-launch decode step does not serve this context");
    if (one_launch && (rc = persist_prepare(c))) return rc;
    hipStream_t s = (hipStream_t)sv;
    if ((rc = flush_pending(c, slots, B, s))) return rc;
    hipEvent_t e0, e1;
    GVC_CHECK_HIP(hipEventCreate(&e0));
    GVC_CHECK_HIP(hipEventCreate(&e1));
    // one pass over the layers with only this kernel class is captured into a graph (eager launches of ~5 us
    // kernels are host-bound) and replayed n_steps times between two events on the caller's stream
    const bool fused = fused_ok(c, B, 0);       // the short-context variant bench.py's workload runs
    c->prof_only = whole ? -1 : which;
    c->prof_skip_one = which >= 16 ? which - 16 : -1;
    hipGraphExec_t ge = nullptr;
    rc = capture_graph(c->cap_stream, &ge, [&] {
        return one_launch ? launch_persist(c, slots, tok_in, c->logits, c->latent, nullptr, c->cap_stream)
                          : decode_group(c, slots, B, 0, tok_in, c->logits, c->latent, nullptr, c->cap_stream, fused);
    });
    c->prof_only = -1;
    c->prof_skip_one = -1;
    hipError_t e = hipSuccess;
    float ms = 0.f;
    if (rc == GVC_OK) {
        (void)hipGraphLaunch(ge, s);                                   // warm-up pass
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < n_steps; ++i) (void)hipGraphLaunch(ge, s);
        (void)hipEventRecord(e1, s);
        e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    }
    if (ge) (void)hipGraphExecDestroy(ge);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    GVC_CHECK_HIP(e);
    const int n = (whole ? 1 : (which == 5 ? 1 : (fused && which == 2 ? 0 : c->dm.n_layer))) * n_steps;
    *avg_us = n ? ms * 1000.0f / (float)n : 0.f;
    if (n_launches) *n_launches = n;
    return GVC_OK;
}

extern "C" int gvc_gpt_decode_variant(gvc_gpt* c) { return c ? c->last_variant : 0; }
extern "C" long long gvc_gpt_rows_step_launches(gvc_gpt* c) { return c ? c->r_launches : 0; }
extern "C" long long gvc_gpt_bf16_gemm_launches(gvc_gpt* c) { return c ? c->b16_launches : 0; }

// one-stream one-launch steps that RAN so far (generation loops, flushes, decode_step; launches that left at the run flag are not
// counted).  Synchronises the device.
extern "C" long long gvc_gpt_one_stream_steps(gvc_gpt* c) {
    long long n = 0;
    if (!c || !c->exec_ctr || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(&n, c->exec_ctr, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return n;
}

// To be called after the caller has synchronised the stream of a decode / generate / cached-prefill call: 0 when that work ran
// cleanly; otherwise the state error of check_ready (a timed-out hand-off has switched the context to the launch-per-phase paths,
// a full KV cache / position table).  Without it such an error surfaces on the next library call.
extern "C" int gvc_gpt_health(gvc_gpt* c) { return check_ready(c); }

// debug / tests: the cached K and V rows of ONE position of one slot, every layer, to the host: host_out[layer][k | v][head][head_dim] in the
// cache's element type (fp32, or bf16 for a bf16 cache).  Returns the bytes written, or a negative error.  Synchronises the device.
extern "C" long long gvc_gpt_debug_kv_row(gvc_gpt* c, int32_t slot, int32_t pos, void* host_out) {
    if (!c || !c->kv || !host_out || slot < 0 || slot >= c->dm.max_slots || pos < 0 || pos >= c->dm.max_seq) return GVC_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return GVC_ERR_HIP;
    const size_t esz = c->kv_bf16 ? 2 : 4, row = (size_t)c->hd * esz;
    const int H = c->dm.n_head;
    char* out = static_cast<char*>(host_out);
    for (int l = 0; l < c->dm.n_layer; ++l)
        for (int which = 0; which < 2; ++which)
            for (int h = 0; h < H; ++h) {       // cache layout: [slot][head][max_seq][head_dim] per (layer, k | v)
                const char* src = reinterpret_cast<const char*>(kv_layer(c, l, which)) + (((size_t)slot * H + h) * c->dm.max_seq + pos) * row;
                if (hipMemcpy(out, src, row, hipMemcpyDeviceToHost) != hipSuccess) return GVC_ERR_HIP;
                out += row;
            }
    return (long long)(out - static_cast<char*>(host_out));
}

// debug / tests: the logits [vocab] and latent [d_model] parked for one slot between calls, to the host.  Synchronises the device.
extern "C" int gvc_gpt_debug_parked(gvc_gpt* c, int32_t slot, float* logits_host, float* latent_host) {
    if (!c || !c->slot_logits || !c->slot_latent || !logits_host || !latent_host || slot < 0 || slot >= c->dm.max_slots) return GVC_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return GVC_ERR_HIP;
    const size_t V = (size_t)c->dm.vocab, d = (size_t)c->dm.d_model;
    if (hipMemcpy(logits_host, c->slot_logits + slot * V, V * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(latent_host, c->slot_latent + slot * d, d * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return GVC_ERR_HIP;
    return GVC_OK;
}

// debug: copy the in-kernel timestamps of the GEMV launches since the last call (GVC_DEBUG_STAMPS=1)
extern "C" int gvc_gpt_debug_stamps(gvc_gpt* c, unsigned long long* host_out, int32_t max_launches) {
    if (c && c->r_dbg && max_launches == -2) {    // stamps of the last one-launch rows step: workgroup 0, [(layer * 5 + phase) * 4 + k]
        (void)hipDeviceSynchronize();
        const int n = 40 * (c->dm.n_layer + 2) + 8 * 5 * kPG;
        (void)hipMemcpy(host_out, c->r_dbg, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        return n;
    }
    if (c && c->p_dbg && max_launches < 0) {     // stamps of the last one-launch decode step (layout: persist_kernel.h)
        (void)hipDeviceSynchronize();
        // -3: with the K/V arrival stamps of the fused phase behind them (4 words per workgroup); -1: the buffer as callers have sized it so far
        const int n = 20 * (c->dm.n_layer + 2) + 2 * 5 * kPG + 8 * kPG + (max_launches == -3 ? 4 * kPG : 0);
        (void)hipMemcpy(host_out, c->p_dbg, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        return n;
    }
    if (!c || !c->dbg) return 0;
    (void)hipDeviceSynchronize();
    const int n = c->dbg_n < max_launches ? c->dbg_n : max_launches;
    (void)hipMemcpy(host_out, c->dbg, (size_t)n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    c->dbg_n = 0;
    return n;
}
