// Per-step sampling: the body of NewGenerationMixin.sample_stream (reference
// layers/stream_generator.py:834-874) with HF's RepetitionPenalty / Temperature / TopK / TopP
// processors restated on the device.  One workgroup per stream, logits staged in LDS.
#pragma once
#include <stdlib.h>

#include "common.h"
#include "logits_proc.h"
#include "watermark.h"

namespace gvc {

struct SampleCall {
    const float* logits;     // [B][vocab]
    int B;
    int32_t* ids;            // [B][ids_stride] input_ids rows of the reference loop
    int ids_stride;
    int32_t* ids_len;        // [B]
    int32_t* finished;       // [B]
    gvc_sample_params p;
    int step;                // RNG counter (used when step_ptr is null)
    const int32_t* step_ptr; // device step counter of the generation loop (nullable)
    int32_t* tok_out;        // [B] token of this step (input of the next decode step)
    int32_t* tokens_out;     // nullable: [B][tok_stride], written at i0 + step
    int tok_stride, i0;
    const float* latent_src; // nullable: [B][d] latent that predicted this token
    float* latents_out;      // nullable: [B][lat_stride][d]
    int lat_stride, d;
    // nullable: [B] per-row settings and RNG keys (gvc_row_sampling, device memory).  Null: every row uses p and draws
    // rng_uniform(p.seed, i0 + step, b).  Set: row b uses rows[b]'s processor settings and draws
    // rng_uniform(seed_b, rng_step0_b + step, rng_row_b); p then carries eos_token / vocab only, and p.top_k == 1 tells
    // launch_sample that every row is greedy.
    const gvc_row_sampling* rows;
    // nullable: the call's length / repetition processors (gvc_logits_processors, device memory).  Null: none, and the kernels
    // compute exactly what they compute without this field
    const gvc_logits_processors* proc;
    // nullable: per-row processor sets (gvc_*_proc_sets calls, device memory).  Set: row b uses proc_sets[set_of_row[b]], or no
    // processors when the index is -1, and proc is not read.  Null: proc serves every row as above
    const gvc_logits_processors* proc_sets;
    const int32_t* set_of_row;
    // nullable: typical / epsilon / eta warpers (gvc_*_warp calls, device memory), one per set: row b uses warps[set_of_row[b]] (none
    // for -1), warps[0] when set_of_row is null.  Null: none, and k_sample computes exactly what it computes without this field
    const gvc_logits_warpers* warps;
    // nullable: the run flag of a deferred-decode loop (gpt.hip: a step is [decode the pending token, sample]).  Set: the sampler raises
    // it behind every sample -- tok_out now holds a token the next decode launch must run -- and advances *step_ptr itself, which the
    // decode step does in the eager order.  One row only
    int32_t* run_flag;
    // nullable: per-step outputs of a gvc_gpt_generate_scores call, [B][out_stride][vocab] fp32 each, written at i0 + step as tokens_out
    // is.  scores_out: the row the draw is taken from, as HF's `scores` holds it -- behind the repetition penalty, the processors and
    // (scores_warped) Temperature and every warper, dropped entries -inf.  logits_out: the raw head output of the step, read from
    // logits_src when that is set (a guided call: the conditional rows; `logits` then holds the guided scores).  Null: none, and the
    // kernels compute exactly what they compute without these fields
    float* scores_out;
    float* logits_out;
    const float* logits_src;
    int out_stride;
    // HF's do_sample of the call (read only with scores_out): 1 = the scores carry Temperature and the warpers (TopK(1)'s row when
    // top_k == 1), 0 = greedy search: the full processed row, no temperature
    int scores_warped;
    // nullable: the call's sequence bias / bad words / forced EOS / renormalised scores (gvc_*_bias calls: gvc_logits_bias, device
    // memory), call-wide: independent of rows, proc_sets and warps.  Null: none, and the kernels compute exactly what they compute
    // without this field
    const gvc_logits_bias* bias;
    // nullable: repetition-aware sampling (gvc_*_ras calls: gvc_logits_ras, device memory), one entry per set, indexed like warps: row b
    // uses ras[set_of_row[b]] (none for -1), ras[0] when set_of_row is null.  Null, or an entry whose window is 0: none, and k_sample
    // computes exactly what it computes without this field, through the same barriers
    const gvc_logits_ras* ras;
    // nullable: [B] redraws of each row, incremented by the step that redraws (read only with ras)
    int32_t* ras_redraws;
    // nullable: presence / frequency / windowed repetition penalties (gvc_*_pen calls: gvc_logits_penalties, device memory), one entry
    // per set, indexed like warps and ras.  Null, or an entry with everything off: none, and both kernels compute exactly what they
    // compute without this field, through the same barriers and with no more LDS traffic
    const gvc_logits_penalties* pen;
    // nullable: green-list watermark entries (gvc_*_wm calls: gvc_logits_watermark, device memory, each pointing at a device table), one
    // entry per set, indexed like warps, ras and pen.  Null, or an entry with a null table: none, and both kernels compute exactly what
    // they compute without this field, through the same barriers and with no more LDS traffic
    const gvc_logits_watermark* wm;
};

// row b's entry of a per-step output buffer at this step (see SampleCall::scores_out)
__device__ __forceinline__ float* step_row(float* out, const SampleCall& C, int b, int step) {
    return out + ((size_t)b * C.out_stride + C.i0 + step) * (size_t)C.p.vocab;
}

// the processors of row b (uniform over the row's workgroup)
__device__ __forceinline__ const gvc_logits_processors* row_procs(const SampleCall& C, int b) {
    if (!C.set_of_row) return C.proc;
    const int k = C.set_of_row[b];
    return k >= 0 && C.proc_sets ? C.proc_sets + k : nullptr;     // (a warpers call may pass indices without processor sets)
}

// the warpers of row b (uniform over the row's workgroup)
__device__ __forceinline__ const gvc_logits_warpers* row_warps(const SampleCall& C, int b) {
    if (!C.warps) return nullptr;
    const int k = C.set_of_row ? C.set_of_row[b] : 0;
    return k >= 0 ? C.warps + k : nullptr;
}

// the repetition-aware sampling of row b (uniform over the row's workgroup); null: off
__device__ __forceinline__ const gvc_logits_ras* row_ras(const SampleCall& C, int b) {
    if (!C.ras) return nullptr;
    const int k = C.set_of_row ? C.set_of_row[b] : 0;
    return k >= 0 && C.ras[k].window > 0 ? C.ras + k : nullptr;
}

// the penalties of row b (uniform over the row's workgroup); null: off (no table, no entry, or an entry with everything off)
__device__ __forceinline__ const gvc_logits_penalties* row_pen(const SampleCall& C, int b) {
    if (!C.pen) return nullptr;
    const int k = C.set_of_row ? C.set_of_row[b] : 0;
    if (k < 0) return nullptr;
    const gvc_logits_penalties& q = C.pen[k];
    return q.presence != 0.f || q.frequency != 0.f || q.window > 0 ? C.pen + k : nullptr;
}

// What a row's penalties come to at one step: the span of ids that counts, and the settings in registers.  on == false: nothing below
// is read and the kernels run as without a table
struct PenRow {
    bool on, windowed;          // windowed: the repetition penalty follows the counts instead of `seen`
    int lo;                     // the counted ids are ids[lo .. len)
    float presence, frequency;
};
__device__ __forceinline__ PenRow pen_row(const SampleCall& C, int b, int len) {
    PenRow q{false, false, len, 0.f, 0.f};
    if (const gvc_logits_penalties* Q = row_pen(C, b)) {
        const int n_gen = len - min(max(Q->prompt_len, 0), len);          // the fake prompt ids never count
        q.on = true;
        q.windowed = Q->window > 0;
        q.lo = len - (q.windowed ? min(Q->window, n_gen) : n_gen);
        q.presence = Q->presence;
        q.frequency = Q->frequency;
    }
    return q;
}
// score - (frequency * c + presence) for c > 0, each operation rounded on its own (include/genvc_hip.h: no fused multiply-add)
__device__ __forceinline__ float pen_score(float v, int c, const PenRow& q) {
    return __fsub_rn(v, __fadd_rn(__fmul_rn(q.frequency, (float)c), q.presence));
}

// What a row's watermark comes to at one step (uniform over the row's workgroup): the table row to stage in LDS and the settings in
// registers.  on == false (no table, no entry, a null table, or a previous id outside the vocabulary): nothing below is read and the
// kernels run as without a table
struct WmRow {
    bool on, self;              // self: selfhash (one row; sampling biases only the green ids among the GVC_WM_SELFHASH_TOP highest scores)
    const uint32_t* row;        // the `words` words of this step's green list (device)
    int words;
    float bias;
};
__device__ __forceinline__ WmRow wm_row(const SampleCall& C, int b, const int32_t* ids, int len) {
    WmRow w{false, false, nullptr, 0, 0.f};
    if (!C.wm) return w;
    const int k = C.set_of_row ? C.set_of_row[b] : 0;
    if (k < 0) return w;
    const gvc_logits_watermark& M = C.wm[k];
    if (!M.table) return w;
    w.self = M.scheme == GVC_WM_SELFHASH;
    w.words = min(max(M.words, 0), kProcWords);          // (checked on the host: ceil(vocab / 32) <= kProcWords)
    w.bias = M.bias;
    if (w.self) {
        w.row = M.table;
        w.on = true;
    } else if (len >= 1) {
        const int prev = ids[len - 1];
        if (prev >= 0 && prev < C.p.vocab) {
            w.row = M.table + (size_t)prev * w.words;
            w.on = true;
        }
    }
    return w;
}
// whether id i is green in the staged row g (LDS)
__device__ __forceinline__ bool wm_green(const uint32_t* g, int i) { return (g[i >> 5] >> (i & 31)) & 1u; }

// a call with a RAS table runs on k_sample whatever its top_k: the redraw reads the full row the greedy kernel never stores
int launch_sample(const SampleCall& sc, hipStream_t s);
// the call parameters live in device memory (graph replay)
// greedy: the call has top_k == 1 (sample_greedy_ok), or every row of a keyed call has: the argmax-only kernel
int launch_sample_indirect(const SampleCall* sc_dev, int B, bool greedy, hipStream_t s);
static inline bool sample_greedy_ok(int top_k, int d) {
    return top_k == 1 && d % 4 == 0;
}

// per-row entries of one call, passed BY VALUE as a kernel argument: the runtime copies kernel arguments when the launch is
// enqueued, so the caller's host array is free again when the launching call returns and no staging buffer has to outlive it
constexpr int kMaxSampleRows = 64;
struct SampleRows {
    gvc_row_sampling r[kMaxSampleRows];
};
// host-side checks of a keyed call: B <= 64, 0 < temperature, top_k <= vocab; *all_greedy = every row has top_k == 1
int check_sample_rows(const gvc_row_sampling* rows, int B, int vocab, bool* all_greedy);
// rows[0..B) -> dst[0..B) on stream s (one small launch; the host array is not read after the launch is enqueued)
int launch_stage_rows(gvc_row_sampling* dst, const gvc_row_sampling* rows, int B, hipStream_t s);

// per-row processor sets: the set index of every row, passed BY VALUE like SampleRows (256 bytes)
struct SetIndex {
    int32_t k[kMaxSampleRows];
};
// host-side checks of a sets call: 1 <= B <= 64, 1 <= n_sets <= B, every index in [-1, n_sets), every set passes check_procs
int check_proc_sets(const gvc_logits_processors* sets, int n_sets, const int32_t* set_of_row, int B, int vocab);
// sets[k] -> dst[k] on stream s for every k some row refers to (a set no row uses is not staged), kProcSetChunk sets per launch
// (1.3 KB of kernel argument, below the 2 KB row entries of the begin launches); the host arrays are free when this returns
constexpr int kProcSetChunk = 4;
int launch_stage_proc_sets(gvc_logits_processors* dst, const gvc_logits_processors* sets, int n_sets, const int32_t* set_of_row, int B,
                           hipStream_t s);
// set_of_row[0..B) -> dst[0..B) on stream s (one small launch)
int launch_stage_set_index(int32_t* dst, const int32_t* set_of_row, int B, hipStream_t s);

// warpers of a gvc_*_warp call, all n_sets of them BY VALUE in one launch (1 KB of kernel argument)
struct WarpTable {
    gvc_logits_warpers w[kMaxSampleRows];
    int32_t n;
};
// host-side checks of a warp call: 1 <= B <= 64, 1 <= n_sets <= B, set_of_row (nullable) in [-1, n_sets), sets (nullable) pass
// check_procs, warps (nullable) hold 0 or a value in (0, 1) each and reserved == 0
int check_warp_sets(const gvc_logits_processors* sets, const gvc_logits_warpers* warps, int n_sets, const int32_t* set_of_row, int B,
                    int vocab);
// warps[0..n_sets) -> dst[0..n_sets) on stream s (one small launch)
int launch_stage_warps(gvc_logits_warpers* dst, const gvc_logits_warpers* warps, int n_sets, hipStream_t s);
// RAS entries of a gvc_*_ras call, all n_sets of them BY VALUE in one launch (1 KB of kernel argument)
struct RasTable {
    gvc_logits_ras r[kMaxSampleRows];
    int32_t n;
};
// host-side checks of a RAS table: 1 <= n_sets <= 64, window in [0, GVC_RAS_MAX_WINDOW], min_count >= 1 where the window is on,
// prompt_len >= 0, reserved == 0
int check_ras(const gvc_logits_ras* ras, int n_sets);
// ras[0..n_sets) -> dst[0..n_sets) on stream s (one small launch)
int launch_stage_ras(gvc_logits_ras* dst, const gvc_logits_ras* ras, int n_sets, hipStream_t s);
// penalty entries of a gvc_*_pen call, all n_sets of them BY VALUE in one launch (1 KB of kernel argument)
struct PenTable {
    gvc_logits_penalties q[kMaxSampleRows];
    int32_t n;
};
// host-side checks of a penalties table: 1 <= n_sets <= 64, presence and frequency finite in [-2, 2], window >= 0, prompt_len >= 0
int check_pen(const gvc_logits_penalties* pen, int n_sets);
// pen[0..n_sets) -> dst[0..n_sets) on stream s (one small launch)
int launch_stage_pen(gvc_logits_penalties* dst, const gvc_logits_penalties* pen, int n_sets, hipStream_t s);
// watermark entries of a gvc_*_wm call, all n_sets of them BY VALUE in one launch (1.5 KB of kernel argument)
struct WmTable {
    gvc_logits_watermark m[kMaxSampleRows];
    int32_t n;
};
// host-side checks of a watermark table: 1 <= n_sets <= 64; of every entry with a table: bias finite, scheme 0 / 1, words == ceil(vocab / 32) <= kProcWords,
// reserved == 0 (watermark.h: wm_entry_ok is the per-entry part)
int check_wm(const gvc_logits_watermark* wm, int n_sets, int vocab);
// wm[0..n_sets) -> dst[0..n_sets) on stream s (one small launch)
int launch_stage_wm(gvc_logits_watermark* dst, const gvc_logits_watermark* wm, int n_sets, hipStream_t s);
// *bias -> *dst on stream s, BY VALUE in one small launch (1.3 KB of kernel argument); check_bias (logits_proc.h) comes first
int launch_stage_bias(gvc_logits_bias* dst, const gvc_logits_bias* bias, hipStream_t s);

}  // namespace gvc
