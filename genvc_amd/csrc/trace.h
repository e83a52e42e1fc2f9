// Kernels of the trace pass (gvc_gpt_trace, include/genvc_hip.h): the attention weights of a teacher-forced pass, the hidden-state taps
// between its phases and the content alignment map.  Included by gpt.hip only; k_attention_tile and its instantiations are untouched
// (k_attention_probs is a kernel of its own that shares phase 1 of k_attention_tile, not a template flag of it).
#pragma once
#include "gpt_kernels.h"

namespace gvc {

// ---------------------------------------------------------------------------------------------
// Attention weights of one (16 query rows, head, item): softmax(scale * Q K^T) with the causal limit, no P V product.
//   1. S = scale * Q K^T as step 1 of k_attention_tile: key tiles shared out over the 8 waves, Q fragments in registers, K fragments
//      straight from the fp32 cache rows (written by this layer's QKV projection), v_mfma_f32_16x16x4_f32, S into LDS [16][nkp + 4]
//      (the + 4 keeps the 16 rows of a tile column on different banks, as in k_attention_tile);
//   2. row softmax in LDS, two rows per wave: the maximum over the keys [0, t] is subtracted, keys past t are left out of the maximum
//      and of the sum (never pushed down by a large negative number) and written as zeros up to T; expf and a division, as
//      torch.softmax computes it.  A row at or past the item's end (t >= P + len[b]) is all zeros;
//   3. the tile's rows are one contiguous span of out[b][h] (rows t0 .. t0+15, T floats each): it leaves LDS as float4 stores along
//      the key axis, with a scalar head and tail where T is no multiple of 4 (the span then starts off a 16-byte boundary).
// grid ((T + 15) / 16, heads, B), 512 threads, dynamic LDS 16 * (nkp + 4) floats, nkp = T rounded up to 16.
// Reads A.q, A.kbase, A.k_*_stride, A.T, A.slots, A.scale of the layer's AttnArgs; rows start at cache position 0 (no base_len).
// out: fp32 [B][heads][T][T] of this layer.
// ---------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(512) void k_attention_probs(const AttnArgs A, int nkp, const int32_t* lens, int P, float* out) {
    constexpr int KB = HD / 16;                    // 16-dim blocks of a head
    extern __shared__ __attribute__((aligned(16))) float tp_lds[];
    const int lds_s = nkp + 4;
    float* S = tp_lds;                              // [16][lds_s]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int t0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const int T = A.T;
    const int bi = A.slots ? A.slots[b] : b;
    const int nk = min(t0 + 16, T);                 // keys any row of the tile sees
    const int nkt = (nk + 15) >> 4;
    const char* kp = reinterpret_cast<const char*>(A.kbase) + (bi * A.k_batch_stride + h * A.k_head_stride) * 4;
    const size_t krow = (size_t)A.k_row_stride * 4;

    // ---- 1. S = scale * Q K^T ----
    float4 qf[KB];
    {
        const int t = min(t0 + r16, T - 1);
        const float* qp = A.q + (size_t)(b * T + t) * A.q_stride + h * HD + 4 * g;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) qf[kb] = *reinterpret_cast<const float4*>(qp + kb * 16);
    }
    for (int kt = wave; kt < nkt; kt += 8) {
        const int key = min(kt * 16 + r16, nk - 1);
        const char* kr = kp + (size_t)key * krow + (size_t)(4 * g) * 4;
        float4 kf[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) kf[kb] = *reinterpret_cast<const float4*>(kr + (size_t)kb * 16 * 4);
        at_f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};       // (two chains: a dependent MFMA waits ~40 cycles)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[kb].x, kf[kb].x, acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[kb].y, kf[kb].y, acc1, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[kb].z, kf[kb].z, acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[kb].w, kf[kb].w, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) S[(4 * g + q) * lds_s + kt * 16 + r16] = (acc[q] + acc1[q]) * A.scale;
    }
    __syncthreads();

    // ---- 2. softmax rows 2*wave, 2*wave + 1: normalised in place, zeros from the causal limit to T ----
    const int live_end = P + lens[b];               // first row past the item's end
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int r = 2 * wave + rr;
        const int t = t0 + r;
        const int lim = t < min(T, live_end) ? t + 1 : 0;      // keys [0, lim); 0: a row past the end (or past T: never stored)
        float* sr = S + r * lds_s;
        float mx = -INFINITY;
        for (int k = lane; k < lim; k += 64) mx = fmaxf(mx, sr[k]);
        mx = wave_max(mx);
        float sum = 0.f;
        for (int k = lane; k < lim; k += 64) {
            const float pr = expf(sr[k] - mx);
            sr[k] = pr;
            sum += pr;
        }
        sum = wave_sum(sum);
        for (int k = lane; k < T; k += 64) sr[k] = k < lim ? sr[k] / sum : 0.f;
    }
    __syncthreads();

    // ---- 3. the tile's span of out[b][h] ----
    const int nrows = min(16, T - t0);
    const int total = nrows * T;
    float* dst = out + (((size_t)b * gridDim.y + h) * T + t0) * (size_t)T;
    const int head = min(total, (int)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3));
    const int nvec = (total - head) >> 2;
    auto at = [&](int e) { const int r = e / T; return S[r * lds_s + (e - r * T)]; };
    if (tid < head) dst[tid] = at(tid);
    for (int j = tid; j < nvec; j += 512) {
        const int e = head + 4 * j;
        *reinterpret_cast<float4*>(dst + e) = make_float4(at(e), at(e + 1), at(e + 2), at(e + 3));
    }
    const int e_tail = head + 4 * nvec + tid;
    if (e_tail < total) dst[e_tail] = at(e_tail);
}

static inline int launch_attention_probs(int head_dim, int n_head, const AttnArgs& A, int batch, const int32_t* lens, int P, float* out,
                                         hipStream_t s) {
    const int nkp = (A.T + 15) & ~15;
    const size_t lds = (size_t)16 * (nkp + 4) * sizeof(float);
    GVC_REQUIRE(lds <= 160 * 1024, GVC_ERR_ARG, "trace: %d rows per item exceed the attention-weight tile's LDS", A.T);
    const dim3 grid((A.T + 15) / 16, n_head, batch);
#define GVC_ATT_PROBS(hd)                                                                                                         \
    {                                                                                                                             \
        static bool attr = false;                                                                                                 \
        if (!attr) {                                                                                                              \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_probs<hd>),                                     \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                                   \
            attr = true;                                                                                                          \
        }                                                                                                                         \
        hipLaunchKernelGGL((k_attention_probs<hd>), grid, dim3(512), lds, s, A, nkp, lens, P, out);                              \
    }
    if (head_dim == 256) GVC_ATT_PROBS(256)
    else if (head_dim == 128) GVC_ATT_PROBS(128)
    else if (head_dim == 64) GVC_ATT_PROBS(64)
    else {
        set_error("trace: head_dim %d unsupported (64, 128 or 256)", head_dim);
        return GVC_ERR_UNSUPPORTED;
    }
#undef GVC_ATT_PROBS
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// Hidden-state tap: rows of src [B][T][d] -> dst [B][T][d]; with w / bias the LayerNorm of the row (k_ln_rows' arithmetic: ln_f for the
// last plane), else a copy; rows at or past the item's end (t >= P + lens[b]) are zeros.  One wave per row, 4 rows per workgroup.
__global__ void k_trace_hidden(const float* src, float* dst, int B, int T, int d, const int32_t* lens, int P, const float* w,
                               const float* bias) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= B * T) return;
    const int b = row / T, t = row - b * T;
    const float* x = src + (size_t)row * d;
    float* y = dst + (size_t)row * d;
    if (t >= P + lens[b]) {
        for (int k = lane * 4; k < d; k += 256) *reinterpret_cast<float4*>(y + k) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    if (!w) {
        for (int k = lane * 4; k < d; k += 256) *reinterpret_cast<float4*>(y + k) = *reinterpret_cast<const float4*>(x + k);
        return;
    }
    const float inv_d = 1.0f / (float)d;
    float s = 0.f;
    for (int k = lane * 4; k < d; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + k);
        s += (v.x + v.y) + (v.z + v.w);
    }
    const float mean = wave_sum(s) * inv_d;
    float q = 0.f;
    for (int k = lane * 4; k < d; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + k);
        const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
        q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_d + 1e-5f);
    for (int k = lane * 4; k < d; k += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + k);
        const float4 gw = *reinterpret_cast<const float4*>(w + k);
        const float4 c = *reinterpret_cast<const float4*>(bias + k);
        v.x = (v.x - mean) * rstd * gw.x + c.x; v.y = (v.y - mean) * rstd * gw.y + c.y;
        v.z = (v.z - mean) * rstd * gw.z + c.z; v.w = (v.w - mean) * rstd * gw.w + c.w;
        *reinterpret_cast<float4*>(y + k) = v;
    }
}

// Alignment map: align[b][i][c] (+)= sum over the heads, in head order, of probs[b][h][P + i][c0 + c] of one layer; the launch of the
// last chosen layer multiplies by `inv` = 1 / (heads * chosen layers).  One thread per output element, the layers' launches in layer
// order on one stream: a fixed summation order, no atomics.
__global__ void k_trace_align(const float* probs, float* align, int B, int H, int T, int P, int n, int c0, int Tc, int first, float inv) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * n * Tc) return;
    const int c = idx % Tc, i = (idx / Tc) % n, b = idx / (Tc * n);
    float acc = first ? 0.f : align[idx];
    for (int h = 0; h < H; ++h) acc += probs[(((size_t)b * H + h) * T + P + i) * (size_t)T + c0 + c];
    align[idx] = inv != 0.f ? acc * inv : acc;
}

}  // namespace gvc
