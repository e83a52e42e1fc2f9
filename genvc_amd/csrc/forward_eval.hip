// Kernels of the GPT.forward evaluation pass (forward_eval.h; reference layers/gpt.py:375-537).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"
#include "gpt_kernels.h"
#include "forward_eval.h"

namespace gvc {

__global__ void k_eval_embed(float* x, const float* cond, int n_cond, const int32_t* text_ids, int Lt, const int32_t* code_ids, int Lm, int d,
                             const float* text_emb, const float* text_pos, int n_text, const float* mel_emb, const float* mel_pos, int vocab) {
    const int T = n_cond + Lt + Lm;
    const int b = blockIdx.x / T, t = blockIdx.x - b * T;
    float4* dst = reinterpret_cast<float4*>(x + (size_t)blockIdx.x * d);
    if (t < n_cond) {
        const float4* src = reinterpret_cast<const float4*>(cond + ((size_t)b * n_cond + t) * d);
        for (int k = threadIdx.x; k < d / 4; k += blockDim.x) dst[k] = src[k];
        return;
    }
    const bool text = t < n_cond + Lt;
    const int i = text ? t - n_cond : t - n_cond - Lt;
    const int id = text ? text_ids[(size_t)b * Lt + i] : code_ids[(size_t)b * Lm + i];
    const int idc = min(max(id, 0), (text ? n_text : vocab) - 1);
    const float4* e = reinterpret_cast<const float4*>((text ? text_emb : mel_emb) + (size_t)idc * d);
    const float4* p = reinterpret_cast<const float4*>((text ? text_pos : mel_pos) + (size_t)i * d);
    for (int k = threadIdx.x; k < d / 4; k += blockDim.x) {
        const float4 a = e[k], c = p[k];
        dst[k] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
}

int launch_eval_embed(float* x, const float* cond, int n_cond, const int32_t* text_ids, int Lt, const int32_t* code_ids, int Lm, int B, int d,
                      const float* text_emb, const float* text_pos, int n_text, const float* mel_emb, const float* mel_pos, int vocab,
                      hipStream_t s) {
    hipLaunchKernelGGL(k_eval_embed, dim3(B * (n_cond + Lt + Lm)), dim3(256), 0, s, x, cond, n_cond, text_ids, Lt, code_ids, Lm, d, text_emb,
                       text_pos, n_text, mel_emb, mel_pos, vocab);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

__global__ void k_eval_gather(const float* src, float* dst, int T, int off, int n, int d) {
    const int b = blockIdx.x / n, i = blockIdx.x - b * n;
    const float4* s4 = reinterpret_cast<const float4*>(src + ((size_t)b * T + off + i) * d);
    float4* d4 = reinterpret_cast<float4*>(dst + (size_t)blockIdx.x * d);
    for (int k = threadIdx.x; k < d / 4; k += blockDim.x) d4[k] = s4[k];
}

int launch_eval_gather(const float* src, float* dst, int B, int T, int off, int n, int d, hipStream_t s) {
    hipLaunchKernelGGL(k_eval_gather, dim3(B * n), dim3(256), 0, s, src, dst, T, off, n, d);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_attention_tile_masked(int head_dim, int n_head, const AttnArgs& A, int batch, int max_keys, hipStream_t s) {
    GVC_REQUIRE(A.key_mask && A.mask_stride >= max_keys && !A.base_len && A.causal, GVC_ERR_ARG,
                "masked attention: a causal pass without cached keys and a mask row of at least %d keys", max_keys);
    GVC_REQUIRE(head_dim == 64 || head_dim == 128 || head_dim == 256, GVC_ERR_UNSUPPORTED, "masked attention: head_dim %d unsupported (64, 128 or 256)",
                head_dim);
    const int nkp = (max_keys + 15) & ~15;
    const dim3 grid((A.T + 15) / 16, n_head, batch);
    if (nkp <= 128) {
        const size_t lds_short = ((size_t)16 * 132 + 16 + (size_t)(128 + 16) * (head_dim + 4)) * sizeof(float);
#define GVC_ATT_SHORT_M(hd)                                                                                                          \
    {                                                                                                                                \
        static bool attr = false;                                                                                                    \
        if (!attr) {                                                                                                                 \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_tile_short<hd, 0, true>),                          \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                                      \
            attr = true;                                                                                                             \
        }                                                                                                                            \
        hipLaunchKernelGGL((k_attention_tile_short<hd, 0, true>), grid, dim3(512), lds_short, s, A);                                \
    }
        if (head_dim == 256) GVC_ATT_SHORT_M(256) else if (head_dim == 128) GVC_ATT_SHORT_M(128) else GVC_ATT_SHORT_M(64)
#undef GVC_ATT_SHORT_M
        GVC_LAUNCH_CHECK();
        return GVC_OK;
    }
    const size_t lds = ((size_t)16 * (nkp + 4) + 16 + (size_t)64 * (head_dim + 4)) * sizeof(float);
    GVC_REQUIRE(lds <= 160 * 1024, GVC_ERR_UNSUPPORTED, "masked attention: %d keys exceed the score tile of the prefill attention", max_keys);
#define GVC_ATT_TILE_M(hd)                                                                                                           \
    {                                                                                                                                \
        static bool attr = false;                                                                                                    \
        if (!attr) {                                                                                                                 \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_tile<hd, 0, 64, true>),                            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                                      \
            attr = true;                                                                                                             \
        }                                                                                                                            \
        hipLaunchKernelGGL((k_attention_tile<hd, 0, 64, true>), grid, dim3(512), lds, s, A, nkp);                                   \
    }
    if (head_dim == 256) GVC_ATT_TILE_M(256) else if (head_dim == 128) GVC_ATT_TILE_M(128) else GVC_ATT_TILE_M(64)
#undef GVC_ATT_TILE_M
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// one wave per logits row (V is no multiple of 64: the tail lanes of the last pass idle); every sum is a fixed lane-strided order
// followed by the wave butterfly, so a row's terms do not depend on the launch
__global__ void k_xent_rows(const float* logits, int ldl, const int32_t* targets, int R, int V, int top_k, float* row_terms) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= R) return;
    float* out = row_terms + (size_t)r * 3;
    const int t = targets[r];
    if (t < 0 || t >= V) {          // -1: ignored (anything else outside the row is a caller error and counts as ignored too)
        if (lane == 0) { out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; }
        return;
    }
    const float* x = logits + (size_t)r * ldl;
    const float xt = x[t];
    float mx = -INFINITY;
    for (int k = lane; k < V; k += 64) mx = fmaxf(mx, x[k]);
    mx = wave_max(mx);
    float se = 0.f, sx = 0.f, above = 0.f;
    for (int k = lane; k < V; k += 64) {
        const float v = x[k];
        se += expf(v - mx);
        sx += v;
        above += v > xt ? 1.f : 0.f;
    }
    se = wave_sum(se);
    sx = wave_sum(sx);
    above = wave_sum(above);
    if (lane == 0) {
        const float lse = mx + logf(se);
        out[0] = lse - xt;
        out[1] = lse - sx / (float)V;
        out[2] = above < (float)top_k ? 1.f : 0.f;
    }
}

// ONE workgroup: thread i sums rows i, i + 256, ... in double, then a fixed tree over the 256 partials
__global__ __launch_bounds__(256) void k_xent_reduce(const float* row_terms, const int32_t* targets, int R, int V, float label_smoothing,
                                                     double* sums) {
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    double nll = 0.0, sm = 0.0, hit = 0.0, cnt = 0.0;
    for (int r = tid; r < R; r += 256) {
        const int t = targets[r];
        if (t < 0 || t >= V) continue;
        nll += (double)row_terms[(size_t)r * 3];
        sm += (double)row_terms[(size_t)r * 3 + 1];
        hit += (double)row_terms[(size_t)r * 3 + 2];
        cnt += 1.0;
    }
    sh[0][tid] = nll; sh[1][tid] = sm; sh[2][tid] = hit; sh[3][tid] = cnt;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w)
            for (int j = 0; j < 4; ++j) sh[j][tid] += sh[j][tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double n = sh[3][0], ls = (double)label_smoothing;
        sums[0] = ((1.0 - ls) * sh[0][0] + ls * sh[1][0]) / n;
        sums[1] = sh[2][0];
        sums[2] = n;
        sums[3] = sh[0][0] / n;
    }
}

int launch_head_xent(const float* logits, int ldl, const int32_t* targets, int R, int V, float label_smoothing, int top_k, float* row_terms,
                     double* sums, hipStream_t s) {
    hipLaunchKernelGGL(k_xent_rows, dim3(cdiv(R, 4)), dim3(256), 0, s, logits, ldl, targets, R, V, top_k, row_terms);
    GVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_xent_reduce, dim3(1), dim3(256), 0, s, row_terms, targets, R, V, label_smoothing, sums);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

__global__ void k_mask_excluded(const uint8_t* key_mask, int32_t* excluded, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) excluded[i] = key_mask[i] == 0 ? 1 : 0;
}

int launch_mask_excluded(const uint8_t* key_mask, int32_t* excluded, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_excluded, dim3(cdiv(n, 256)), dim3(256), 0, s, key_mask, excluded, n);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc
