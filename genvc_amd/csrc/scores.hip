// transformers' GenerationMixin.compute_transition_scores without beams (generation/utils.py):
//     scores = torch.stack(scores)                                   # [n, R, V] -> here [R, n, V]
//     if normalize_logits: scores = log_softmax(scores, dim=vocabulary)
//     transition_scores = scores.gather(vocabulary, sequences[:, -n:])
// restated on the device.  One workgroup per (row, step).
#include "scores.h"

namespace gvc {

// max of v over the workgroup, the same bits in every thread: xor butterfly inside the wave, the four wave results through scr[4]
__device__ __forceinline__ float score_block_max(float v, float* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    __syncthreads();
    if (lane == 0) scr[wave] = v;
    __syncthreads();
    return fmaxf(fmaxf(scr[0], scr[1]), fmaxf(scr[2], scr[3]));
}

// sum of v over the workgroup in a fixed order (the same row gives the same bits on every run): see cfg_block_sum2 of cfg.hip
__device__ __forceinline__ float score_block_sum(float v, float* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if (lane == 0) scr[wave] = v;
    __syncthreads();
    return ((scr[0] + scr[1]) + scr[2]) + scr[3];
}

__global__ __launch_bounds__(kScoreThreads) void k_transition_scores(const float* scores, long long row_stride, const int32_t* tokens,
                                                                     int n, int V, int normalize, float* out) {
    __shared__ float scr[4];
    const int r = blockIdx.x / n, t = blockIdx.x % n, tid = threadIdx.x;
    const float* row = scores + (size_t)r * (size_t)row_stride + (size_t)t * V;
    const size_t at = (size_t)r * n + t;
    const int tok = tokens[at];
    const bool valid = tok >= 0 && tok < V;
    if (!normalize) {
        if (tid == 0) out[at] = valid ? row[tok] : NAN;
        return;
    }
    // log_softmax as torch evaluates it: x - max - log(sum exp(x - max)); a -inf entry adds exp(-inf) = 0
    float m = -INFINITY;
    for (int i = tid; i < V; i += kScoreThreads) m = fmaxf(m, row[i]);
    m = score_block_max(m, scr);
    float z = 0.f;
    for (int i = tid; i < V; i += kScoreThreads) z += expf(row[i] - m);
    z = score_block_sum(z, scr);
    if (tid == 0) out[at] = valid ? (row[tok] - m) - logf(z) : NAN;
}

int launch_transition_scores(const float* scores, long long row_stride, const int32_t* tokens, int R, int n, int V, int normalize,
                             float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_transition_scores, dim3((unsigned)(R * n)), dim3(kScoreThreads), 0, s, scores, row_stride, tokens, n, V, normalize,
                       out);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc

extern "C" int gvc_transition_scores(const float* scores, int64_t row_stride, const int32_t* tokens, int32_t R, int32_t n, int32_t V,
                                     int32_t normalize, float* out, gvc_stream sv) {
    GVC_REQUIRE(scores && tokens && out, GVC_ERR_ARG, "gvc_transition_scores: null argument");
    GVC_REQUIRE(R >= 1 && n >= 1 && V >= 1 && (long long)R * n <= 0x7fffffffLL, GVC_ERR_ARG,
                "gvc_transition_scores: bad shape [%d, %d, %d]", R, n, V);
    GVC_REQUIRE(row_stride >= (int64_t)n * V, GVC_ERR_ARG, "gvc_transition_scores: row stride %lld below n * V = %lld",
                (long long)row_stride, (long long)n * V);
    GVC_REQUIRE(normalize == 0 || normalize == 1, GVC_ERR_ARG, "gvc_transition_scores: normalize must be 0 or 1, not %d", normalize);
    return gvc::launch_transition_scores(scores, row_stride, tokens, R, n, V, normalize, out, (hipStream_t)sv);
}
