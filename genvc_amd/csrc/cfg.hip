// Classifier-free guidance: the combine step of transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__
// (generation/logits_process.py):
//     scores = log_softmax(scores, dim=-1)
//     unconditional_logits = log_softmax(logits[:, -1], dim=-1)
//     scores_processed = guidance_scale * (scores - unconditional_logits) + unconditional_logits
// restated on the device.  One workgroup per item, both rows staged in LDS.
#include "cfg.h"

namespace gvc {

// max of (a, b) over the workgroup, the same bits in every thread: xor butterfly inside the wave, the four wave results through scr[8]
__device__ __forceinline__ void cfg_block_max2(float& a, float& b, float* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a = fmaxf(a, __shfl_xor(a, off)); b = fmaxf(b, __shfl_xor(b, off)); }
    __syncthreads();
    if (lane == 0) { scr[wave] = a; scr[4 + wave] = b; }
    __syncthreads();
    a = fmaxf(fmaxf(scr[0], scr[1]), fmaxf(scr[2], scr[3]));
    b = fmaxf(fmaxf(scr[4], scr[5]), fmaxf(scr[6], scr[7]));
}

// sum of (a, b) over the workgroup in a fixed order (the same row gives the same bits on every run): see block_sum2 of sampler.hip
__device__ __forceinline__ void cfg_block_sum2(float& a, float& b, float* scr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    __syncthreads();
    if (lane == 0) { scr[wave] = a; scr[4 + wave] = b; }
    __syncthreads();
    a = ((scr[0] + scr[1]) + scr[2]) + scr[3];
    b = ((scr[4] + scr[5]) + scr[6]) + scr[7];
}

__global__ __launch_bounds__(kCfgThreads) void k_cfg_guide(const float* cond, const float* uncond, int vocab, float scale,
                                                           const float* scale_dev, float* guided) {
    __shared__ float lc[kCfgMaxVocab];
    __shared__ float lu[kCfgMaxVocab];
    __shared__ float scr[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float s = scale_dev ? *scale_dev : scale;
    const float* c = cond + (size_t)b * vocab;
    const float* u = uncond + (size_t)b * vocab;
    float mc = -INFINITY, mu = -INFINITY;
    for (int i = tid; i < vocab; i += kCfgThreads) {
        const float x = c[i], y = u[i];
        lc[i] = x; lu[i] = y;
        mc = fmaxf(mc, x); mu = fmaxf(mu, y);
    }
    cfg_block_max2(mc, mu, scr);
    // the max comes off before exp: every term lies in (0, 1], the sum in [1, vocab], for finite inputs of any range
    float zc = 0.f, zu = 0.f;
    for (int i = tid; i < vocab; i += kCfgThreads) {       // (a thread reads back only what it staged itself)
        zc += expf(lc[i] - mc);
        zu += expf(lu[i] - mu);
    }
    cfg_block_sum2(zc, zu, scr);
    const float lzc = logf(zc), lzu = logf(zu);
    float* o = guided + (size_t)b * vocab;
    for (int i = tid; i < vocab; i += kCfgThreads) {
        const float pc = (lc[i] - mc) - lzc;                 // log_softmax as torch evaluates it: x - max - log(sum)
        const float pu = (lu[i] - mu) - lzu;
        // HF's operation order, every step rounded on its own (no contraction into an fma)
        o[i] = __fadd_rn(__fmul_rn(s, __fsub_rn(pc, pu)), pu);
    }
}

__global__ void k_cfg_mirror(int32_t* tok, int B) {
    if ((int)threadIdx.x < B) tok[B + threadIdx.x] = tok[threadIdx.x];
}

__global__ void k_cfg_begin(int32_t* slot_table, const int32_t* uncond_slots, int B, float scale, float* scale_dev, float* logits,
                            const float* slot_logits, int vocab, float* latent, const float* slot_latent, int d) {
    const int b = blockIdx.x;
    const size_t sl = (size_t)uncond_slots[b];
    if (threadIdx.x == 0) {
        slot_table[B + b] = (int32_t)sl;
        if (b == 0) *scale_dev = scale;
    }
    for (int i = threadIdx.x; i < vocab; i += blockDim.x) logits[(size_t)(B + b) * vocab + i] = slot_logits[sl * vocab + i];
    for (int i = threadIdx.x; i < d; i += blockDim.x) latent[(size_t)(B + b) * d + i] = slot_latent[sl * d + i];
}

int launch_cfg_guide(const float* cond, const float* uncond, int B, int vocab, float scale, const float* scale_dev, float* guided,
                     hipStream_t s) {
    GVC_REQUIRE(vocab >= 1 && vocab <= kCfgMaxVocab, GVC_ERR_UNSUPPORTED, "cfg_guide: vocab %d outside [1, %d]", vocab, kCfgMaxVocab);
    hipLaunchKernelGGL(k_cfg_guide, dim3(B), dim3(kCfgThreads), 0, s, cond, uncond, vocab, scale, scale_dev, guided);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_cfg_mirror(int32_t* tok, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_cfg_mirror, dim3(1), dim3(64), 0, s, tok, B);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

int launch_cfg_begin(int32_t* slot_table, const int32_t* uncond_slots, int B, float scale, float* scale_dev, float* logits,
                     const float* slot_logits, int vocab, float* latent, const float* slot_latent, int d, hipStream_t s) {
    hipLaunchKernelGGL(k_cfg_begin, dim3(B), dim3(256), 0, s, slot_table, uncond_slots, B, scale, scale_dev, logits, slot_logits, vocab,
                       latent, slot_latent, d);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc

using namespace gvc;

extern "C" int gvc_cfg_guide(const float* logits_cond, const float* logits_uncond, int32_t B, int32_t vocab, float scale, float* out,
                             gvc_stream sv) {
    GVC_REQUIRE(logits_cond && logits_uncond && out && B >= 1, GVC_ERR_ARG, "gvc_cfg_guide: bad argument");
    GVC_REQUIRE(scale == scale && fabsf(scale) <= 3.0e38f, GVC_ERR_ARG, "gvc_cfg_guide: scale is not finite");
    return launch_cfg_guide(logits_cond, logits_uncond, B, vocab, scale, nullptr, out, (hipStream_t)sv);
}
