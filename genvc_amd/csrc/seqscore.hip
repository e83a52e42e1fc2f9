// gvc_gpt_sequence_logprobs: sum over a sequence's generated tokens of log_softmax(mel_head(latent))[token].  The generation loop's
// latents are final_norm(ln_f(h)), so mel_head of a step's latent is the logits row that step's token was chosen from: the score is
// that of the raw model distribution (no repetition penalty, processor or warper).
#include "seqscore.h"

#include "gemm.h"

namespace gvc {

// one workgroup per sequence; a wave per step (steps wave, wave + 4, ...): max, log-sum-exp with the accurate expf / logf, the chosen
// logit; the terms are summed in double, per wave in step order and over the four waves in wave order (the same sum on every run)
__global__ void __launch_bounds__(256) k_seq_logprob(const float* logits, const int32_t* tokens, int tok_stride, int n, int vocab, int eos,
                                                     double* logprob, int32_t* length, float* tok_lp) {
    __shared__ int s_len;
    __shared__ double s_part[4];
    const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t* tok = tokens + (size_t)r * tok_stride;
    if (tid == 0) s_len = n;
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x)
        if (tok[i] == eos) atomicMin(&s_len, i + 1);             // up to and including the first stop token
    __syncthreads();
    const int len = s_len;
    double acc = 0.0;
    for (int t = wave; t < len; t += 4) {
        const float* x = logits + ((size_t)r * n + t) * vocab;
        float m = -INFINITY;
        for (int i = lane; i < vocab; i += 64) m = fmaxf(m, x[i]);
        m = wave_max(m);
        float e = 0.f;
        for (int i = lane; i < vocab; i += 64) e += expf(x[i] - m);
        e = wave_sum(e);
        const int k = tok[t];
        const float lp = k >= 0 && k < vocab ? (x[k] - m) - logf(e) : __builtin_nanf("");
        acc += (double)lp;
        if (tok_lp && lane == 0) tok_lp[(size_t)r * n + t] = lp;
    }
    if (tok_lp)
        for (int i = len + tid; i < n; i += blockDim.x) tok_lp[(size_t)r * n + i] = 0.f;
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        logprob[r] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
        length[r] = len;
    }
}

int launch_sequence_logprobs(const float* latents, const int32_t* tokens, int tok_stride, int R, int n, int d, int vocab, int eos,
                             const float* head_w, const float* head_b, float* scratch, long long scratch_floats, double* logprob,
                             int32_t* length, float* tok_lp, hipStream_t s) {
    const long long half = scratch_floats / 2, per_seq = (long long)n * vocab;
    GVC_REQUIRE(per_seq <= half, GVC_ERR_ARG, "sequence_logprobs: %d steps x %d logits exceed the scratch (%lld floats)", n, vocab, half);
    const int chunk = (int)(half / per_seq < R ? half / per_seq : R);
    for (int r0 = 0; r0 < R; r0 += chunk) {
        const int Rc = R - r0 < chunk ? R - r0 : chunk;
        GemmArgs G;
        memset(&G, 0, sizeof(G));
        G.A = latents + (size_t)r0 * n * d; G.lda = d; G.Wt = head_w; G.ldw = d; G.C = scratch; G.ldc = vocab;
        G.M = Rc * n; G.N = vocab; G.K = d; G.work = scratch + half; G.e.bias = head_b;
        int rc = launch_gemm_cap(G, 1, half, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_seq_logprob, dim3(Rc), dim3(256), 0, s, scratch, tokens + (size_t)r0 * tok_stride, tok_stride, n, vocab, eos,
                           logprob + r0, length + r0, tok_lp ? tok_lp + (size_t)r0 * n : nullptr);
        GVC_LAUNCH_CHECK();
    }
    return GVC_OK;
}

}  // namespace gvc
