// Sequence log-probabilities of generated tokens under the raw model distribution (include/genvc_hip.h: gvc_gpt_sequence_logprobs):
// logits = mel_head(latents) by the fp32 GEMM into the caller's scratch, then one row kernel per sequence.
#pragma once
#include "common.h"

namespace gvc {

// R sequences of n steps: latents [R][n][d] (contiguous), tokens [R][tok_stride] -> logprob [R] (double), length [R]; tok_lp (nullable)
// [R][n] the per-token terms (0 past the length).  head_w [vocab][d], head_b [vocab]; scratch holds scratch_floats floats (the logits of
// as many whole sequences as fit, and the GEMM's split-K planes).  No allocation, no synchronisation
int launch_sequence_logprobs(const float* latents, const int32_t* tokens, int tok_stride, int R, int n, int d, int vocab, int eos,
                             const float* head_w, const float* head_b, float* scratch, long long scratch_floats, double* logprob,
                             int32_t* length, float* tok_lp, hipStream_t s);

}  // namespace gvc
