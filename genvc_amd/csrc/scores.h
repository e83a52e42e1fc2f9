// Transition scores on the device (include/genvc_hip.h: gvc_transition_scores): transformers' GenerationMixin.compute_transition_scores
// without beams -- the score of every generated token, gathered from the per-step scores a gvc_gpt_generate_scores call stored,
// optionally behind a log_softmax over the row.
#pragma once
#include "common.h"

namespace gvc {

constexpr int kScoreThreads = 256;

// out[r][t] = scores[r][t][tokens[r][t]] (normalize == 0) or log_softmax(scores[r][t])[tokens[r][t]] (normalize == 1), fp32; one
// workgroup per (r, t).  scores: row r starts at scores + r * row_stride floats and holds n dense [V] rows; tokens / out: dense [R][n].
// A token outside [0, V) gives NaN
int launch_transition_scores(const float* scores, long long row_stride, const int32_t* tokens, int R, int n, int V, int normalize,
                             float* out, hipStream_t s);

}  // namespace gvc
