// Classifier-free guidance on the device (include/genvc_hip.h: gvc_cfg_guide, gvc_gpt_generate_cfg): the combine step of HF's
// UnbatchedClassifierFreeGuidanceLogitsProcessor and the token mirror of the guided generation loop.  The step graph that chains them
// with the sampler and the decode step over 2B rows lives in gpt.hip.
#pragma once
#include "common.h"

namespace gvc {

constexpr int kCfgThreads = 256;
constexpr int kCfgMaxVocab = 2048;      // both rows of an item are staged in LDS (the sampler's bound: kSortN)

// guided[b][v] = scale * (lsm(cond[b])[v] - lsm(uncond[b])[v]) + lsm(uncond[b])[v], lsm = log_softmax over the vocabulary, fp32, in
// HF's operation order; one workgroup per item.  vocab <= kCfgMaxVocab (the callers check)
// scale_dev (nullable, device memory) takes the place of scale: a captured launch is independent of the call's scale
int launch_cfg_guide(const float* cond, const float* uncond, int B, int vocab, float scale, const float* scale_dev, float* guided,
                     hipStream_t s);
// tok[B + b] = tok[b]: the unconditional row of item b decodes the token chosen for the item
int launch_cfg_mirror(int32_t* tok, int B, hipStream_t s);
// start of a guided call, behind the begin launch of the B conditional rows: slot_table[B + b] = uncond_slots[b], *scale_dev = scale,
// and the parked next-step logits and latent of those slots go to rows B..2B-1 of the staging buffers
int launch_cfg_begin(int32_t* slot_table, const int32_t* uncond_slots, int B, float scale, float* scale_dev, float* logits,
                     const float* slot_logits, int vocab, float* latent, const float* slot_latent, int d, hipStream_t s);

}  // namespace gvc
