// Green-list watermark (include/genvc_hip.h: gvc_logits_watermark, gvc_wm_score): the table indexing and the argument checks, in plain
// C++ that host code, the sampler kernels and the detector kernel share.  Nothing here needs the HIP runtime: scripts/wm_host_check.cpp
// exercises it stand-alone under the host sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GVC_WM_HD __host__ __device__
#else
#define GVC_WM_HD
#endif

namespace gvc {

constexpr int kWmMaxScoreLen = 8192;           // gvc_wm_score: codes per row

// words of one table row
GVC_WM_HD inline int wm_words(int vocab) { return (vocab + 31) >> 5; }

// word offset of the bit (prev, i) in a lefthash table, of the bit i in a selfhash table (prev ignored); -1 when an id lies outside
// [0, vocab): such an n-gram is neither biased nor scored
GVC_WM_HD inline long long wm_word_at(int scheme, int prev, int i, int words, int vocab) {
    if (i < 0 || i >= vocab) return -1;
    if (scheme == 1) return i >> 5;
    if (prev < 0 || prev >= vocab) return -1;
    return (long long)prev * words + (i >> 5);
}
GVC_WM_HD inline uint32_t wm_mask(int i) { return 1u << (i & 31); }

// one entry of a watermark table: a finite bias (a NaN fails both comparisons), scheme 0 / 1, words == ceil(vocab / 32) <= max_words,
// reserved == 0
inline bool wm_entry_ok(float bias, int scheme, int words, int reserved, int vocab, int max_words) {
    return bias >= -3.4028234664e38f && bias <= 3.4028234664e38f && (scheme == 0 || scheme == 1) && vocab >= 1 &&
           words == wm_words(vocab) && words <= max_words && reserved == 0;
}

// the shape of a gvc_wm_score call
inline bool wm_score_args_ok(int B, int n, int scheme, int words, int vocab, int ignore_repeated) {
    return B >= 1 && n >= 1 && n <= kWmMaxScoreLen && (scheme == 0 || scheme == 1) && vocab >= 1 && words == wm_words(vocab) &&
           (ignore_repeated == 0 || ignore_repeated == 1);
}

}  // namespace gvc
