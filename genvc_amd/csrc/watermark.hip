// The detector's counts of the green-list watermark (include/genvc_hip.h: gvc_wm_score): transformers' WatermarkDetector
// (_score_ngrams_in_passage with context_width 1) restated on the device.  One workgroup per row of codes; integer arithmetic only.
#include "common.h"
#include "watermark.h"

namespace gvc {

constexpr int kWmThreads = 256;

__global__ __launch_bounds__(kWmThreads) void k_wm_score(const int32_t* codes, const int32_t* lens, int n, const uint32_t* table,
                                                         int scheme, int words, int vocab, int ignore_repeated, int32_t* counts,
                                                         uint8_t* flags) {
    __shared__ int s_scored, s_green;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t* row = codes + (size_t)b * n;
    uint8_t* fl = flags + (size_t)b * n;
    const int len = lens ? min(max(lens[b], 0), n) : n;
    if (tid == 0) { s_scored = 0; s_green = 0; }
    __syncthreads();
    int scored = 0, green = 0;
    for (int t = tid; t < n; t += kWmThreads) {
        int flag = 2;
        // lefthash scores position t >= 1 with (codes[t-1], codes[t]); selfhash scores every position with codes[t] alone
        if (t < len && (scheme == GVC_WM_SELFHASH || t >= 1)) {
            const int cur = row[t], prev = scheme == GVC_WM_SELFHASH ? 0 : row[t - 1];
            long long at = wm_word_at(scheme, prev, cur, words, vocab);          // (-1: an id outside the vocabulary)
            if (at >= 0 && ignore_repeated) {
                // an n-gram counts at its first occurrence: an earlier one has the same ids, so it was scored
                for (int u = scheme == GVC_WM_SELFHASH ? 0 : 1; u < t; ++u)
                    if (row[u] == cur && (scheme == GVC_WM_SELFHASH || row[u - 1] == prev)) { at = -1; break; }
            }
            if (at >= 0) {
                flag = (table[at] & wm_mask(cur)) ? 1 : 0;
                ++scored;
                green += flag;
            }
        }
        fl[t] = (uint8_t)flag;
    }
    if (scored) atomicAdd(&s_scored, scored);          // (integer adds: any order, the same counts)
    if (green) atomicAdd(&s_green, green);
    __syncthreads();
    if (tid == 0) { counts[2 * b] = s_scored; counts[2 * b + 1] = s_green; }
}

}  // namespace gvc

extern "C" int gvc_wm_score(const int32_t* codes, const int32_t* lens, int32_t B, int32_t n, const uint32_t* table, int32_t scheme,
                            int32_t words, int32_t vocab, int32_t ignore_repeated, int32_t* counts, uint8_t* flags, gvc_stream sv) {
    GVC_REQUIRE(codes && table && counts && flags, GVC_ERR_ARG, "gvc_wm_score: null argument");
    GVC_REQUIRE(gvc::wm_score_args_ok(B, n, scheme, words, vocab, ignore_repeated), GVC_ERR_ARG,
                "gvc_wm_score: B %d (>= 1), n %d (1..%d), scheme %d (0 / 1), words %d (ceil(vocab %d / 32)), ignore_repeated %d (0 / 1)", B, n,
                gvc::kWmMaxScoreLen, scheme, words, vocab, ignore_repeated);
    hipLaunchKernelGGL(gvc::k_wm_score, dim3((unsigned)B), dim3(gvc::kWmThreads), 0, (hipStream_t)sv, codes, lens, n, table, scheme, words,
                       vocab, ignore_repeated, counts, flags);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}
