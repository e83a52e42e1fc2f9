// Stand-alone host check of the watermark's table indexing and argument checks (genvc_amd/csrc/watermark.h), meant to run under the
// host sanitizers:
//     hipcc -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Igenvc_amd/csrc scripts/wm_host_check.cpp -o wm_host_check
//     (or: c++ -std=c++17 -fsanitize=address,undefined -Igenvc_amd/csrc scripts/wm_host_check.cpp -o wm_host_check)
// It builds tables of the exact sizes the library indexes (no slack), sets and reads every bit through wm_word_at / wm_mask, restates
// the detector's counting loop on the host, and walks the argument checks over their edges.  No GPU is touched.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "watermark.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

using namespace gvc;

static void tables(int vocab) {
    const int words = wm_words(vocab);
    CHECK(words * 32 >= vocab && (words - 1) * 32 < vocab);
    // lefthash: vocab rows of exactly `words` words; every (prev, i) lands inside, once
    std::vector<uint32_t> left((size_t)vocab * words, 0u);
    for (int prev = 0; prev < vocab; ++prev)
        for (int i = 0; i < vocab; ++i) {
            const long long at = wm_word_at(0, prev, i, words, vocab);
            CHECK(at >= 0 && at < (long long)left.size());
            CHECK(!(left[(size_t)at] & wm_mask(i)));
            if ((prev * 31 + i) % 3 == 0) left[(size_t)at] |= wm_mask(i);
        }
    for (int prev = 0; prev < vocab; ++prev)
        for (int i = 0; i < vocab; ++i)
            CHECK(((left[(size_t)wm_word_at(0, prev, i, words, vocab)] & wm_mask(i)) != 0) == ((prev * 31 + i) % 3 == 0));
    // selfhash: one row; prev is ignored, whatever it is
    std::vector<uint32_t> self((size_t)words, 0u);
    for (int i = 0; i < vocab; ++i) {
        const long long at = wm_word_at(1, std::numeric_limits<int>::min(), i, words, vocab);
        CHECK(at >= 0 && at < words && at == wm_word_at(1, std::numeric_limits<int>::max(), i, words, vocab));
        self[(size_t)at] |= wm_mask(i);
    }
    for (int w = 0; w < words; ++w) {
        const int in_word = vocab - 32 * w >= 32 ? 32 : vocab - 32 * w;
        CHECK(self[(size_t)w] == (in_word == 32 ? 0xffffffffu : (1u << in_word) - 1u));          // no bit past the vocabulary
    }
    // ids outside [0, vocab) index nothing
    const int outs[] = {-1, vocab, vocab + 1, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()};
    for (int o : outs) {
        CHECK(wm_word_at(0, o, 0, words, vocab) == -1 && wm_word_at(0, 0, o, words, vocab) == -1);
        CHECK(wm_word_at(1, 0, o, words, vocab) == -1);
    }
    // the detector's loop on the host, over codes with ids outside the vocabulary and a ragged length
    std::vector<int> codes;
    for (int t = 0; t < 300; ++t) codes.push_back((t * 7919) % (vocab + 3) - 1);
    const int len = 257;
    for (int scheme = 0; scheme < 2; ++scheme)
        for (int ignore = 0; ignore < 2; ++ignore) {
            int scored = 0, green = 0;
            for (int t = 0; t < (int)codes.size(); ++t) {
                if (t >= len || (scheme == 0 && t < 1)) continue;
                const int cur = codes[(size_t)t], prev = scheme == 1 ? 0 : codes[(size_t)t - 1];
                long long at = wm_word_at(scheme, prev, cur, words, vocab);
                if (at >= 0 && ignore)
                    for (int u = scheme == 1 ? 0 : 1; u < t; ++u)
                        if (codes[(size_t)u] == cur && (scheme == 1 || codes[(size_t)u - 1] == prev)) { at = -1; break; }
                if (at < 0) continue;
                const std::vector<uint32_t>& tb = scheme == 1 ? self : left;
                CHECK(at < (long long)tb.size());
                ++scored;
                green += (tb[(size_t)at] & wm_mask(cur)) ? 1 : 0;
            }
            CHECK((vocab < 32 || scored > 0) && green <= scored && scored <= len);
        }
}

static void checks() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    CHECK(wm_entry_ok(2.0f, 0, 33, 0, 1026, 33) && wm_entry_ok(-3.0e38f, 1, 33, 0, 1026, 33) && wm_entry_ok(0.0f, 0, 3, 0, 70, 33));
    CHECK(!wm_entry_ok(inf, 0, 33, 0, 1026, 33) && !wm_entry_ok(-inf, 0, 33, 0, 1026, 33) && !wm_entry_ok(nan, 0, 33, 0, 1026, 33));
    CHECK(!wm_entry_ok(2.0f, 2, 33, 0, 1026, 33) && !wm_entry_ok(2.0f, -1, 33, 0, 1026, 33));
    CHECK(!wm_entry_ok(2.0f, 0, 32, 0, 1026, 33) && !wm_entry_ok(2.0f, 0, 34, 0, 1026, 33) && !wm_entry_ok(2.0f, 0, 33, 1, 1026, 33));
    CHECK(!wm_entry_ok(2.0f, 0, 34, 0, 1060, 33) && !wm_entry_ok(2.0f, 0, 0, 0, 0, 33));
    CHECK(wm_score_args_ok(1, 1, 0, 33, 1026, 0) && wm_score_args_ok(8, kWmMaxScoreLen, 1, 33, 1026, 1));
    CHECK(!wm_score_args_ok(0, 8, 0, 33, 1026, 0) && !wm_score_args_ok(1, 0, 0, 33, 1026, 0));
    CHECK(!wm_score_args_ok(1, kWmMaxScoreLen + 1, 0, 33, 1026, 0) && !wm_score_args_ok(1, 8, 2, 33, 1026, 0));
    CHECK(!wm_score_args_ok(1, 8, 0, 32, 1026, 0) && !wm_score_args_ok(1, 8, 0, 33, 1026, 2) && !wm_score_args_ok(1, 8, 0, 0, 0, 0));
    CHECK(wm_words(1) == 1 && wm_words(32) == 1 && wm_words(33) == 2 && wm_words(1026) == 33 && wm_words(70) == 3);
}

int main() {
    tables(1026);
    tables(70);
    tables(32);
    tables(1);
    checks();
    std::puts("wm_host_check: ok");
    return 0;
}
