// Mel inversion and Griffin-Lim (reference utils.py:164-172 -> torchaudio.transforms.InverseMelScale, then librosa.griffinlim with its
// defaults: momentum 0.99, random start, centre=True, zero ("constant") padding).
//
// k_gl_inverse_mel: S = relu(W exp(mel * norms)), W = fb (fb^T fb)^-1 the minimum-norm inverse of the mel filterbank, built on the host in
//   double (Cholesky of the n_mels x n_mels Gram matrix) -- what torch.linalg.lstsq(driver="gels") returns for a full-rank fb^T.
// k_gl_synth:  one workgroup per (frame, item): half spectrum S * angles -> inverse FFT in LDS -> windowed frame [win].
// k_gl_iter:   one workgroup per (frame, item): every sample of the frame's window is gathered from the overlapping stored frames in
//   ascending frame order, divided by the window envelope and zeroed outside the kept range (the reference trims n_fft / 2 per side and
//   pads with zeros again); window, forward FFT, angles = normalise(rebuilt - alpha * tprev), tprev = rebuilt; then the synthesis of the
//   SAME frame for the next iteration into the other frame buffer.  A frame's angles depend on that frame's rebuilt column alone, so the
//   analysis and the next synthesis are one launch and the angles never leave the workgroup.
// k_gl_output: the same gather into wav.
// No atomics and a fixed summation order everywhere: the same input gives the same bits.  n_iter + 2 launches per gvc_gl_run.
// The FFT is the in-LDS radix-2 decimation-in-time transform of mel.hip with two stages per LDS round trip, the log2 size a template
// argument and the conjugate twiddles for the inverse.
#include <float.h>
#include <math.h>

#include <vector>

#include "common.h"

namespace gvc {

constexpr int kGlThreads = 256;

struct GlDev {
    int n_fft, hop, win, n_freq, n_mels, woff;   // woff: first sample of the window inside the n_fft frame
    const float* window;      // [win] periodic Hann
    const float2* twiddle;    // [n_fft/2]  exp(-2 pi i k / n_fft)
    const float* wt;          // [n_mels][n_freq]: W transposed (threads run over the bins)
    const float* norms;       // [n_mels]
};

// the generator of the sampler (sample_body.h: rng_uniform; oracle/genvc_oracle.py:rng_uniform) keyed by (seed, item, (bin, frame))
__device__ __forceinline__ double gl_uniform(uint64_t seed, uint64_t item, uint64_t bin, uint64_t frame) {
    const uint64_t row = (bin << 32) | frame;
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + item * 0xBF58476D1CE4E5B9ull + row * 0x94D049BB133111EBull + 0x2545F4914F6CDD1Dull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 40) * (1.0 / 16777216.0);
}

// angles [B][n_freq][F] = exp(2 pi i u): evaluated in double and rounded once, so |angle| is 1 to half an ulp per component
__global__ __launch_bounds__(kGlThreads) void k_gl_init_angles(uint64_t seed, int n_freq, int F, long long total, float2* angles) {
    const long long i = (long long)blockIdx.x * kGlThreads + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % F);
    const int k = (int)((i / F) % n_freq);
    const long long b = i / ((long long)F * n_freq);
    double s, c;
    sincospi(2.0 * gl_uniform(seed, (uint64_t)b, (uint64_t)k, (uint64_t)t), &s, &c);
    angles[i] = make_float2((float)c, (float)s);
}

// S[b][k][t0 + i] = relu(sum_m W[k][m] exp(mel[b][m][t0 + i] norms[m])), m ascending; one workgroup per (tile of kGlTile frames, item)
constexpr int kGlTile = 8;
__global__ __launch_bounds__(kGlThreads) void k_gl_inverse_mel(const GlDev G, const float* mel, int F, float* spec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [n_mels][kGlTile]
    const int t0 = blockIdx.x * kGlTile, b = blockIdx.y, tid = threadIdx.x;
    const float* x = mel + (size_t)b * G.n_mels * F;
    for (int i = tid; i < G.n_mels * kGlTile; i += kGlThreads) {
        const int m = i / kGlTile, t = t0 + i % kGlTile;
        lds[i] = t < F ? expf(x[(size_t)m * F + t] * G.norms[m]) : 0.f;
    }
    __syncthreads();
    for (int k = tid; k < G.n_freq; k += kGlThreads) {
        float acc[kGlTile];
#pragma unroll
        for (int i = 0; i < kGlTile; ++i) acc[i] = 0.f;
        for (int m = 0; m < G.n_mels; ++m) {
            const float w = G.wt[(size_t)m * G.n_freq + k];
#pragma unroll
            for (int i = 0; i < kGlTile; ++i) acc[i] = fmaf(w, lds[m * kGlTile + i], acc[i]);
        }
        float* o = spec + ((size_t)b * G.n_freq + k) * F + t0;
#pragma unroll
        for (int i = 0; i < kGlTile; ++i)
            if (t0 + i < F) o[i] = fmaxf(acc[i], 0.f);
    }
}

// in-LDS decimation-in-time FFT of 2^LOG2N points: input at the bit-reversed index, output in natural order.  The radix-2 stages of
// mel.hip, taken two at a time in registers (four points per work item: half the LDS round trips and barriers; the loop is bound by LDS
// traffic), after one single stage where LOG2N is odd.  INVERSE uses the conjugate twiddles and leaves the 1 / n to the caller.  Ends
// with a barrier.
template <bool INVERSE>
__device__ __forceinline__ float2 gl_twiddle(const float2* twiddle, int i) {
    float2 w = twiddle[i];
    if (INVERSE) w.y = -w.y;
    return w;
}

// (a, b) <- (a + w b, a - w b)
__device__ __forceinline__ void gl_butterfly(float2& a, float2& b, const float2 w) {
    const float tr = b.x * w.x - b.y * w.y;
    const float ti = b.x * w.y + b.y * w.x;
    b = make_float2(a.x - tr, a.y - ti);
    a = make_float2(a.x + tr, a.y + ti);
}

template <int LOG2N, bool INVERSE>
__device__ __forceinline__ void gl_fft(float* re, float* im, const float2* twiddle) {
    constexpr int half_n = 1 << (LOG2N - 1);
    const int tid = threadIdx.x;
    if (LOG2N & 1) {                                   // stage 0 alone: neighbours, twiddle 1
        for (int j = tid; j < half_n; j += kGlThreads) {
            const float ar = re[2 * j], ai = im[2 * j], br = re[2 * j + 1], bi = im[2 * j + 1];
            re[2 * j] = ar + br; im[2 * j] = ai + bi;
            re[2 * j + 1] = ar - br; im[2 * j + 1] = ai - bi;
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = LOG2N & 1; s < LOG2N; s += 2) {       // stages s and s + 1 on the points p, p + h, p + 2 h, p + 3 h
        const int h = 1 << s;
        for (int j = tid; j < half_n / 2; j += kGlThreads) {
            const int pos = j & (h - 1);
            const int p = ((j >> s) << (s + 2)) + pos;
            float2 x0 = make_float2(re[p], im[p]), x1 = make_float2(re[p + h], im[p + h]);
            float2 x2 = make_float2(re[p + 2 * h], im[p + 2 * h]), x3 = make_float2(re[p + 3 * h], im[p + 3 * h]);
            const float2 w1 = gl_twiddle<INVERSE>(twiddle, pos * (half_n >> s));
            gl_butterfly(x0, x1, w1);
            gl_butterfly(x2, x3, w1);
            gl_butterfly(x0, x2, gl_twiddle<INVERSE>(twiddle, pos * (half_n >> (s + 1))));
            gl_butterfly(x1, x3, gl_twiddle<INVERSE>(twiddle, (pos + h) * (half_n >> (s + 1))));
            re[p] = x0.x; im[p] = x0.y;
            re[p + h] = x1.x; im[p + h] = x1.y;
            re[p + 2 * h] = x2.x; im[p + 2 * h] = x2.y;
            re[p + 3 * h] = x3.x; im[p + 3 * h] = x3.y;
        }
        __syncthreads();
    }
}

template <int LOG2N>
__device__ __forceinline__ int gl_brev(int n) { return (int)(__brev((unsigned)n) >> (32 - LOG2N)); }

// bins this thread owns: k = tid + i * kGlThreads < n_freq
template <int LOG2N>
struct GlBins { static constexpr int n = (1 << (LOG2N - 1)) / kGlThreads + 1; };

// y[i]: the half spectrum's bins of this thread -> Hermitian-extended into LDS (the imaginary parts of bin 0 and of the Nyquist bin are
// dropped, as irfft drops them), inverse FFT, and the windowed frame [win] to `frame`.  The caller has finished reading re / im.
template <int LOG2N>
__device__ __forceinline__ void gl_synth_frame(const GlDev& G, float* re, float* im, const float2 (&y)[GlBins<LOG2N>::n], float* frame) {
    constexpr int N = 1 << LOG2N;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < GlBins<LOG2N>::n; ++i) {
        const int k = tid + i * kGlThreads;
        if (k > N / 2) continue;
        const bool edge = k == 0 || k == N / 2;
        const int r = gl_brev<LOG2N>(k);
        re[r] = y[i].x;
        im[r] = edge ? 0.f : y[i].y;
        if (!edge) {
            const int r2 = gl_brev<LOG2N>(N - k);
            re[r2] = y[i].x;
            im[r2] = -y[i].y;
        }
    }
    __syncthreads();
    gl_fft<LOG2N, true>(re, im, G.twiddle);
    const float scale = 1.0f / (float)N;
    for (int j = tid; j < G.win; j += kGlThreads) frame[j] = re[G.woff + j] * scale * G.window[j];
}

// the overlap-added, envelope-normalised sample at position p of the padded signal (p in the kept range), from the stored windowed
// frames fr [F][win] of one item: frames in ascending order, the envelope (sum of squared windows) in the same order
__device__ __forceinline__ float gl_gather(const GlDev& G, const float* fr, int F, int p) {
    const int q = p - G.woff;                                   // >= win / 2 in the kept range
    const int f_lo = max(0, (q - G.win + G.hop) / G.hop);       // first frame whose window reaches q
    const int f_hi = min(F - 1, q / G.hop);
    float acc = 0.f, env = 0.f;
    for (int f = f_lo; f <= f_hi; ++f) {
        const int j = q - f * G.hop;                            // in [0, win)
        const float w = G.window[j];
        acc += fr[(size_t)f * G.win + j];
        env = fmaf(w, w, env);
    }
    return acc / env;
}

// first launch of a run: public layouts spec [B][n_freq][F], angles [B][n_freq][F] -> frames-major spec_fm [B][F][n_freq] and frame 0
template <int LOG2N>
__global__ __launch_bounds__(kGlThreads) void k_gl_synth(const GlDev G, const float* spec, const float2* angles, int F, float* spec_fm,
                                                         float* frames) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int N = 1 << LOG2N;
    float* re = lds;
    float* im = lds + N;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float2 y[GlBins<LOG2N>::n];
#pragma unroll
    for (int i = 0; i < GlBins<LOG2N>::n; ++i) {
        const int k = tid + i * kGlThreads;
        y[i] = make_float2(0.f, 0.f);
        if (k > N / 2) continue;
        const size_t src = ((size_t)b * G.n_freq + k) * F + t;
        const float s = spec[src];
        const float2 a = angles[src];
        spec_fm[((size_t)b * F + t) * G.n_freq + k] = s;
        y[i] = make_float2(s * a.x, s * a.y);
    }
    gl_synth_frame<LOG2N>(G, re, im, y, frames + ((size_t)b * F + t) * G.win);
}

// one Griffin-Lim iteration for one frame: frames_in -> rebuilt column -> angles -> frames_out; tprev [B][F][n_freq] in place
template <int LOG2N>
__global__ __launch_bounds__(kGlThreads) void k_gl_iter(const GlDev G, const float* spec_fm, const float* frames_in, float* frames_out,
                                                        float2* tprev, int F, float alpha, int have_prev) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int N = 1 << LOG2N;
    float* re = lds;
    float* im = lds + N;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* fr = frames_in + (size_t)b * F * G.win;
    const int keep_lo = N / 2, keep_hi = N / 2 + G.hop * (F - 1);
    for (int n = tid; n < N; n += kGlThreads) {
        float v = 0.f;
        const int wn = n - G.woff;
        const int p = t * G.hop + n;
        if (wn >= 0 && wn < G.win && p >= keep_lo && p < keep_hi) v = gl_gather(G, fr, F, p) * G.window[wn];
        const int r = gl_brev<LOG2N>(n);
        re[r] = v;
        im[r] = 0.f;
    }
    __syncthreads();
    gl_fft<LOG2N, false>(re, im, G.twiddle);
    float2 y[GlBins<LOG2N>::n];
    const size_t col = ((size_t)b * F + t) * G.n_freq;
#pragma unroll
    for (int i = 0; i < GlBins<LOG2N>::n; ++i) {
        const int k = tid + i * kGlThreads;
        y[i] = make_float2(0.f, 0.f);
        if (k > N / 2) continue;
        const float2 rebuilt = make_float2(re[k], im[k]);
        float2 a = rebuilt;
        if (have_prev) {
            const float2 tp = tprev[col + k];
            a.x = rebuilt.x - alpha * tp.x;
            a.y = rebuilt.y - alpha * tp.y;
        }
        tprev[col + k] = rebuilt;
        const float d = hypotf(a.x, a.y) + FLT_MIN;            // an exactly zero entry stays zero
        const float s = spec_fm[col + k];
        y[i] = make_float2(s * (a.x / d), s * (a.y / d));
    }
    __syncthreads();                                            // every bin is in registers before the LDS is overwritten
    gl_synth_frame<LOG2N>(G, re, im, y, frames_out + ((size_t)b * F + t) * G.win);
}

__global__ __launch_bounds__(kGlThreads) void k_gl_output(const GlDev G, const float* frames, int F, float* wav) {
    const int L = G.hop * (F - 1);
    const int i = blockIdx.x * kGlThreads + threadIdx.x, b = blockIdx.y;
    if (i >= L) return;
    wav[(size_t)b * L + i] = gl_gather(G, frames + (size_t)b * F * G.win, F, i + G.n_fft / 2);
}

}  // namespace gvc

using namespace gvc;

struct gvc_gl {
    GlDev dev;
    gvc_gl_options opt;
    int log2n = 0;
    void* blob = nullptr;
    float* spec_fm = nullptr;          // [max_batch][max_frames][n_freq]
    float2* tprev = nullptr;           // [max_batch][max_frames][n_freq]
    float* frames[2] = {nullptr, nullptr};   // [max_batch][max_frames][win] each
    std::vector<float> w_host;         // [n_freq][n_mels]
    long long launches = 0;
};

// W = fb (fb^T fb)^-1 in double: Cholesky of the Gram matrix, then two triangular solves per frequency bin.  Returns the first filter
// at which the factorisation breaks down (a filter without a bin, or one that depends on the others), or -1.
static int gl_inverse_matrix(const std::vector<double>& fb, int n_freq, int n_mels, std::vector<float>* w) {
    const int M = n_mels;
    std::vector<double> L((size_t)M * M, 0.0);
    for (int i = 0; i < M; ++i)
        for (int j = 0; j <= i; ++j) {
            double g = 0.0;
            for (int k = 0; k < n_freq; ++k) g += fb[(size_t)k * M + i] * fb[(size_t)k * M + j];
            L[(size_t)i * M + j] = g;
        }
    for (int j = 0; j < M; ++j) {
        double d = L[(size_t)j * M + j];
        const double gjj = d;
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * M + k] * L[(size_t)j * M + k];
        if (!(d > 1e-12 * gjj) || !(gjj > 0.0)) return j;
        const double ljj = sqrt(d);
        L[(size_t)j * M + j] = ljj;
        for (int i = j + 1; i < M; ++i) {
            double s = L[(size_t)i * M + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * M + k] * L[(size_t)j * M + k];
            L[(size_t)i * M + j] = s / ljj;
        }
    }
    w->assign((size_t)n_freq * M, 0.f);
    std::vector<double> z(M);
    for (int k = 0; k < n_freq; ++k) {
        for (int i = 0; i < M; ++i) {                       // L z = fb[k]
            double s = fb[(size_t)k * M + i];
            for (int j = 0; j < i; ++j) s -= L[(size_t)i * M + j] * z[j];
            z[i] = s / L[(size_t)i * M + i];
        }
        for (int i = M - 1; i >= 0; --i) {                  // L^T w = z
            double s = z[i];
            for (int j = i + 1; j < M; ++j) s -= L[(size_t)j * M + i] * z[j];
            z[i] = s / L[(size_t)i * M + i];
        }
        for (int i = 0; i < M; ++i) (*w)[(size_t)k * M + i] = (float)z[i];
    }
    return -1;
}

extern "C" int gvc_gl_create(const gvc_gl_options* o, const float* mel_norms_host, gvc_gl** out) {
    GVC_REQUIRE(o && out, GVC_ERR_ARG, "gvc_gl_create: null argument");
    int log2n = 0;
    while ((1 << log2n) < o->n_fft) ++log2n;
    GVC_REQUIRE((1 << log2n) == o->n_fft && o->n_fft >= 512 && o->n_fft <= 2048, GVC_ERR_ARG,
                "gvc_gl_create: n_fft %d is not a power of two in [512, 2048]", o->n_fft);
    GVC_REQUIRE(o->win >= 2 && o->win <= o->n_fft && (o->n_fft - o->win) % 2 == 0, GVC_ERR_ARG,
                "gvc_gl_create: win %d outside [2, n_fft = %d] (or not centred)", o->win, o->n_fft);
    GVC_REQUIRE(o->hop >= 1 && o->win % o->hop == 0 && o->win / o->hop >= 2, GVC_ERR_ARG,
                "gvc_gl_create: hop %d must divide win %d at least twice", o->hop, o->win);
    GVC_REQUIRE(o->n_mels >= 1 && o->n_mels <= 256 && o->sample_rate >= 2 && o->f_max > o->f_min && o->f_min >= 0.f, GVC_ERR_ARG,
                "gvc_gl_create: bad n_mels / sample_rate / band");
    GVC_REQUIRE(o->max_batch >= 1 && o->max_batch <= 4096 && o->max_frames >= 2 && o->max_frames <= (1 << 20), GVC_ERR_ARG,
                "gvc_gl_create: max_batch %d / max_frames %d outside [1, 4096] / [2, 2^20]", o->max_batch, o->max_frames);
    const int n_fft = o->n_fft, win = o->win, n_mels = o->n_mels, n_freq = n_fft / 2 + 1;
    // torchaudio.functional.melscale_fbanks(norm="slaney", mel_scale="htk"), as gvc_mel_create builds it, kept in double
    auto hz2mel = [](double f) { return 2595.0 * log10(1.0 + f / 700.0); };
    auto mel2hz = [](double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); };
    std::vector<double> fpts(n_mels + 2);
    const double m_lo = hz2mel(o->f_min), m_hi = hz2mel(o->f_max);
    for (int i = 0; i < n_mels + 2; ++i) fpts[i] = mel2hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    std::vector<double> fb((size_t)n_freq * n_mels);
    for (int m = 0; m < n_mels; ++m) {
        const double enorm = 2.0 / (fpts[m + 2] - fpts[m]);
        bool any = false;
        for (int k = 0; k < n_freq; ++k) {
            const double f = (double)(o->sample_rate / 2) * k / (n_freq - 1);
            const double down = (f - fpts[m]) / (fpts[m + 1] - fpts[m]);
            const double up = (fpts[m + 2] - f) / (fpts[m + 2] - fpts[m + 1]);
            const double v = fmax(0.0, fmin(down, up)) * enorm;
            fb[(size_t)k * n_mels + m] = v;
            any |= v > 0.0;
        }
        GVC_REQUIRE(any, GVC_ERR_ARG, "gvc_gl_create: mel filter %d of %d has no frequency bin (n_fft %d at %d Hz): the filterbank has no "
                    "inverse", m, n_mels, n_fft, o->sample_rate);
    }
    auto* c = new gvc_gl();
    const int bad = gl_inverse_matrix(fb, n_freq, n_mels, &c->w_host);
    if (bad >= 0) {
        delete c;
        GVC_REQUIRE(false, GVC_ERR_ARG, "gvc_gl_create: mel filter %d of %d is not independent of the filters before it: the filterbank's "
                    "Gram matrix is not positive definite", bad, n_mels);
    }
    std::vector<float> window(win);
    for (int n = 0; n < win; ++n) window[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / win));
    std::vector<float> tw(n_fft);
    for (int k = 0; k < n_fft / 2; ++k) {
        tw[2 * k] = (float)cos(-2.0 * M_PI * k / n_fft);
        tw[2 * k + 1] = (float)sin(-2.0 * M_PI * k / n_fft);
    }
    std::vector<float> wt((size_t)n_mels * n_freq);
    for (int k = 0; k < n_freq; ++k)
        for (int m = 0; m < n_mels; ++m) wt[(size_t)m * n_freq + k] = c->w_host[(size_t)k * n_mels + m];
    auto al = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t o_win = 0, o_tw = al(o_win + (size_t)win * 4), o_wt = al(o_tw + (size_t)n_fft * 4), o_nrm = al(o_wt + wt.size() * 4),
                 total = al(o_nrm + (size_t)n_mels * 4);
    std::vector<char> host(total, 0);
    memcpy(&host[o_win], window.data(), (size_t)win * 4);
    memcpy(&host[o_tw], tw.data(), (size_t)n_fft * 4);
    memcpy(&host[o_wt], wt.data(), wt.size() * 4);
    for (int m = 0; m < n_mels; ++m) reinterpret_cast<float*>(&host[o_nrm])[m] = mel_norms_host ? mel_norms_host[m] : 1.0f;
    const size_t cols = (size_t)o->max_batch * o->max_frames;
    hipError_t e = hipMalloc(&c->blob, total);
    if (e == hipSuccess) e = hipMemcpy(c->blob, host.data(), total, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->spec_fm), cols * n_freq * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->tprev), cols * n_freq * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->frames[0]), cols * win * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->frames[1]), cols * win * sizeof(float));
    if (e != hipSuccess) {
        gvc_gl_destroy(c);
        GVC_REQUIRE(false, GVC_ERR_HIP, "gvc_gl_create: device allocation failed: %s", hipGetErrorString(e));
    }
    char* base = (char*)c->blob;
    c->opt = *o;
    c->log2n = log2n;
    c->dev.n_fft = n_fft; c->dev.hop = o->hop; c->dev.win = win; c->dev.n_freq = n_freq; c->dev.n_mels = n_mels;
    c->dev.woff = (n_fft - win) / 2;
    c->dev.window = (const float*)(base + o_win); c->dev.twiddle = (const float2*)(base + o_tw);
    c->dev.wt = (const float*)(base + o_wt); c->dev.norms = (const float*)(base + o_nrm);
    *out = c;
    return GVC_OK;
}

extern "C" int gvc_gl_destroy(gvc_gl* c) {
    if (!c) return GVC_OK;
    if (c->blob) hipFree(c->blob);
    if (c->spec_fm) hipFree(c->spec_fm);
    if (c->tprev) hipFree(c->tprev);
    for (float* f : c->frames)
        if (f) hipFree(f);
    delete c;
    return GVC_OK;
}

extern "C" int gvc_gl_inverse_matrix(gvc_gl* c, float* W) {
    GVC_REQUIRE(c && W, GVC_ERR_ARG, "gvc_gl_inverse_matrix: null argument");
    memcpy(W, c->w_host.data(), c->w_host.size() * sizeof(float));
    return GVC_OK;
}

extern "C" long long gvc_gl_launches(gvc_gl* c) { return c ? c->launches : -1; }

extern "C" int gvc_gl_inverse_mel(gvc_gl* c, const float* mel, int32_t B, int32_t F, float* spec, gvc_stream sv) {
    GVC_REQUIRE(c && mel && spec, GVC_ERR_ARG, "gvc_gl_inverse_mel: null argument");
    GVC_REQUIRE(B >= 1 && B <= 65535 && F >= 1, GVC_ERR_ARG, "gvc_gl_inverse_mel: B=%d F=%d", B, F);
    const size_t lds = (size_t)c->dev.n_mels * kGlTile * sizeof(float);
    hipLaunchKernelGGL(k_gl_inverse_mel, dim3(cdiv(F, kGlTile), B), dim3(kGlThreads), lds, (hipStream_t)sv, c->dev, mel, F, spec);
    GVC_LAUNCH_CHECK();
    ++c->launches;
    return GVC_OK;
}

extern "C" int gvc_gl_init_angles(gvc_gl* c, uint64_t seed, int32_t B, int32_t F, void* angles, gvc_stream sv) {
    GVC_REQUIRE(c && angles, GVC_ERR_ARG, "gvc_gl_init_angles: null argument");
    GVC_REQUIRE(B >= 1 && F >= 1, GVC_ERR_ARG, "gvc_gl_init_angles: B=%d F=%d", B, F);
    const long long total = (long long)B * c->dev.n_freq * F;
    GVC_REQUIRE(total <= (long long)kGlThreads * 0x7fffffff, GVC_ERR_ARG, "gvc_gl_init_angles: B=%d F=%d is too large", B, F);
    hipLaunchKernelGGL(k_gl_init_angles, dim3((unsigned)((total + kGlThreads - 1) / kGlThreads)), dim3(kGlThreads), 0, (hipStream_t)sv,
                       seed, c->dev.n_freq, F, total, (float2*)angles);
    GVC_LAUNCH_CHECK();
    ++c->launches;
    return GVC_OK;
}

template <int LOG2N>
static int gl_run(gvc_gl* c, const float* spec, const float2* init, int B, int F, int n_iter, float alpha, float* wav, hipStream_t s) {
    const size_t lds = 2 * sizeof(float) << LOG2N;
    const dim3 grid(F, B), block(kGlThreads);
    int cur = 0;
    hipLaunchKernelGGL(k_gl_synth<LOG2N>, grid, block, lds, s, c->dev, spec, init, F, c->spec_fm, c->frames[cur]);
    GVC_LAUNCH_CHECK();
    ++c->launches;
    for (int it = 0; it < n_iter; ++it) {
        hipLaunchKernelGGL(k_gl_iter<LOG2N>, grid, block, lds, s, c->dev, c->spec_fm, c->frames[cur], c->frames[cur ^ 1], c->tprev, F,
                           alpha, it > 0 ? 1 : 0);
        GVC_LAUNCH_CHECK();
        ++c->launches;
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_gl_output, dim3(cdiv(c->dev.hop * (F - 1), kGlThreads), B), block, 0, s, c->dev, c->frames[cur], F, wav);
    GVC_LAUNCH_CHECK();
    ++c->launches;
    return GVC_OK;
}

extern "C" int gvc_gl_run(gvc_gl* c, const float* spec, const void* init_angles, int32_t B, int32_t F, int32_t n_iter, float momentum,
                          float* wav, gvc_stream sv) {
    GVC_REQUIRE(c && spec && init_angles && wav, GVC_ERR_ARG, "gvc_gl_run: null argument");
    GVC_REQUIRE(B >= 1 && B <= c->opt.max_batch && F >= 2 && F <= c->opt.max_frames, GVC_ERR_ARG,
                "griffinlim: B=%d F=%d outside capacity (%d, 2..%d)", B, F, c->opt.max_batch, c->opt.max_frames);
    GVC_REQUIRE(n_iter >= 0 && momentum >= 0.f && momentum < 1.f, GVC_ERR_ARG, "griffinlim: n_iter %d / momentum %g (n_iter >= 0, "
                "0 <= momentum < 1)", n_iter, (double)momentum);
    GVC_REQUIRE(B <= 65535, GVC_ERR_ARG, "griffinlim: B=%d exceeds the grid", B);
    const float alpha = (float)((double)momentum / (1.0 + (double)momentum));
    const float2* init = (const float2*)init_angles;
    hipStream_t s = (hipStream_t)sv;
    switch (c->log2n) {
        case 9: return gl_run<9>(c, spec, init, B, F, n_iter, alpha, wav, s);
        case 10: return gl_run<10>(c, spec, init, B, F, n_iter, alpha, wav, s);
        default: return gl_run<11>(c, spec, init, B, F, n_iter, alpha, wav, s);
    }
}
