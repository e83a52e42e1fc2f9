// Waveform-domain discriminators of the vocoder trainer's evaluation step (reference layers/hifigan.py: DiscriminatorS :247-279,
// MultiScaleDiscriminator :281-314, DiscriminatorP :316-396, MultiPeriodDiscriminator :399-426) in eval mode, and the reductions
// behind the criteria of layers/hifigan_loss.py:78-123.  DESIGN.md section 4.22.
//
// Layout: every feature map is stored once, channel-major [2 B][C][H][W] (MSD: W = 1), which is the reference's own layout -- the
// Python layer hands out views -- and the layout the next layer stages from.  The real and the generated waveform are items
// [0, B) and [B, 2 B) of one batch, so a call reads every weight once.
//
// k_disc_conv is the wide grouped / strided conv (41 taps, 4 or 16 groups, stride 1 / 2 / 4; MPD: 5 taps, stride 3, dense):
// out[co][t] = sum_{ci, j} W[co][ci][j] x[ci][s t + j - pad] as an implicit GEMM on v_mfma_f32_16x16x4_f32 with the WEIGHTS as
// the A operand (a lane's four results are four channels of one frame, 16 lanes store 16 consecutive frames of a channel) and the
// input window of the workgroup's frames, staged ONCE per channel chunk in LDS, as the B operand: tap j of frame t is LDS word
// s t + j of the channel's row, so no im2col copy exists anywhere.  Zero padding, the MPD's period view (column = extra batch,
// frame stride = period) are address arithmetic of the staging loop.  A wave owns 16 channels x 64 frames (four independent
// accumulators: the 16x16x4 f32 MFMA has a 40-cycle dependent latency at a 32-cycle issue interval).  Weights are repacked at
// bind time into the order the lanes read them (64 consecutive floats per MFMA step).
//
// The CI = 1 first layers (k_disc_first; the MSD's average pools and the MPD's reflect padding + period view are folded into its
// staging) and the one-channel conv_post (k_disc_post) are plain vector code.
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace gvc {

typedef float dc_f32x4 __attribute__((ext_vector_type(4)));

// where element (co, ci, j) of a conv weight [Co][Cig][k] sits in the MFMA operand order: [co / 16][ci / 4][j][lane], lane = (ci % 4) * 16 + co % 16
__host__ __device__ __forceinline__ size_t dc_pack_idx(int co, int ci, int j, int Cig, int k) {
    return ((((size_t)(co >> 4) * (Cig >> 2) + (ci >> 2)) * k + j) << 6) + ((ci & 3) << 4) + (co & 15);
}

// block sum of 256 threads in a fixed order, result in every thread
__device__ __forceinline__ float dc_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// weight norm (torch._weight_norm, dim 0): w[co] = v[co] * (g[co] / |v[co]|); one workgroup per output channel
__global__ __launch_bounds__(256) void k_disc_fold_wn(const float* v, const float* g, float* out, int R, int Cig, int k, int packed) {
    __shared__ float red[4];
    const int co = blockIdx.x;
    const float* vr = v + (size_t)co * R;
    float s = 0.f;
    for (int i = threadIdx.x; i < R; i += 256) s = fmaf(vr[i], vr[i], s);
    const float scale = g[co] / sqrtf(dc_block_sum(s, red));
    for (int i = threadIdx.x; i < R; i += 256) {
        const size_t at = packed ? dc_pack_idx(co, i / k, i % k, Cig, k) : (size_t)co * R + i;
        out[at] = vr[i] * scale;
    }
}

// spectral norm, eval mode (torch.nn.utils.spectral_norm: sigma = u . (W_mat v) with the stored u, v): part[co] = u[co] (W_mat v)[co]
__global__ __launch_bounds__(256) void k_disc_sn_rows(const float* w, const float* u, const float* v, float* part, int R) {
    __shared__ float red[4];
    const int co = blockIdx.x;
    const float* wr = w + (size_t)co * R;
    float s = 0.f;
    for (int i = threadIdx.x; i < R; i += 256) s = fmaf(wr[i], v[i], s);
    s = dc_block_sum(s, red);
    if (threadIdx.x == 0) part[co] = u[co] * s;
}

// w = weight_orig / sigma, sigma = sum of part[0 .. Co) in a fixed order (every workgroup computes the same value)
__global__ __launch_bounds__(256) void k_disc_fold_sn(const float* w, const float* part, float* out, int Co, int R, int Cig, int k, int packed) {
    __shared__ float red[4];
    const int co = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < Co; i += 256) s += part[i];
    const float sigma = dc_block_sum(s, red);
    const float* wr = w + (size_t)co * R;
    for (int i = threadIdx.x; i < R; i += 256) {
        const size_t at = packed ? dc_pack_idx(co, i / k, i % k, Cig, k) : (size_t)co * R + i;
        out[at] = wr[i] / sigma;
    }
}

// folded weight back in the plain order [Co][Cig][k]
__global__ void k_disc_export(const float* w, float* out, int Co, int Cig, int k, int packed) {
    const size_t n = (size_t)Co * Cig * k;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % k), ci = (int)((i / k) % Cig), co = (int)(i / ((size_t)k * Cig));
        out[i] = w[packed ? dc_pack_idx(co, ci, j, Cig, k) : i];
    }
}

// ---- first layers (C_in = 1) ---------------------------------------------------------------------------------------------------
// sum of the AvgPool1d(4, 2, padding = 2) window that starts at x[t] (zero padding counts, as count_include_pad does)
__device__ __forceinline__ float dc_win4(const float* x, int T, int t) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += (t + i >= 0 && t + i < T) ? x[t + i] : 0.f;
    return s;
}

// sample t of the input of MSD scale `scale`: the waveform after `scale` average pools; 0 outside the pooled length
__device__ __forceinline__ float dc_msd_in(const float* x, int T, int scale, int t) {
    if (scale == 0) return (t >= 0 && t < T) ? x[t] : 0.f;
    const int T1 = T / 2 + 1;
    if (scale == 1) return (t >= 0 && t < T1) ? 0.25f * dc_win4(x, T, 2 * t - 2) : 0.f;
    const int T2 = T1 / 2 + 1;
    if (t < 0 || t >= T2) return 0.f;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = 2 * t - 2 + i;
        s += (u >= 0 && u < T1) ? 0.25f * dc_win4(x, T, 2 * u - 2) : 0.f;
    }
    return 0.25f * s;
}

// row h, column col of the MPD's view [H][p] of the waveform, reflect-padded on the right to H p samples; 0 outside [0, H)
__device__ __forceinline__ float dc_mpd_in(const float* x, int T, int p, int col, int H, int h) {
    if (h < 0 || h >= H) return 0.f;
    const int i = h * p + col;
    return x[i < T ? i : 2 * (T - 1) - i];
}

// y[n][co][t][col] = lrelu(bias[co] + sum_j w[co][j] in(s t + j - pad)); mode 0: MSD scale prm, mode 1: MPD period prm (P = prm columns
// as extra batch).  A workgroup owns 256 frames of one (item, column): their window is staged in LDS, a thread keeps its K taps in
// registers and walks the output channels (weights and bias are wave-uniform loads)
template <int K>
__global__ __launch_bounds__(256) void k_disc_first(const float* wav, int T, int mode, int prm, int Tin, int Tout, int stride, int pad,
                                                    const float* w, const float* bias, int Co, float* y, int P, long long y_ns,
                                                    long long y_cs, int y_ts, float slope) {
    extern __shared__ __attribute__((aligned(16))) float dc_lds[];
    const int n = blockIdx.y / P, col = blockIdx.y % P, t0 = blockIdx.x * 256;
    const float* x = wav + (size_t)n * T;
    const int ws = t0 * stride - pad, wlen = 255 * stride + K;
    for (int wi = threadIdx.x; wi < wlen; wi += 256)
        dc_lds[wi] = mode == 0 ? dc_msd_in(x, T, prm, ws + wi) : dc_mpd_in(x, T, prm, col, Tin, ws + wi);
    __syncthreads();
    float xv[K];
#pragma unroll
    for (int j = 0; j < K; ++j) xv[j] = dc_lds[threadIdx.x * stride + j];
    const int t = t0 + threadIdx.x;
    if (t >= Tout) return;
    float* yo = y + (size_t)n * y_ns + col + (size_t)t * y_ts;
    for (int co = 0; co < Co; ++co) {
        float acc = bias[co];
#pragma unroll
        for (int j = 0; j < K; ++j) acc = fmaf(w[co * K + j], xv[j], acc);
        yo[(size_t)co * y_cs] = acc > 0.f ? acc : slope * acc;
    }
}

// ---- the grouped / strided conv on the matrix cores ----------------------------------------------------------------------------
struct DcConvArgs {
    const float* x;
    float* y;
    const float* wp;          // packed weights (dc_pack_idx)
    const float* bias;
    int Cig, Cog, k, stride, pad, Tin, Tout;
    int ncot, m;              // 16-channel tiles and 64-frame tiles of a workgroup (ncot * m = 4 waves)
    int CC, W;                // channels staged per round and the LDS row length (>= (64 m - 1) stride + k)
    int P;                    // columns that ride along as extra batch (MPD: the period)
    long long x_ns, x_cs, y_ns, y_cs;     // item and channel strides
    int x_ts, y_ts;           // frame strides
    float slope;
};

__global__ __launch_bounds__(256) void k_disc_conv(const DcConvArgs A) {
    extern __shared__ __attribute__((aligned(16))) float dc_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tl = lane & 15, kq = lane >> 4;
    const int n = blockIdx.z / A.P, col = blockIdx.z % A.P;
    const int cot = blockIdx.y * A.ncot + wave % A.ncot, sub = wave / A.ncot;
    const int g = (blockIdx.y * A.ncot * 16) / A.Cog;
    const int t0 = blockIdx.x * 64 * A.m;
    const int ws = t0 * A.stride - A.pad, wlen = (64 * A.m - 1) * A.stride + A.k;
    const float* xb = A.x + (size_t)n * A.x_ns + col + (size_t)g * A.Cig * A.x_cs;
    const int nq = A.Cig >> 2;
    dc_f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = dc_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cc0 = 0; cc0 < A.Cig; cc0 += A.CC) {
        if (cc0) __syncthreads();
        for (int ci = wave; ci < A.CC; ci += 4) {
            const float* xr = xb + (size_t)(cc0 + ci) * A.x_cs;
            float* row = dc_lds + ci * A.W;
            for (int wi = lane; wi < wlen; wi += 64) {
                const int t = ws + wi;
                row[wi] = (t >= 0 && t < A.Tin) ? xr[(size_t)t * A.x_ts] : 0.f;
            }
        }
        __syncthreads();
        const float* wq = A.wp + (((size_t)cot * nq + (cc0 >> 2)) * A.k << 6) + lane;
        const float* bq = dc_lds + kq * A.W + (sub * 64 + tl) * A.stride;
        for (int q = 0; q < (A.CC >> 2); ++q) {
            for (int j = 0; j < A.k; ++j) {
                const float a = wq[((size_t)q * A.k + j) << 6];
                const float* bp = bq + q * 4 * A.W + j;
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[u * 16 * A.stride], acc[u], 0, 0, 0);
            }
        }
    }
    float* yb = A.y + (size_t)n * A.y_ns + col;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = t0 + sub * 64 + u * 16 + tl;
        if (t >= A.Tout) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = cot * 16 + kq * 4 + r;
            const float v = acc[u][r] + A.bias[co];
            yb[(size_t)co * A.y_cs + (size_t)t * A.y_ts] = v > 0.f ? v : A.slope * v;
        }
    }
}

// ---- conv_post (C_out = 1, k = 3, no activation) -------------------------------------------------------------------------------
// y[n][q] = bias + sum_{ci, j} w[ci][j] x[n][ci][q + (j - 1) dil] over the flat frame index q in [0, L): MSD dil = 1; the MPD's (3, 1)
// conv over [H][p] is the same with dil = p.  64 frames per workgroup, the channels in four quarters added in a fixed order
__global__ __launch_bounds__(256) void k_disc_post(const float* x, const float* w, const float* bias, float* y, int Ci, int L, int dil) {
    __shared__ float red[4][64];
    const int ql = threadIdx.x & 63, cq = threadIdx.x >> 6, n = blockIdx.y;
    const int q = blockIdx.x * 64 + ql, per = Ci >> 2;
    float acc = 0.f;
    if (q < L) {
        const float* xr = x + ((size_t)n * Ci + (size_t)cq * per) * L;
        const float* wr = w + (size_t)cq * per * 3;
        const bool lo = q - dil >= 0, hi = q + dil < L;
        for (int ci = 0; ci < per; ++ci, xr += L, wr += 3) {
            if (lo) acc = fmaf(wr[0], xr[q - dil], acc);
            acc = fmaf(wr[1], xr[q], acc);
            if (hi) acc = fmaf(wr[2], xr[q + dil], acc);
        }
    }
    red[cq][ql] = acc;
    __syncthreads();
    if (cq == 0 && q < L) y[(size_t)n * L + q] = bias[0] + (((red[0][ql] + red[1][ql]) + red[2][ql]) + red[3][ql]);
}

// ---- reductions ----------------------------------------------------------------------------------------------------------------
// mode 0: |a - b|, 1: (1 - a)^2, 2: a^2
struct DcRedJob { const float* a; const float* b; long long n; int mode; int pad_; };
constexpr int kDcRedBlocks = 256;

// part[job][block] = sum of the block's contiguous slice: thread-strided float sums, then a fixed tree in double -- no atomics
__global__ __launch_bounds__(256) void k_disc_red_partials(const DcRedJob* jobs, DcRedJob one, double* part) {
    __shared__ double red[256];
    const DcRedJob J = jobs ? jobs[blockIdx.y] : one;
    const long long chunk = (J.n + kDcRedBlocks - 1) / kDcRedBlocks;
    const long long i0 = (long long)blockIdx.x * chunk, i1 = i0 + chunk < J.n ? i0 + chunk : J.n;
    float s = 0.f;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        const float a = J.a[i];
        if (J.mode == 0) s += fabsf(a - J.b[i]);
        else if (J.mode == 1) s = fmaf(1.f - a, 1.f - a, s);
        else s = fmaf(a, a, s);
    }
    red[threadIdx.x] = (double)s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * kDcRedBlocks + blockIdx.x] = red[0];
}

// out[job] = scale * (sum of part[job][..]) / n
__global__ __launch_bounds__(256) void k_disc_red_finish(const DcRedJob* jobs, DcRedJob one, const double* part, float scale, float* out) {
    __shared__ double red[256];
    const long long n = jobs ? jobs[blockIdx.x].n : one.n;
    red[threadIdx.x] = part[(size_t)blockIdx.x * kDcRedBlocks + threadIdx.x];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)((double)scale * red[0] / (double)n);
}

}  // namespace gvc

using namespace gvc;

namespace {

constexpr float kDcSlope = 0.1f;          // LRELU_SLOPE
constexpr int kDcLdsMax = 64 * 1024;      // dynamic LDS a launch may ask for without an attribute

struct DcConv {
    int Co = 0, Ci = 0, k = 0, stride = 1, pad = 0, groups = 1, Cig = 0, Cog = 0;
    bool sn = false, packed = false;
    float *raw = nullptr, *g = nullptr, *u = nullptr, *sv = nullptr, *bias = nullptr, *fold = nullptr, *sig = nullptr;
    int have = 0;                         // 1: weight_v / weight_orig, 2: weight_g / weight_u, 4: spectral weight_v
    int R() const { return Cig * k; }
    int need() const { return sn ? 7 : 3; }
};

struct DcPlan {
    hipGraphExec_t ge = nullptr;
    DcRedJob* jobs = nullptr;
};

}  // namespace

struct gvc_disc {
    gvc_disc_dims dm;
    int n_sub = 0, n_layers = 0;
    std::vector<std::vector<DcConv>> conv;            // [sub][layer]
    std::vector<std::vector<long long>> off;          // [sub][layer] arena offsets (capacity geometry)
    long long arena_floats = 0;
    float* arena = nullptr;
    float *wav = nullptr, *stats = nullptr;
    double* part = nullptr;
    int n_jobs = 0;
    std::map<std::string, int> bound;
    int n_expected = 0;
    std::map<long long, DcPlan> plans;
    hipStream_t cap_stream = nullptr;
    std::vector<void*> allocs;
};

static int dc_alloc(gvc_disc* c, float** p, size_t n) {
    GVC_CHECK_HIP(hipMalloc((void**)p, (n ? n : 1) * sizeof(float)));
    c->allocs.push_back(*p);
    return GVC_OK;
}

// frames per layer of sub-discriminator `sub` at T samples: H[l] (MPD: rows of the [H][p] view; MSD: samples)
static void dc_geometry(const gvc_disc* c, int sub, int T, int* H) {
    int h;
    if (c->dm.kind == GVC_DISC_MSD) {
        h = T;
        for (int i = 0; i < sub; ++i) h = h / 2 + 1;                   // AvgPool1d(4, 2, padding = 2)
    } else {
        const int p = c->dm.periods[sub];
        h = (T + p - 1) / p;
    }
    for (int l = 0; l < c->n_layers; ++l) {
        const DcConv& w = c->conv[sub][l];
        h = (h + 2 * w.pad - w.k) / w.stride + 1;
        H[l] = h;
    }
}

extern "C" int gvc_disc_create(const gvc_disc_dims* dims, gvc_disc** out) {
    GVC_REQUIRE(dims && out, GVC_ERR_ARG, "gvc_disc_create: null argument");
    const gvc_disc_dims& D = *dims;
    GVC_REQUIRE(D.kind == GVC_DISC_MSD || D.kind == GVC_DISC_MPD, GVC_ERR_ARG, "gvc_disc_create: kind %d", D.kind);
    GVC_REQUIRE(D.max_batch >= 1 && D.max_batch <= 64 && D.max_samples >= 16 && D.max_samples <= (1 << 24), GVC_ERR_ARG,
                "gvc_disc_create: max_batch %d / max_samples %d outside [1, 64] / [16, 2^24]", D.max_batch, D.max_samples);
    auto* c = new gvc_disc();
    c->dm = D;
    int rc = GVC_OK;
    auto add = [&](std::vector<DcConv>& v, int Co, int Ci, int k, int stride, int pad, int groups, bool sn) {
        DcConv w;
        w.Co = Co; w.Ci = Ci; w.k = k; w.stride = stride; w.pad = pad; w.groups = groups; w.sn = sn;
        w.Cig = Ci / groups; w.Cog = Co / groups;
        w.packed = Ci > 1 && Co > 1;
        v.push_back(w);
    };
    if (D.kind == GVC_DISC_MSD) {
        c->n_sub = 3;
        for (int i = 0; i < 3; ++i) {
            std::vector<DcConv> v;
            const bool sn = i == 0;
            add(v, 128, 1, 15, 1, 7, 1, sn);
            add(v, 128, 128, 41, 2, 20, 4, sn);
            add(v, 256, 128, 41, 2, 20, 16, sn);
            add(v, 512, 256, 41, 4, 20, 16, sn);
            add(v, 1024, 512, 41, 4, 20, 16, sn);
            add(v, 1024, 1024, 41, 1, 20, 16, sn);
            add(v, 1024, 1024, 5, 1, 2, 1, sn);
            add(v, 1, 1024, 3, 1, 1, 1, sn);
            c->conv.push_back(v);
        }
    } else {
        if (D.n_sub < 1 || D.n_sub > GVC_DISC_MAX_SUB) { delete c; gvc::set_error("gvc_disc_create: %d periods", D.n_sub); return GVC_ERR_ARG; }
        c->n_sub = D.n_sub;
        for (int i = 0; i < D.n_sub; ++i) {
            if (D.periods[i] < 1 || D.periods[i] > 64) { delete c; gvc::set_error("gvc_disc_create: period %d", D.periods[i]); return GVC_ERR_ARG; }
            std::vector<DcConv> v;
            const bool sn = D.spectral_norm != 0;
            int ci = 1;
            for (int l = 0; l < 5; ++l) {
                const int co = D.channels[l];
                // a channel count feeds the MFMA kernel as C_in (multiple of 4) and, from the second conv on, as C_out (multiple of 16)
                if (co < 4 || co % 4 || (l > 0 && co % 16)) {
                    delete c;
                    gvc::set_error("gvc_disc_create: MPD width %d of conv %d is not supported (multiples of 4, of 16 after the first)", co, l);
                    return GVC_ERR_UNSUPPORTED;
                }
                add(v, co, ci, 5, 3, 2, 1, sn);       // (all five: stride (3, 1), padding (2, 0) -- reference :324-369)
                ci = co;
            }
            add(v, 1, ci, 3, 1, 1, 1, sn);
            c->conv.push_back(v);
        }
    }
    c->n_layers = (int)c->conv[0].size();
    for (auto& v : c->conv)
        for (DcConv& w : v) {
            const size_t n = (size_t)w.Co * w.R();
            if (!rc) rc = dc_alloc(c, &w.raw, n);
            if (!rc) rc = dc_alloc(c, &w.fold, n);
            if (!rc) rc = dc_alloc(c, &w.bias, w.Co);
            if (!rc) rc = dc_alloc(c, w.sn ? &w.u : &w.g, w.Co);
            if (!rc && w.sn) rc = dc_alloc(c, &w.sv, w.R());
            if (!rc && w.sn) rc = dc_alloc(c, &w.sig, w.Co);
            c->n_expected += w.sn ? 4 : 3;
        }
    // arena: one slot per (sub, layer) at the capacity geometry
    std::vector<int> H(c->n_layers);
    long long at = 0;
    for (int s = 0; s < c->n_sub; ++s) {
        dc_geometry(c, s, D.max_samples, H.data());
        const int W = D.kind == GVC_DISC_MPD ? D.periods[s] : 1;
        std::vector<long long> o;
        for (int l = 0; l < c->n_layers; ++l) {
            o.push_back(at);
            at += ((long long)2 * D.max_batch * c->conv[s][l].Co * H[l] * W + 63) / 64 * 64;
        }
        c->off.push_back(o);
    }
    c->arena_floats = at;
    c->n_jobs = c->n_sub * (3 + c->n_layers);
    if (!rc) rc = dc_alloc(c, &c->wav, (size_t)2 * D.max_batch * D.max_samples);
    if (!rc) rc = dc_alloc(c, &c->stats, c->n_jobs);
    if (!rc) rc = dc_alloc(c, reinterpret_cast<float**>(&c->part), (size_t)2 * c->n_jobs * kDcRedBlocks);
    if (!rc && hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking) != hipSuccess) {
        gvc::set_error("gvc_disc_create: hipStreamCreateWithFlags failed");
        rc = GVC_ERR_HIP;
    }
    if (rc) { gvc_disc_destroy(c); return rc; }
    *out = c;
    return GVC_OK;
}

static void dc_drop_plans(gvc_disc* c) {
    for (auto& kv : c->plans) {
        if (kv.second.ge) (void)hipGraphExecDestroy(kv.second.ge);
        if (kv.second.jobs) (void)hipFree(kv.second.jobs);
    }
    c->plans.clear();
}

extern "C" int gvc_disc_destroy(gvc_disc* c) {
    if (!c) return GVC_OK;
    dc_drop_plans(c);
    if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
    for (void* p : c->allocs) hipFree(p);
    delete c;
    return GVC_OK;
}

// every tensor of the conv is bound: fold its parametrisation into w.fold (operand order for the MFMA layers)
static int dc_fold(DcConv& w, hipStream_t s) {
    if (w.sn) {
        hipLaunchKernelGGL(k_disc_sn_rows, dim3(w.Co), dim3(256), 0, s, w.raw, w.u, w.sv, w.sig, w.R());
        GVC_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_disc_fold_sn, dim3(w.Co), dim3(256), 0, s, w.raw, w.sig, w.fold, w.Co, w.R(), w.Cig, w.k, w.packed ? 1 : 0);
    } else {
        hipLaunchKernelGGL(k_disc_fold_wn, dim3(w.Co), dim3(256), 0, s, w.raw, w.g, w.fold, w.R(), w.Cig, w.k, w.packed ? 1 : 0);
    }
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

extern "C" int gvc_disc_bind_weight(gvc_disc* c, const char* name, const float* src, int64_t numel, gvc_stream sv) {
    GVC_REQUIRE(c && name && src, GVC_ERR_ARG, "gvc_disc_bind_weight: null argument");
    hipStream_t s = (hipStream_t)sv;
    const std::string n(name);
    const std::string pre = "discriminators.";
    if (n.rfind(pre, 0) != 0) return GVC_OK;
    const size_t d1 = n.find('.', pre.size());
    if (d1 == std::string::npos) return GVC_OK;
    const int sub = atoi(n.substr(pre.size(), d1 - pre.size()).c_str());
    if (sub < 0 || sub >= c->n_sub) return GVC_OK;
    std::string rest = n.substr(d1 + 1);
    int layer = -1;
    if (rest.rfind("conv_post.", 0) == 0) {
        layer = c->n_layers - 1;
        rest = rest.substr(10);
    } else if (rest.rfind("convs.", 0) == 0) {
        const size_t d2 = rest.find('.', 6);
        if (d2 == std::string::npos) return GVC_OK;
        layer = atoi(rest.substr(6, d2 - 6).c_str());
        rest = rest.substr(d2 + 1);
        if (layer < 0 || layer >= c->n_layers - 1) return GVC_OK;
    } else {
        return GVC_OK;
    }
    DcConv& w = c->conv[sub][layer];
    float* dst = nullptr;
    int64_t want = 0;
    int bit = 0;
    const int64_t full = (int64_t)w.Co * w.R();
    if (rest == "bias") { dst = w.bias; want = w.Co; }
    else if (!w.sn && rest == "weight_v") { dst = w.raw; want = full; bit = 1; }
    else if (!w.sn && rest == "weight_g") { dst = w.g; want = w.Co; bit = 2; }
    else if (w.sn && rest == "weight_orig") { dst = w.raw; want = full; bit = 1; }
    else if (w.sn && rest == "weight_u") { dst = w.u; want = w.Co; bit = 2; }
    else if (w.sn && rest == "weight_v") { dst = w.sv; want = w.R(); bit = 4; }
    else return GVC_OK;                     // (a parametrisation this conv does not use)
    GVC_REQUIRE(numel == want, GVC_ERR_ARG, "%s: expected %lld elements, got %lld", name, (long long)want, (long long)numel);
    GVC_CHECK_HIP(hipMemcpyAsync(dst, src, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    w.have |= bit;
    c->bound[n] = 1;
    if (bit && w.have == w.need()) return dc_fold(w, s);
    return GVC_OK;
}

extern "C" int gvc_disc_missing_weights(gvc_disc* c) { return c ? c->n_expected - (int)c->bound.size() : -1; }

extern "C" int gvc_disc_layers(gvc_disc* c) { return c ? c->n_layers : -1; }

extern "C" int64_t gvc_disc_arena_floats(gvc_disc* c) { return c ? c->arena_floats : -1; }

extern "C" int gvc_disc_set_arena(gvc_disc* c, float* arena) {
    GVC_REQUIRE(c && arena, GVC_ERR_ARG, "gvc_disc_set_arena: null argument");
    if (arena != c->arena) dc_drop_plans(c);          // (the captured graphs hold the old addresses)
    c->arena = arena;
    return GVC_OK;
}

static int dc_check_shape(gvc_disc* c, int B, int T) {
    GVC_REQUIRE(B >= 1 && B <= c->dm.max_batch && T >= 16 && T <= c->dm.max_samples, GVC_ERR_ARG,
                "disc: B=%d T=%d outside capacity (%d, 16..%d)", B, T, c->dm.max_batch, c->dm.max_samples);
    if (c->dm.kind == GVC_DISC_MPD)
        for (int i = 0; i < c->n_sub; ++i)
            GVC_REQUIRE(T > c->dm.periods[i], GVC_ERR_ARG, "disc: %d samples are too few for the reflect padding of period %d", T, c->dm.periods[i]);
    return GVC_OK;
}

extern "C" int gvc_disc_layer(gvc_disc* c, int32_t sub, int32_t layer, int32_t B, int32_t T, int64_t* offset, int32_t* C, int32_t* H, int32_t* W) {
    GVC_REQUIRE(c && offset && C && H && W, GVC_ERR_ARG, "gvc_disc_layer: null argument");
    GVC_REQUIRE(sub >= 0 && sub < c->n_sub && layer >= 0 && layer < c->n_layers, GVC_ERR_ARG, "gvc_disc_layer: sub %d layer %d", sub, layer);
    int rc = dc_check_shape(c, B, T);
    if (rc) return rc;
    std::vector<int> h(c->n_layers);
    dc_geometry(c, sub, T, h.data());
    *offset = c->off[sub][layer];
    *C = c->conv[sub][layer].Co;
    *H = h[layer];
    *W = c->dm.kind == GVC_DISC_MPD ? c->dm.periods[sub] : 1;
    return GVC_OK;
}

extern "C" int gvc_disc_folded_weight(gvc_disc* c, int32_t sub, int32_t layer, float* out, int64_t numel, gvc_stream sv) {
    GVC_REQUIRE(c && out, GVC_ERR_ARG, "gvc_disc_folded_weight: null argument");
    GVC_REQUIRE(sub >= 0 && sub < c->n_sub && layer >= 0 && layer < c->n_layers, GVC_ERR_ARG, "gvc_disc_folded_weight: sub %d layer %d", sub, layer);
    const DcConv& w = c->conv[sub][layer];
    GVC_REQUIRE(w.have == w.need(), GVC_ERR_STATE, "gvc_disc_folded_weight: the conv's tensors are not all bound");
    GVC_REQUIRE(numel == (int64_t)w.Co * w.R(), GVC_ERR_ARG, "gvc_disc_folded_weight: expected %lld elements", (long long)w.Co * w.R());
    hipLaunchKernelGGL(k_disc_export, dim3(256), dim3(256), 0, (hipStream_t)sv, w.fold, out, w.Co, w.Cig, w.k, w.packed ? 1 : 0);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// one MFMA conv layer: x [NB][Ci][Hin][P] -> y [NB][Co][Hout][P]
static int dc_conv(const DcConv& w, const float* x, float* y, int NB, int Hin, int Hout, int P, float slope, hipStream_t s) {
    DcConvArgs A;
    memset(&A, 0, sizeof(A));
    A.x = x; A.y = y; A.wp = w.fold; A.bias = w.bias;
    A.Cig = w.Cig; A.Cog = w.Cog; A.k = w.k; A.stride = w.stride; A.pad = w.pad; A.Tin = Hin; A.Tout = Hout;
    const int cot_g = w.Cog / 16;
    A.ncot = cot_g % 4 == 0 ? 4 : cot_g % 2 == 0 ? 2 : 1;
    A.m = 4 / A.ncot;
    const int wlen = (64 * A.m - 1) * w.stride + w.k;
    // LDS row length: the lanes of a b32 read are 16 frames x 2 channel rows -- an odd stride wants rows 16 banks apart, an even one
    // an odd row length
    A.W = (w.stride & 1) ? (wlen + 15) / 32 * 32 + 16 : wlen | 1;
    A.CC = 4;
    for (int cc : {32, 16, 8})
        if (w.Cig % cc == 0 && (size_t)cc * A.W * sizeof(float) <= (size_t)kDcLdsMax) { A.CC = cc; break; }
    GVC_REQUIRE(w.Cig % 4 == 0 && w.Cog % 16 == 0 && (size_t)A.CC * A.W * sizeof(float) <= (size_t)kDcLdsMax, GVC_ERR_UNSUPPORTED,
                "disc conv: %d -> %d channels in %d groups is not supported", w.Ci, w.Co, w.groups);
    A.P = P;
    A.x_ns = (long long)w.Ci * Hin * P; A.x_cs = (long long)Hin * P; A.x_ts = P;
    A.y_ns = (long long)w.Co * Hout * P; A.y_cs = (long long)Hout * P; A.y_ts = P;
    A.slope = slope;
    hipLaunchKernelGGL(k_disc_conv, dim3(cdiv(Hout, 64 * A.m), w.Co / (16 * A.ncot), NB * P), dim3(256), (size_t)A.CC * A.W * sizeof(float), s, A);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// layer l of sub-discriminator `sub` at (B, T): the first conv reads c->wav, every other one its predecessor's feature map
static int dc_layer(gvc_disc* c, int sub, int l, int B, int T, hipStream_t s) {
    const int NB = 2 * B, L = c->n_layers;
    std::vector<int> H(L);
    dc_geometry(c, sub, T, H.data());
    const bool mpd = c->dm.kind == GVC_DISC_MPD;
    const int P = mpd ? c->dm.periods[sub] : 1;
    const std::vector<DcConv>& cv = c->conv[sub];
    auto buf = [&](int i) { return c->arena + c->off[sub][i]; };
    if (l == 0) {
        const DcConv& w = cv[0];
        int Hin;
        if (mpd) Hin = (T + P - 1) / P;
        else { Hin = T; for (int i = 0; i < sub; ++i) Hin = Hin / 2 + 1; }
        const size_t lds = (size_t)(255 * w.stride + w.k) * sizeof(float);
        const dim3 grid(cdiv(H[0], 256), NB * P);
        if (w.k == 15)
            hipLaunchKernelGGL(k_disc_first<15>, grid, dim3(256), lds, s, c->wav, T, mpd ? 1 : 0, mpd ? P : sub, Hin, H[0], w.stride, w.pad, w.fold,
                               w.bias, w.Co, buf(0), P, (long long)w.Co * H[0] * P, (long long)H[0] * P, P, kDcSlope);
        else
            hipLaunchKernelGGL(k_disc_first<5>, grid, dim3(256), lds, s, c->wav, T, mpd ? 1 : 0, mpd ? P : sub, Hin, H[0], w.stride, w.pad, w.fold,
                               w.bias, w.Co, buf(0), P, (long long)w.Co * H[0] * P, (long long)H[0] * P, P, kDcSlope);
        GVC_LAUNCH_CHECK();
        return GVC_OK;
    }
    if (l < L - 1) return dc_conv(cv[l], buf(l - 1), buf(l), NB, H[l - 1], H[l], P, kDcSlope, s);
    const DcConv& wp = cv[L - 1];
    const int flat = H[L - 1] * P;          // (conv_post keeps the frame count: flat = H[L - 2] * P too)
    hipLaunchKernelGGL(k_disc_post, dim3(cdiv(flat, 64), NB), dim3(256), 0, s, buf(L - 2), wp.fold, wp.bias, buf(L - 1), wp.Ci, flat, P);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// everything a forward enqueues after the two waveforms are in c->wav
static int dc_body(gvc_disc* c, int B, int T, const DcRedJob* jobs, hipStream_t s) {
    int rc;
    for (int sub = 0; sub < c->n_sub; ++sub)
        for (int l = 0; l < c->n_layers; ++l)
            if ((rc = dc_layer(c, sub, l, B, T, s))) return rc;
    DcRedJob none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL(k_disc_red_partials, dim3(kDcRedBlocks, c->n_jobs), dim3(256), 0, s, jobs, none, c->part);
    GVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_disc_red_finish, dim3(c->n_jobs), dim3(256), 0, s, jobs, none, c->part, 1.0f, c->stats);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

extern "C" int gvc_disc_forward(gvc_disc* c, const float* y, const float* y_hat, int32_t B, int32_t T, float* stats, gvc_stream sv) {
    GVC_REQUIRE(c && y && y_hat && stats, GVC_ERR_ARG, "gvc_disc_forward: null argument");
    GVC_REQUIRE(c->arena, GVC_ERR_STATE, "gvc_disc_forward: no arena (gvc_disc_set_arena)");
    GVC_REQUIRE(gvc_disc_missing_weights(c) == 0, GVC_ERR_STATE, "%d discriminator weight tensors are not bound", gvc_disc_missing_weights(c));
    int rc = dc_check_shape(c, B, T);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)sv;
    const long long key = ((long long)B << 32) | (unsigned)T;
    auto it = c->plans.find(key);
    if (it == c->plans.end()) {
        if (c->plans.size() >= 32) dc_drop_plans(c);      // bounded cache: the sample count of an evaluation batch varies freely
        // the reduction jobs of this geometry: per sub-discriminator three logit means, then |f_r - f_g| per layer
        const int L = c->n_layers;
        std::vector<DcRedJob> jobs;
        std::vector<int> H(L);
        for (int sub = 0; sub < c->n_sub; ++sub) {
            dc_geometry(c, sub, T, H.data());
            const int P = c->dm.kind == GVC_DISC_MPD ? c->dm.periods[sub] : 1;
            auto job = [&](int l, int mode, bool gen) {
                const long long n = (long long)B * c->conv[sub][l].Co * H[l] * P;
                const float* base = c->arena + c->off[sub][l];
                DcRedJob j;
                memset(&j, 0, sizeof(j));
                j.a = gen ? base + n : base; j.b = base + n; j.n = n; j.mode = mode;
                jobs.push_back(j);
            };
            job(L - 1, 1, false);
            job(L - 1, 2, true);
            job(L - 1, 1, true);
            for (int l = 0; l < L; ++l) job(l, 0, false);
        }
        DcPlan pl;
        GVC_CHECK_HIP(hipMalloc((void**)&pl.jobs, jobs.size() * sizeof(DcRedJob)));
        hipError_t e = hipMemcpy(pl.jobs, jobs.data(), jobs.size() * sizeof(DcRedJob), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(pl.jobs); GVC_CHECK_HIP(e); }
        rc = capture_graph(c->cap_stream, &pl.ge, [&]() { return dc_body(c, B, T, pl.jobs, c->cap_stream); });
        if (rc) { (void)hipFree(pl.jobs); return rc; }
        it = c->plans.emplace(key, pl).first;
    }
    const size_t bytes = (size_t)B * T * sizeof(float);
    GVC_CHECK_HIP(hipMemcpyAsync(c->wav, y, bytes, hipMemcpyDeviceToDevice, s));
    GVC_CHECK_HIP(hipMemcpyAsync(c->wav + (size_t)B * T, y_hat, bytes, hipMemcpyDeviceToDevice, s));
    GVC_CHECK_HIP(hipGraphLaunch(it->second.ge, s));
    GVC_CHECK_HIP(hipMemcpyAsync(stats, c->stats, (size_t)c->n_jobs * sizeof(float), hipMemcpyDeviceToDevice, s));
    return GVC_OK;
}

extern "C" int gvc_disc_time_layer(gvc_disc* c, int32_t sub, int32_t layer, int32_t B, int32_t T, int32_t iters, float* avg_us, gvc_stream sv) {
    GVC_REQUIRE(c && avg_us && iters >= 1, GVC_ERR_ARG, "gvc_disc_time_layer: bad argument");
    GVC_REQUIRE(c->arena && gvc_disc_missing_weights(c) == 0, GVC_ERR_STATE, "gvc_disc_time_layer: no arena or unbound weights");
    GVC_REQUIRE(sub >= 0 && sub < c->n_sub && layer >= 0 && layer < c->n_layers, GVC_ERR_ARG, "gvc_disc_time_layer: sub %d layer %d", sub, layer);
    int rc = dc_check_shape(c, B, T);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)sv;
    hipEvent_t e0, e1;
    GVC_CHECK_HIP(hipEventCreate(&e0));
    GVC_CHECK_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 3 && !rc; ++i) rc = dc_layer(c, sub, layer, B, T, s);
    if (!rc && hipEventRecord(e0, s) != hipSuccess) rc = GVC_ERR_HIP;
    for (int i = 0; i < iters && !rc; ++i) rc = dc_layer(c, sub, layer, B, T, s);
    if (!rc && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) rc = GVC_ERR_HIP;
    float ms = 0.f;
    if (!rc && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = GVC_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == GVC_ERR_HIP) gvc::set_error("gvc_disc_time_layer: a HIP call failed");
    if (!rc) *avg_us = ms * 1000.f / (float)iters;
    return rc;
}

extern "C" int gvc_l1_mean(const float* a, const float* b, int64_t n, float scale, float* out, float* work, gvc_stream sv) {
    GVC_REQUIRE(a && b && out && work && n >= 1, GVC_ERR_ARG, "gvc_l1_mean: bad argument");
    hipStream_t s = (hipStream_t)sv;
    DcRedJob one;
    memset(&one, 0, sizeof(one));
    one.a = a; one.b = b; one.n = n; one.mode = 0;
    double* part = reinterpret_cast<double*>(work);
    hipLaunchKernelGGL(k_disc_red_partials, dim3(kDcRedBlocks, 1), dim3(256), 0, s, (const DcRedJob*)nullptr, one, part);
    GVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_disc_red_finish, dim3(1), dim3(256), 0, s, (const DcRedJob*)nullptr, one, part, scale, out);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}
