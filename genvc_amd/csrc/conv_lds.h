// One-round-trip convolution kernel shared by the vocoder (hifigan.hip) and the ContentVec feature extractor (hubert.hip).
#pragma once
#include "gemm.h"

namespace gvc {

// ---------------------------------------------------------------------------------------------
// Convolutions over time-major activations whose K = taps * CI extent is small -- HiFi-GAN: ResBlock convs (CI = 32 / 64 / 128 channels
// in and out, <= 7 taps, dilation <= 12), the polyphase ConvTranspose1d layers (3 taps of CI = 256 / 128 / 64), conv_pre in 64-channel
// slices; ContentVec: the strided feature-extractor convs 1..6 (2-3 taps of CI = 512).  Instead of the tiled GEMM's k-loop (one
// global->LDS->sync round trip per 32 columns: 11 us for 0.05 GFLOP) a workgroup pays ONE memory round trip:
//   * it owns 32 (64 when CI <= 64) frames x 16 output columns; their (frames-1)*stride + (k-1)*dil + 1 input rows go to LDS once
//     (leaky-ReLU -- and, for the input of a HiFi-GAN stage, the sum of the three ResBlock outputs and the 1/3 -- applied on the way
//     in; rows of a strided conv are stored de-interleaved by row % stride, so the fragment reads stay bank-conflict-free);
//   * weights are stored in MFMA fragment order (FM16, gemm.h) and go straight from global memory into registers, 1 KiB per
//     wave-wide load, all of a wave's loads in flight before the input rows are staged;
//   * the NW waves split the (tap, 16-channel block) steps of the reduction (v_mfma_f32_16x16x4_f32, two M tiles share the B
//     operand) and combine through LDS; bias, residual and GELU in the epilogue.
// The three ResBlocks of a stage are independent given the stage input (hifigan.py:224-229: xs += resblocks[i*nk + j](x)), so
// ONE launch runs the first conv of all three (grid.y = job x column tile) and a second launch the second convs; each ResBlock
// writes its own output plane and the consumer of the stage adds the planes while staging, in the reference's order.
// ---------------------------------------------------------------------------------------------
// 16-frame M tiles per workgroup of k_conv_lds: 64 frames for the narrow late stages (thousands of frames: half the workgroups, every
// one resident at once), 32 otherwise
__host__ __device__ constexpr int conv_lds_mt(int ci, bool split) { return (ci <= 64 && !split) ? 4 : 2; }

__device__ __forceinline__ float conv_lds_act(float v, int act) {
    if (act == ACT_GELU_ERF) return gelu_erf(v);
    if (act == ACT_RELU) return v > 0.f ? v : 0.f;
    return v;
}

struct ConvLdsJob {
    const float4* wp;                    // FM16 copy of [N][k*CI]
    const float* b;                      // [N]
    int k, dil, row_off;                 // output frame t reads input rows x_row0 + t*stride + row_off + j*dil, j < k
};

struct ConvLdsArgs {
    // input: time-major [B][x_rows][ldx]; job j reads plane(s) at x + j*x_ps (x_ps = 0: every job reads the same input); row indices
    // are clamped to x_rows - 1 (rows past the end only feed frames >= T)
    const float* x; long long x_bs, x_ps, x_ss;      // x_ss: distance between the NSUM planes that are added while staging
    float x_scale, slope;                            // staged value = lrelu(x_scale * (p0 + p1 + p2)); x_scale only with NSUM > 1
    // output element (t, n) of job j, batch b: y[b*y_bs + j*y_ps + y_off + t*ldy + n]; resid (nullable) is indexed the same way
    float* y; long long y_bs, y_ps, y_off; int ldy;
    const float* resid; long long r_ps;
    int T, ntiles;                                   // output frames, N / 16
    int ldx;                                         // floats between input rows (CI, or more when the jobs are channel slices)
    int x_row0, x_rows, stride;                      // first input row of frame 0 (the padding of a padded buffer), rows per batch element, conv stride
    int act;                                         // GemmAct applied after bias and residual (ACT_NONE / ACT_RELU / ACT_GELU_ERF)
    // SPLIT (conv_pre: few outputs, K = 7 * 1024): job j < split is the channel slice [j*CI, (j+1)*CI) of every tap -- x_ps = CI, weights
    // job[0].wp + j*wp_js -- and writes RAW partial sums to plane j of y; the last workgroup to finish a tile (cnt) adds the
    // planes in order, adds the bias (and resid, indexed like yf), applies act and writes yf[b*yf_bs + yf_off + t*ldy + n]
    int split; long long wp_js; int* cnt;
    float* yf; long long yf_bs, yf_off;
    ConvLdsJob job[3];
};

typedef float hf_f32x4 __attribute__((ext_vector_type(4)));

// steps per wave whose B operands are held in registers (7 taps: 3.5 / 3.5 / 7; ups: 6; 3 x 512: 12); further steps load theirs in the loop
__host__ __device__ constexpr int conv_lds_maxs(int ci) { return ci <= 64 ? 4 : (ci >= 512 ? 12 : 8); }
// the same for the 11-tap convs of ResBlock1 (k_conv_lds_k11): ceil(11 * CI / 16 / NW) = 6 / 6 / 11 for CI = 32 / 64 / 128
__host__ __device__ constexpr int conv_lds_maxs_k11(int ci, int nw) { return (11 * (ci / 16) + nw - 1) / nw; }

template <int CI, int NW, int NSUM, bool SPLIT = false>
__global__ __launch_bounds__(NW * 64) void k_conv_lds(const ConvLdsArgs A) {
    constexpr int MAXS = conv_lds_maxs(CI);
#include "conv_lds_body.h"
}

// The same workgroup for launches that hold an 8..11-tap job (HiFi-GAN ResBlock1, kernels 3 / 7 / 11): every step's B operand is
// requested before the input rows are staged, as k_conv_lds does for <= 7 taps (there, taps 8.. would wait for their weights inside the
// MFMA loop).  CI = 32 / 64 / 128 only, one input plane, no K split.
template <int CI, int NW>
__global__ __launch_bounds__(NW * 64) void k_conv_lds_k11(const ConvLdsArgs A) {
    constexpr int NSUM = 1, MAXS = conv_lds_maxs_k11(CI, NW);
    constexpr bool SPLIT = false;
#include "conv_lds_body.h"
}

// conv weights [Co][Ci][k] (the reference's layout) -> per channel slice s (CS channels) the FM16 copy of [Co][k*CS] (column tap*CS + c):
// [Ci/CS][FM16].  CS = Ci: the one FM16 matrix of an unsplit conv.
static __global__ void k_conv_pack_slices(const float* w, float* out, int Co, int Ci, int k, int CS) {
    const int K = k * CS;
    const size_t per = (size_t)Co * K, n4 = per * (Ci / CS) / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int sl = (int)(i * 4 / per);
        const size_t r = i * 4 - (size_t)sl * per;
        const int n = (int)(r / K), kc = (int)(r % K), tap = kc / CS, cl = kc % CS;
        const float* src = w + ((size_t)n * Ci + sl * CS + cl) * k + tap;
        *reinterpret_cast<float4*>(out + (size_t)sl * per + fm16_index(n, kc, K)) = make_float4(src[0], src[k], src[2 * k], src[3 * k]);
    }
}

// K-split launch (k_conv_lds<CS, 8, 1, true>): A.split channel slices of CS = 64 or 256 channels, partial sums in A.y, result in A.yf
static inline int launch_conv_lds_split(int cs, const ConvLdsArgs& A, int B, size_t lds, hipStream_t s) {
    const dim3 grid(cdiv(A.T, 32), A.split * A.ntiles, B);
    if (cs == 64) hipLaunchKernelGGL((k_conv_lds<64, 8, 1, true>), grid, dim3(512), lds, s, A);
    else if (cs == 256) hipLaunchKernelGGL((k_conv_lds<256, 8, 1, true>), grid, dim3(512), lds, s, A);
    else return GVC_ERR_UNSUPPORTED;
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// LDS bytes of k_conv_lds: the input rows, later the reduction buffer
static inline size_t conv_lds_bytes(int ci, int k, int dil, bool split = false, int stride = 1) {
    const int mt = conv_lds_mt(ci, split), R = (16 * mt - 1) * stride + (k - 1) * dil + 1, RH = (R + stride - 1) / stride;
    const size_t stage = (size_t)RH * stride * (ci + 4), red = (size_t)8 * 4 * mt * 64;
    return (stage > red ? stage : red) * sizeof(float);
}
constexpr size_t kConvLdsMax = 150 * 1024;
static inline bool conv_lds_ci_ok(int ci) { return ci == 32 || ci == 64 || ci == 128 || ci == 256 || ci == 512; }

#define GVC_CONV_LDS_FOR_EACH(X) X(32, 4) X(64, 8) X(128, 8) X(256, 8) X(512, 8)
#define GVC_CONV_LDS_K11_FOR_EACH(X) X(32, 4) X(64, 8) X(128, 8)
static inline bool conv_lds_k11_ok(int ci, int k) { return (ci == 32 || ci == 64 || ci == 128) && k > 7 && k <= 11; }

// up to ~150 KB of dynamic LDS: raise the per-kernel limits once, outside any capture
static inline void conv_lds_init_attributes() {
#define GVC_CL_ATTR(CI, NW)                                                                                                                   \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_lds<CI, NW, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_lds<CI, NW, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    GVC_CONV_LDS_FOR_EACH(GVC_CL_ATTR)
#undef GVC_CL_ATTR
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_lds<64, 8, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_lds<256, 8, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
#define GVC_CL_ATTR(CI, NW) \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_lds_k11<CI, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    GVC_CONV_LDS_K11_FOR_EACH(GVC_CL_ATTR)
#undef GVC_CL_ATTR
    (void)hipGetLastError();
}

// grid (frame tiles, jobs x column tiles, batch)
static inline int launch_conv_lds(int ci, int nsum, const ConvLdsArgs& A, int njobs, int B, size_t lds, hipStream_t s) {
    const dim3 grid(cdiv(A.T, 16 * conv_lds_mt(ci, false)), njobs * A.ntiles, B);
#define GVC_CL_LAUNCH(CI, NW)                                                                            \
    if (ci == CI) {                                                                                      \
        if (nsum == 1) hipLaunchKernelGGL((k_conv_lds<CI, NW, 1>), grid, dim3(NW * 64), lds, s, A);     \
        else hipLaunchKernelGGL((k_conv_lds<CI, NW, 3>), grid, dim3(NW * 64), lds, s, A);               \
    }
    GVC_CONV_LDS_FOR_EACH(GVC_CL_LAUNCH)
#undef GVC_CL_LAUNCH
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

// the same grid on k_conv_lds_k11: launches whose widest job has 8..11 taps (conv_lds_k11_ok)
static inline int launch_conv_lds_k11(int ci, const ConvLdsArgs& A, int njobs, int B, size_t lds, hipStream_t s) {
    const dim3 grid(cdiv(A.T, 16 * conv_lds_mt(ci, false)), njobs * A.ntiles, B);
    if (!(ci == 32 || ci == 64 || ci == 128)) return GVC_ERR_UNSUPPORTED;
#define GVC_CL_LAUNCH(CI, NW) \
    if (ci == CI) hipLaunchKernelGGL((k_conv_lds_k11<CI, NW>), grid, dim3(NW * 64), lds, s, A);
    GVC_CONV_LDS_K11_FOR_EACH(GVC_CL_LAUNCH)
#undef GVC_CL_LAUNCH
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc
