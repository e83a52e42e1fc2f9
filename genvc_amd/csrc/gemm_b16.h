// bf16 matrix-core GEMM for the GPT's multi-row passes (weight_dtype 4, "bf16_mfma"): C = epilogue(A W^T), both operands bf16 in
// the fragment-major layout below, products exact in fp32, fp32 accumulation (v_mfma_f32_16x16x32_bf16).
#pragma once
#include "gemm.h"

namespace gvc {

// "FB16" fragment-major layout of an [M][K] bf16 matrix (M % 16 == 0, K % 32 == 0), the analogue of FM16: each (16 rows x 32 k)
// block is stored as the 64 sixteen-byte fragments a wave feeds to v_mfma_f32_16x16x32_bf16 -- lane (m % 16) + 16 * ((k % 32) / 8)
// holds the 8 consecutive k of row m that start at k & ~7 -- so a block is 1 KiB contiguous: one global_load_lds of 16 bytes per
// lane for an activation block, one 16-byte global load per lane for a streamed weight fragment.  Index in bf16 elements.
__host__ __device__ __forceinline__ size_t fb16_index(int m, int k, int K) {
    return ((size_t)(m >> 4) * (K >> 5) + (k >> 5)) * 512 + (size_t)((((m & 15) + 16 * ((k & 31) >> 3)) << 3) + (k & 7));
}

// what the bf16 strip kernel's epilogue does beyond GemmEpi (bias, gelu_new, the QKV scatter, raw K-split partials):
struct B16Epi {
    const float* stats;      // folded LayerNorm: [M][2] = (mean, rstd) of the bf16 row the GEMM consumed; null: none
    const float* S;          // [N] S_r = sum_k bf16(W_rk g_k)
    const float* Cc;         // [N] C_r = sum_k W_rk b_k + bias_r      y = rstd (acc - mean S_r) + C_r  (G.e.bias is not added)
    unsigned short* c_b16;   // non-null: the result (after bias and activation) is rounded to bf16 and stored here in FB16 (row length N)
};

// Strip GEMM on bf16 matrix cores: G.A and G.Wt are FB16 matrices of bf16 elements (rows of A padded to 16; rows past M may hold
// anything finite or not: their results are never stored), N % 64 == 0, K % 32 == 0.  Same decomposition and arguments as
// launch_gemm_strip; one kernel family serves 1 .. max_rows rows.
int launch_gemm_strip_b16(GemmArgs G, const B16Epi& F, int sk_max, long long work_cap, int raw_partials, int* sk_used, hipStream_t s);
void gemm_b16_init_attributes();        // raises dynamic-LDS limits; call once, outside stream capture

// row-major fp32 [N][K] -> FB16 bf16, dst = bf16(src * gain[k]) rounded to nearest even (gain null: bf16(src), exact for values that
// are bf16 already); rows N .. Np - 1 (Np = N padded to 16) are zeroed
int launch_to_fb16(const float* src, unsigned short* dst, int N, int K, const float* gain, hipStream_t s);

// x_out[row] = x_in[row] + bias + sum_s part[s][row] as launch_ln_sum_rows (the same order); then, unless a_b16 is null, the row
// rounded to bf16 goes to a_b16 in FB16 and stats[row] = (mean, rstd) of the ROUNDED row (fp32, eps 1e-5): what the LayerNorm-folded
// GEMM consumes.  part null: the row is x_in alone.
int launch_ln_sum_rows_b16(const float* x_in, float* x_out, unsigned short* a_b16, float* stats, const float* part, int SK, const float* bias,
                           int rows, int d, hipStream_t s);

}  // namespace gvc
