// Test hook for the attention kernels (include/genvc_hip.h: gvc_attn_probe): one launch of one kernel class on the caller's buffers,
// every AttnArgs / AttnProjArgs / k_attn64_mfma argument a product caller sets taken from the case as it stands.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "gemm.h"
#include "gpt_kernels.h"
#include "attn64.h"
#include "forward_eval.h"

namespace gvc {

static int probe_attn64(const gvc_attn_case* c, hipStream_t s) {
    const dim3 grid((c->Tq + 15) / 16, c->n_head, c->batch);
    const float* q = c->q;
    const float* k = static_cast<const float*>(c->kbase);
    const float* v = static_cast<const float*>(c->vbase);
#define GVC_ATTN64(mask, nw)                                                                                                                 \
    hipLaunchKernelGGL((k_attn64_mfma<mask, nw>), grid, dim3(nw * 64), 0, s, q, k, v, (long long)c->ld, (long long)c->bs, c->Tq, c->Tk, c->out, \
                       c->out_rows, c->E, c->scale, c->out_fm16, c->fmask)
    if (c->nw == 4) { if (c->mask) GVC_ATTN64(true, 4); else GVC_ATTN64(false, 4); }
    else { if (c->mask) GVC_ATTN64(true, 16); else GVC_ATTN64(false, 16); }
#undef GVC_ATTN64
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

static int probe_fused_proj(const gvc_attn_case* c, hipStream_t s) {
    // fused_ok's conditions (gpt.hip) on the caller's numbers; the key count lives on the device
    GVC_REQUIRE(c->head_dim == 256 && c->n_head >= 1 && c->d == c->n_head * 256 && c->d % 16 == 0 && c->d <= 1024, GVC_ERR_ARG,
                "attn_probe: the fused kernel needs head_dim 256 and d = n_head * 256 <= 1024 (head_dim=%d n_head=%d d=%d)", c->head_dim, c->n_head, c->d);
    GVC_REQUIRE(c->seq_len && c->Wp && c->slots && c->max_seq >= 1, GVC_ERR_ARG, "attn_probe: the fused kernel needs slots, seq_len, Wp and max_seq");
    int32_t slot = -1, len = -1;
    GVC_CHECK_HIP(hipMemcpyAsync(&slot, c->slots, sizeof(slot), hipMemcpyDeviceToHost, s));
    GVC_CHECK_HIP(hipStreamSynchronize(s));
    GVC_REQUIRE(slot >= 0, GVC_ERR_ARG, "attn_probe: slot %d", slot);
    GVC_CHECK_HIP(hipMemcpyAsync(&len, c->seq_len + slot, sizeof(len), hipMemcpyDeviceToHost, s));
    GVC_CHECK_HIP(hipStreamSynchronize(s));
    GVC_REQUIRE(len >= 0 && len + 1 <= 8 * kFusedMaxKeys && len + 1 <= c->max_seq, GVC_ERR_ARG,
                "attn_probe: the fused kernel holds at most %d keys (seq_len[%d] + 1 = %d, max_seq %d)", 8 * kFusedMaxKeys, slot, len + 1, c->max_seq);
    AttnProjArgs F;
    F.q = c->q; F.kcache = c->kbase; F.vcache = c->vbase; F.slots = c->slots; F.seq_len = c->seq_len;
    F.max_seq = c->max_seq; F.n_head = c->n_head; F.d = c->d; F.scale = c->scale; F.Wp = c->Wp; F.part2 = c->out;
    if (c->kv_bf16) hipLaunchKernelGGL((k_attn_proj<256, 1>), dim3(c->d / 16, c->n_head), dim3(512), 0, s, F);
    else hipLaunchKernelGGL((k_attn_proj<256, 0>), dim3(c->d / 16, c->n_head), dim3(512), 0, s, F);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc

extern "C" int gvc_attn_probe(gvc_attn_case* c, gvc_stream sv) {
    using namespace gvc;
    GVC_REQUIRE(c && c->kind >= GVC_ATTN_ROWS && c->kind <= GVC_ATTN_64, GVC_ERR_ARG, "attn_probe: bad argument");
    GVC_REQUIRE(c->q && c->kbase && c->vbase && c->out && c->n_head >= 1, GVC_ERR_ARG, "attn_probe: q, kbase, vbase, out and n_head are needed");
    hipStream_t s = (hipStream_t)sv;
    int rc = GVC_OK;
    if (c->kind == GVC_ATTN_64) {
        GVC_REQUIRE((c->nw == 4 || c->nw == 16) && c->Tq >= 1 && c->Tk >= 1 && c->batch >= 1 && c->E == c->n_head * 64 && c->ld % 4 == 0 && c->bs % 4 == 0 &&
                    c->out_rows >= c->Tq && (!c->mask || c->fmask), GVC_ERR_ARG, "attn_probe: bad k_attn64_mfma case");
        rc = probe_attn64(c, s);
    } else if (c->kind == GVC_ATTN_FUSED_PROJ) {
        rc = probe_fused_proj(c, s);
    } else {
        AttnArgs A;
        memset(&A, 0, sizeof(A));
        A.q = c->q; A.q_stride = c->q_stride; A.kbase = c->kbase; A.vbase = c->vbase;
        A.k_batch_stride = c->k_batch_stride; A.k_head_stride = c->k_head_stride; A.k_row_stride = c->k_row_stride;
        A.T = c->T; A.slots = c->slots; A.base_len = c->base_len; A.causal = c->causal; A.n_keys = c->n_keys; A.scale = c->scale;
        A.out = c->out; A.out_stride = c->out_stride; A.out_fm16 = c->out_fm16; A.key_mask = c->key_mask; A.mask_stride = c->mask_stride;
        // (every load of the kernels is a float4 / uint2 of four consecutive elements)
        GVC_REQUIRE(c->T >= 1 && c->q_stride % 4 == 0 && c->k_row_stride % 4 == 0 && c->k_batch_stride % 4 == 0 && c->k_head_stride % 4 == 0 &&
                    c->out_stride % 4 == 0 && (c->causal || c->n_keys >= 1), GVC_ERR_ARG, "attn_probe: bad AttnArgs");
        if (c->kind == GVC_ATTN_ROWS) {
            GVC_REQUIRE(c->chunks >= 1 && c->rows >= 1 && (!c->direct || c->chunks == 1) && (!c->wide || c->head_dim == 256), GVC_ERR_ARG,
                        "attn_probe: rows case needs chunks >= 1 (1 when direct), rows >= 1, wide only with head_dim 256");
            rc = launch_attention_hd(c->head_dim, c->n_head, A, c->chunks, c->rows, c->direct != 0, s, c->wide != 0, c->kv_bf16 != 0);
        } else {
            GVC_REQUIRE(c->batch >= 1 && c->max_keys >= 1, GVC_ERR_ARG, "attn_probe: tile case needs batch and max_keys");
            c->taken = 0;
            c->ran = GVC_ATTN_RAN_NONE;
            if (c->kind == GVC_ATTN_TILE) {
                int lrc = GVC_OK;
                c->taken = launch_attention_tile(c->head_dim, c->n_head, A, c->batch, c->max_keys, s, c->kv_bf16 != 0, &lrc) ? 1 : 0;
                if (c->taken) rc = lrc;
            } else {
                rc = launch_attention_tile_masked(c->head_dim, c->n_head, A, c->batch, c->max_keys, s);
                c->taken = rc == GVC_OK;
            }
            // the launchers' rule RESTATED (they do not report their choice): up to 128 (padded) keys go to the kernel that keeps K and V whole
            // in LDS.  Keep equal to launch_attention_tile / launch_attention_tile_masked
            if (c->taken) c->ran = ((c->max_keys + 15) & ~15) <= 128 ? GVC_ATTN_RAN_SHORT : GVC_ATTN_RAN_TILED;
        }
    }
    const hipError_t he = hipStreamSynchronize(s);
    if (rc == GVC_OK && he != hipSuccess) { set_error("attn_probe: %s", hipGetErrorString(he)); rc = GVC_ERR_HIP; }
    return rc;
}
