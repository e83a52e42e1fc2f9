// bf16 matrix-core strip GEMM (see gemm_b16.h)
#include "gemm_b16.h"

namespace gvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- k_gemm_strip_b16: k_gemm_strip's decomposition on v_mfma_f32_16x16x32_bf16 ----
// A workgroup = 8 waves = one (m group of <= MTW 16-row tiles, 64-column n block, K split).  The group's A blocks (16 rows x 32 k,
// 1 KiB, FB16) are staged ONCE per workgroup in LDS by LDS-DMA in stages of KC k-blocks, two stage buffers; wave (wn, kh) streams
// the weight fragments of column tile wn for half kh of every stage straight from global memory into MFMA operands (16 bytes per
// lane per k-block, requested a stage ahead) and keeps MTW independent 16x16 accumulators.
// Per k-block (32 k) and wave: 1 global 16-byte load, MTW ds_read_b128, MTW MFMAs of 16 cycles (8 passes) -- the fp32 kernel spends
// 8 x MTW MFMAs of 32 cycles on the same 32 k.  What bounds the loop now, from the documented rates (LDS 128 B/clk per CU, bf16 MFMA
// 16x the fp32 rate) -- a model, NOT a counter measurement; what was measured is the whole GEMM (1.8x - 4.0x the
// fp32 strip kernel at 128 - 550 rows, i.e. far from the 16x of the MFMA rate, which is what a loop bound elsewhere looks like):
//   * LDS reads: every one of the four column tiles reads each A block of a stage once, 4 KC MTW KiB per stage and workgroup; at
//     128 B/clk that is 32 KC MTW cycles per stage, twice the 16 KC MTW cycles the stage's MFMAs take on a SIMD (two waves each);
//   * the stage's memory round trip (ASSUMED ~2000 cycles from L2 / HBM, not measured): with MTW <= 3 a stage's LDS reads are shorter
//     than that and the loop runs at one round trip per stage, hidden only by a second resident workgroup of the CU (two fit by their
//     LDS, <= 72 KiB each; residency was not measured either).
// By these rates the MFMA pipe is not the bound; launch_gemm_strip_b16's geometry model is built on the two terms above.
struct StripGeomB { int MG, NB, SK, mt, kb, raw; };       // m groups, n blocks, K splits, m tiles, 32-wide k blocks; raw: partials to G.work even when SK == 1

template <int MTW> struct StripCfgB {
    static constexpr int KC = MTW >= 5 ? 4 : 8;                      // k-blocks per stage: <= 36 KiB of A per stage
    static constexpr size_t stage_bytes = (size_t)2 * KC * MTW * 1024, tile_bytes = (size_t)MTW * 16 * 68 * 4;
    static constexpr size_t lds_bytes = stage_bytes > tile_bytes ? stage_bytes : tile_bytes;
};

template <int MTW, int T = 0>
__device__ __forceinline__ void strip_b16_read(f32x4 (&a)[MTW], unsigned addr) {
    if constexpr (T < MTW) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[T]) : "v"(addr), "n"(T * 1024));
        strip_b16_read<MTW, T + 1>(a, addr);
    }
}
template <int MTW>
__device__ __forceinline__ void strip_b16_wait(f32x4 (&a)[MTW]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < MTW; ++t) asm volatile("" : "+v"(a[t]));
}

// four consecutive columns n .. n + 3 of row m: LayerNorm fold or bias, activation, then the bf16 FB16 store, the QKV scatter or
// the row-major store -- fp32 math throughout
__device__ __forceinline__ void b16_store4(const GemmArgs& G, const B16Epi& F, int m, int n, float4 v) {
    const GemmEpi& e = G.e;
    if (F.stats) {
        const float2 st = *reinterpret_cast<const float2*>(F.stats + 2 * (size_t)m);
        const float4 s4 = *reinterpret_cast<const float4*>(F.S + n), c4 = *reinterpret_cast<const float4*>(F.Cc + n);
        v.x = st.y * (v.x - st.x * s4.x) + c4.x; v.y = st.y * (v.y - st.x * s4.y) + c4.y;
        v.z = st.y * (v.z - st.x * s4.z) + c4.z; v.w = st.y * (v.w - st.x * s4.w) + c4.w;
    } else if (e.bias) {
        const float4 b = *reinterpret_cast<const float4*>(e.bias + n);
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    }
    if (e.act == ACT_GELU_NEW) { v.x = gelu_new(v.x); v.y = gelu_new(v.y); v.z = gelu_new(v.z); v.w = gelu_new(v.w); }
    if (F.c_b16) {
        ushort4 o;
        o.x = f32_to_bf16(v.x); o.y = f32_to_bf16(v.y); o.z = f32_to_bf16(v.z); o.w = f32_to_bf16(v.w);
        *reinterpret_cast<ushort4*>(F.c_b16 + fb16_index(m, n, G.N)) = o;
        return;
    }
    if (e.qkv) {
        const int which = n / e.d;
        const int c = n - which * e.d;
        if (which == 0) {
            *reinterpret_cast<float4*>(G.C + (size_t)m * G.ldc + c) = v;
        } else {
            const int b = m / e.T, t = m - b * e.T;
            const int slot = e.slots[b];
            const int pos = t + (e.base_len ? e.base_len[slot] : 0);
            const int h = c / e.head_dim, j = c - h * e.head_dim;
            float* cache = which == 1 ? e.kcache : e.vcache;
            const size_t at = (((size_t)slot * e.n_head + h) * e.max_seq + pos) * e.head_dim + j;
            if (e.kv_bf16) {
                ushort4 o;
                o.x = f32_to_bf16(v.x); o.y = f32_to_bf16(v.y); o.z = f32_to_bf16(v.z); o.w = f32_to_bf16(v.w);
                *reinterpret_cast<ushort4*>(reinterpret_cast<unsigned short*>(cache) + at) = o;
            } else {
                *reinterpret_cast<float4*>(cache + at) = v;
            }
        }
        return;
    }
    *reinterpret_cast<float4*>(G.C + (size_t)m * G.ldc + n) = v;
}

template <int MTW>
__global__ __launch_bounds__(512) void k_gemm_strip_b16(const GemmArgs G, const B16Epi F, const StripGeomB S) {
    constexpr int KC = StripCfgB<MTW>::KC, KCW = KC / 2, NWV = 8;
    extern __shared__ __attribute__((aligned(16))) float strip_lds[];        // [2][KC][MTW][1 KiB]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 3, kh = wave >> 2;
    int id = blockIdx.x;
    const int nb = id % S.NB;       // n block fastest: where NB % 8 == 0 (N = 1024, 3072, 4096) the m groups / K splits of one n block share an
                                    // XCD and its L2; other widths (N = 256, 768) spread them over the XCDs and re-read the weights per XCD
    id /= S.NB;
    const int mg = id % S.MG, sk = id / S.MG;
    const int t_lo = (int)((long long)mg * S.mt / S.MG), nt = (int)((long long)(mg + 1) * S.mt / S.MG) - t_lo;     // <= MTW
    const int kb_lo = (int)((long long)sk * S.kb / S.SK), nkb = (int)((long long)(sk + 1) * S.kb / S.SK) - kb_lo;
    const int n_tile = nb * 4 + wn;
    // both operands are addressed in 1 KiB blocks (256 floats / 64 uint4): block (tile, k-block) of an FB16 matrix
    const uint4* wp = reinterpret_cast<const uint4*>(G.Wt) + ((size_t)n_tile * S.kb + kb_lo) * 64 + lane;
    const float* abase = G.A + ((size_t)t_lo * S.kb + kb_lo) * 256 + lane * 4;
    const int nst = (nkb + KC - 1) / KC;
    const unsigned lds_base = (unsigned)(size_t)strip_lds + (unsigned)lane * 16u;       // LDS byte address of this lane's fragment in block 0

    // this wave's share of a stage's A blocks: pairs p = wave + NWV i -> (t = p / KC, kc = p % KC)
    auto stage_a = [&](int st, int buf) {
        constexpr int NP = (MTW * KC + NWV - 1) / NWV;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int pidx = wave + NWV * i;
            const int t = pidx / KC, kc = pidx - t * KC;
            const int kbi = min(st * KC + kc, nkb - 1);            // (past the end: a valid block again, met by zero weights)
            if (pidx < MTW * KC && t < nt)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(abase + ((size_t)t * S.kb + kbi) * 256),
                                                 (__attribute__((address_space(3))) void*)(strip_lds + ((size_t)(buf * KC + kc) * MTW + t) * 256),
                                                 16, 0, 0);
        }
    };
    uint4 wnext[KCW], wcur[KCW];
    auto stage_w = [&](int st) {
#pragma unroll
        for (int j = 0; j < KCW; ++j)
            wnext[j] = wp[(size_t)min(st * KC + kh * KCW + j, nkb - 1) * 64];        // (past the end: a valid block again, zeroed at use)
    };
    f32x4 acc[MTW];
#pragma unroll
    for (int t = 0; t < MTW; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};

    stage_a(0, 0);
    stage_w(0);
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        // k-blocks past the end get zero weights, so that the k loop has no tail case; the select sits here, not at the load,
        // which it would wait for
#pragma unroll
        for (int j = 0; j < KCW; ++j) wcur[j] = st * KC + kh * KCW + j < nkb ? wnext[j] : make_uint4(0u, 0u, 0u, 0u);
        // everything this wave requested has landed (stage st of A, in LDS, included); past the barrier that holds for all
        // waves, and every wave is done reading the other buffer
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // (ds_read_b128 from inline asm, as in k_gemm_strip: a ds_read the compiler can see makes it drain vmcnt first)
        const unsigned ab = lds_base + (unsigned)((buf * KC + kh * KCW) * MTW * 1024);
        f32x4 af[2][MTW];
        strip_b16_read<MTW>(af[0], ab);
#pragma unroll
        for (int j = 0; j < KCW; ++j) {
            strip_b16_wait<MTW>(af[j & 1]);
            if (j + 1 < KCW) strip_b16_read<MTW>(af[(j + 1) & 1], ab + (unsigned)((j + 1) * MTW * 1024));
            const bf16x8 wv = __builtin_bit_cast(bf16x8, wcur[j]);
#pragma unroll
            for (int t = 0; t < MTW; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[j & 1][t]), wv, acc[t], 0, 0, 0);
            // the next stage's requests go out behind the first k-block's MFMAs
            if (j == 0 && st + 1 < nst) {
                stage_a(st + 1, buf ^ 1);
                stage_w(st + 1);
            }
        }
    }
    // Epilogue through LDS as in k_gemm_strip: the workgroup's [16 * MTW rows][64 columns] tile (lower k half + upper k half, a
    // fixed order), then float4 pieces of a row per lane
    constexpr int LDT = 68;
    __syncthreads();                    // every wave is done with the stage buffers
    float* T = strip_lds;
    if (kh == 0) {
#pragma unroll
        for (int t = 0; t < MTW; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) T[(t * 16 + 4 * (lane >> 4) + q) * LDT + wn * 16 + (lane & 15)] = acc[t][q];
    }
    __syncthreads();
    if (kh == 1) {
#pragma unroll
        for (int t = 0; t < MTW; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) T[(t * 16 + 4 * (lane >> 4) + q) * LDT + wn * 16 + (lane & 15)] += acc[t][q];
    }
    __syncthreads();
    const bool part = S.SK > 1 || S.raw;
    const int row = (wave * 4 + (lane >> 4)) & 15;          // wave w stores rows 4 (w & 3) .. + 3 of the tiles t with t % 2 == kh
    const int col = 4 * (lane & 15);
    const int n = nb * 64 + col;
#pragma unroll
    for (int tt = 0; tt < (MTW + 1) / 2; ++tt) {
        const int t = kh + tt * 2;
        const int m = (t_lo + t) * 16 + row;
        if (t < nt && m < G.M) {
            const float4 v = *reinterpret_cast<const float4*>(T + (t * 16 + row) * LDT + col);
            if (part) *reinterpret_cast<float4*>(G.work + ((size_t)sk * G.M + m) * G.N + n) = v;
            else b16_store4(G, F, m, n, v);
        }
    }
}

// Geometry: the (tiles per group w, K split) pair with the shortest modelled time, in cycles.  A workgroup runs cdiv(kb / sk, KC)
// stages; a stage costs the larger of its memory round trip (kLat) and the LDS reads of the workgroups that share the CU
// (32 KC w cycles each, see above); the resident workgroups of a CU (two: <= 72 KiB of LDS each) run their stages side by side,
// further rounds back to back.  A K split of a GEMM with its own epilogue pays the epilogue launch.  kLat and the 20000-cycle price of
// that launch (~8 us, the dependent-launch cost DESIGN.md section 4.3 reports) are assumptions of the model, not fitted to measurements;
// the model only ranks geometries, and the times it leads to are the measured ones of DESIGN.md section 4.19.
int launch_gemm_strip_b16(GemmArgs G, const B16Epi& F, int sk_max, long long work_cap, int raw_partials, int* sk_used, hipStream_t s) {
    GVC_REQUIRE(G.M >= 1 && G.N >= 64 && G.N % 64 == 0 && G.K >= 32 && G.K % 32 == 0 && G.conv_cin == 0 && G.a_act == 0 && G.ldc % 4 == 0 &&
                    !G.e.resid && !G.e.resid2 && !G.e.c_fm16 && !G.e.geglu && G.e.out_scale == 0.f && !G.att_part &&
                    (G.e.act == ACT_NONE || G.e.act == ACT_GELU_NEW) && (!G.e.qkv || (G.e.d % 64 == 0 && G.e.head_dim % 4 == 0)), GVC_ERR_ARG,
                "bf16 strip gemm: unsupported shape or epilogue M=%d N=%d K=%d (FB16 operands, N %% 64 == 0, K %% 32 == 0)", G.M, G.N, G.K);
    StripGeomB S;
    S.mt = cdiv(G.M, 16); S.NB = G.N / 64; S.kb = G.K / 32;
    GVC_REQUIRE(!raw_partials || (G.work && (long long)G.M * G.N <= work_cap), GVC_ERR_ARG, "bf16 strip gemm: raw partials need a work buffer");
    const bool own_epi = F.stats || F.c_b16 || G.e.qkv || G.e.act != ACT_NONE;       // what k_splitk_epilogue cannot finish
    if (!G.work || (own_epi && !raw_partials)) sk_max = 1;
    if (sk_max < 1) sk_max = 1;
    if (sk_max > 8) sk_max = 8;
    int best_w = 0, best_sk = 1;
    double best = 1e30;
    constexpr double kLat = 2000.0;
    for (int w = 1; w <= 9; ++w) {
        const int MG = cdiv(S.mt, w);
        if (cdiv(S.mt, MG) != w) continue;              // the balanced partition's largest group: only exact fits are candidates
        const int KC = w >= 5 ? 4 : 8;
        for (int sk = 1; sk <= sk_max; ++sk) {
            if (sk > 1 && S.kb / sk < 4) break;
            if (sk > 1 && (long long)sk * G.M * G.N > work_cap) break;
            const long long wgs = (long long)MG * S.NB * sk;
            const int rounds = cdiv((int)wgs, 512), share = wgs > 256 ? 2 : 1;
            const double lds = 32.0 * KC * w * share;
            const double cost = (double)rounds * (cdiv(cdiv(S.kb, sk), KC) * (lds > kLat ? lds : kLat) + kLat) +
                                (sk > 1 && !raw_partials ? 20000.0 : 0.0);
            if (cost < best) { best = cost; best_w = w; best_sk = sk; }
        }
    }
    GVC_REQUIRE(best_w > 0, GVC_ERR_ARG, "bf16 strip gemm: no geometry for M=%d N=%d K=%d", G.M, G.N, G.K);
    S.MG = cdiv(S.mt, best_w); S.SK = best_sk;
    S.raw = raw_partials && G.work ? 1 : 0;
    G.SK = best_sk;
    if (sk_used) *sk_used = best_sk;
    const dim3 grid(S.MG * S.NB * S.SK);
#define GVC_STRIP_B16(w)                                                                                              \
    case w:                                                                                                           \
        hipLaunchKernelGGL((k_gemm_strip_b16<w>), grid, dim3(512), StripCfgB<w>::lds_bytes, s, G, F, S);              \
        break;
    switch (best_w) { GVC_STRIP_B16(1) GVC_STRIP_B16(2) GVC_STRIP_B16(3) GVC_STRIP_B16(4) GVC_STRIP_B16(5) GVC_STRIP_B16(6) GVC_STRIP_B16(7) GVC_STRIP_B16(8) GVC_STRIP_B16(9) }
#undef GVC_STRIP_B16
    GVC_LAUNCH_CHECK();
    if (best_sk > 1 && !raw_partials) {
        const long long mn = (long long)G.M * G.N;
        int gx = (int)((mn + 255) / 256);
        if (gx > 2048) gx = 2048;
        hipLaunchKernelGGL(k_splitk_epilogue, dim3(gx, 1, 1), dim3(256), 0, s, G);
        GVC_LAUNCH_CHECK();
    }
    return GVC_OK;
}

void gemm_b16_init_attributes() {
#define GVC_STRIP_B16_ATTR(w) \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_strip_b16<w>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    GVC_STRIP_B16_ATTR(1) GVC_STRIP_B16_ATTR(2) GVC_STRIP_B16_ATTR(3) GVC_STRIP_B16_ATTR(4) GVC_STRIP_B16_ATTR(5) GVC_STRIP_B16_ATTR(6)
    GVC_STRIP_B16_ATTR(7) GVC_STRIP_B16_ATTR(8) GVC_STRIP_B16_ATTR(9)
#undef GVC_STRIP_B16_ATTR
}

// a thread converts the 8 consecutive k of one fragment
__global__ void k_to_fb16(const float* src, unsigned short* dst, int N, int Np, int K, const float* gain) {
    const size_t n8 = (size_t)Np * (K / 8);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / (K / 8)), k = (int)(i % (K / 8)) * 8;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (n < N) {
            const float* p = src + (size_t)n * K + k;
            float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
            if (gain) {
                const float4 ga = *reinterpret_cast<const float4*>(gain + k), gb = *reinterpret_cast<const float4*>(gain + k + 4);
                a.x *= ga.x; a.y *= ga.y; a.z *= ga.z; a.w *= ga.w; b.x *= gb.x; b.y *= gb.y; b.z *= gb.z; b.w *= gb.w;
            }
            o.x = (unsigned)f32_to_bf16(a.x) | ((unsigned)f32_to_bf16(a.y) << 16); o.y = (unsigned)f32_to_bf16(a.z) | ((unsigned)f32_to_bf16(a.w) << 16);
            o.z = (unsigned)f32_to_bf16(b.x) | ((unsigned)f32_to_bf16(b.y) << 16); o.w = (unsigned)f32_to_bf16(b.z) | ((unsigned)f32_to_bf16(b.w) << 16);
        }
        *reinterpret_cast<uint4*>(dst + fb16_index(n, k, K)) = o;
    }
}

int launch_to_fb16(const float* src, unsigned short* dst, int N, int K, const float* gain, hipStream_t s) {
    GVC_REQUIRE(src && dst && N >= 1 && K >= 32 && K % 32 == 0, GVC_ERR_ARG, "to_fb16: bad shape N=%d K=%d", N, K);
    const int Np = (N + 15) & ~15;
    const size_t n8 = (size_t)Np * (K / 8);
    const int gx = (int)(n8 / 256 + 1 < 2048 ? n8 / 256 + 1 : 2048);
    hipLaunchKernelGGL(k_to_fb16, dim3(gx), dim3(256), 0, s, src, dst, N, Np, K, gain);
    GVC_LAUNCH_CHECK();
    return GVC_OK;
}

}  // namespace gvc

// the layout's index function as the host sees it (include/genvc_hip.h)
extern "C" int64_t gvc_fb16_index(int32_t m, int32_t k, int32_t K) { return (int64_t)gvc::fb16_index(m, k, K); }
