// The body of k_conv_lds and k_conv_lds_k11 (conv_lds.h), included into both: the two kernels differ only in MAXS, the number of
// reduction steps per wave whose B operands are requested up front and held in registers.  It is text, not a function template, so
// that the instantiations of k_conv_lds compile to what they compiled to before k_conv_lds_k11 existed.
// Expects in scope: CI, NW, NSUM, SPLIT, MAXS (compile-time constants) and `const ConvLdsArgs A`.
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int XS = CI + 4, NTH = NW * 64, C4 = CI / 4, CB = CI / 16;
    constexpr int MT = conv_lds_mt(CI, SPLIT), TF = 16 * MT;       // 16-frame M tiles, frames per workgroup
    float* Xs = lds;                       // [R][XS]
    float* red = lds;                      // [NW][4 * MT][64] after the MFMA loop (aliases Xs)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int jb = blockIdx.y / A.ntiles, tile = blockIdx.y - jb * A.ntiles;
    const ConvLdsJob J = A.job[SPLIT ? 0 : jb];
    const int t0 = blockIdx.x * TF, b = blockIdx.z;
    const int S = A.stride;
    const int nsteps = J.k * CB, R = (TF - 1) * S + (J.k - 1) * J.dil + 1, RH = (R + S - 1) / S;      // input row r lives in LDS row (r % S)*RH + r / S
    // this wave's B operands: steps wave, wave + NW, ...; requested before anything else
    const float4* wp = J.wp + (SPLIT ? (size_t)jb * A.wp_js : 0) + (size_t)tile * nsteps * 64 + lane;
    float4 wv[MAXS];
#pragma unroll
    for (int u = 0; u < MAXS; ++u) wv[u] = wp[(size_t)min(wave + NW * u, nsteps - 1) * 64];
    const float bn = J.b ? J.b[tile * 16 + (lane & 15)] : 0.f;
    __builtin_amdgcn_sched_barrier(0);
    // input rows -> LDS: UL requests per thread go out before the first LDS store (rows past the buffer only feed frames >= T)
    const int last_row = A.x_rows - 1, row0 = A.x_row0 + t0 * S + J.row_off;
    const float* xb = A.x + (size_t)b * A.x_bs + (size_t)jb * A.x_ps;
    constexpr int UL = NSUM == 1 ? (CI >= 512 ? 9 : 8) : 4;
    for (int i0 = tid; i0 < R * C4; i0 += NTH * UL) {
        float4 xv[UL][NSUM];
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int i = min(i0 + u * NTH, R * C4 - 1);
            const float* src = xb + (size_t)min(row0 + i / C4, last_row) * A.ldx + (i % C4) * 4;
#pragma unroll
            for (int p = 0; p < NSUM; ++p) xv[u][p] = *reinterpret_cast<const float4*>(src + (size_t)p * A.x_ss);
        }
        __builtin_amdgcn_sched_barrier(0);         // (the scheduler would sink every request to just above its store)
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int i = i0 + u * NTH;
            if (i < R * C4) {
                float4 v = xv[u][0];
                if constexpr (NSUM > 1) {
#pragma unroll
                    for (int p = 1; p < NSUM; ++p) { v.x += xv[u][p].x; v.y += xv[u][p].y; v.z += xv[u][p].z; v.w += xv[u][p].w; }
                    v.x *= A.x_scale; v.y *= A.x_scale; v.z *= A.x_scale; v.w *= A.x_scale;
                }
                v.x = v.x > 0.f ? v.x : v.x * A.slope; v.y = v.y > 0.f ? v.y : v.y * A.slope;
                v.z = v.z > 0.f ? v.z : v.z * A.slope; v.w = v.w > 0.f ? v.w : v.w * A.slope;
                const int r = i / C4;
                *reinterpret_cast<float4*>(&Xs[((r % S) * RH + r / S) * XS + (i % C4) * 4]) = v;
            }
        }
    }
    // thread (wave, lane) will finish accumulator registers r = wave, wave + NW, ... of the tile -- frame 16*(r/4) + 4*(lane/16) + r%4 --
    // and asks for its residuals now, so that the round trip hides under the matrix work
    constexpr int RPW = 4 * MT / NW;
    const int n = tile * 16 + (lane & 15);
    const size_t ob = (size_t)b * A.y_bs + A.y_off + n;
    float r1[RPW];
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int r = wave + NW * rr, m = 16 * (r >> 2) + 4 * (lane >> 4) + (r & 3);
        r1[rr] = (A.resid && t0 + m < A.T) ? A.resid[ob + (size_t)jb * A.r_ps + (size_t)(t0 + m) * A.ldy] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    hf_f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
    const int fi = lane & 15, fg = lane >> 4;
    auto step = [&](int it, const float4& w4) {
        const int tap = it / CB, cb = it - tap * CB;
        const int ro = tap * J.dil;
        const float* xp = &Xs[((ro % S) * RH + ro / S + fi) * XS + 16 * cb + 4 * fg];
        float4 a[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const float4*>(xp + 16 * t * XS);
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, w4.x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, w4.y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, w4.z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, w4.w, acc[t], 0, 0, 0);
    };
#pragma unroll
    for (int u = 0; u < MAXS; ++u)
        if (wave + NW * u < nsteps) step(wave + NW * u, wv[u]);
    for (int it = wave + NW * MAXS; it < nsteps; it += NW) step(it, wp[(size_t)it * 64]);      // (more taps than any GenVC config has)
    __syncthreads();                      // everyone is done reading Xs: the region becomes the reduction buffer
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) red[(wave * 4 * MT + 4 * t + v) * 64 + lane] = acc[t][v];
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int r = wave + NW * rr, m = 16 * (r >> 2) + 4 * (lane >> 4) + (r & 3);
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += red[(w * 4 * MT + r) * 64 + lane];
        if constexpr (!SPLIT) {
            v += bn;
            if (A.resid) v += r1[rr];
            v = conv_lds_act(v, A.act);
        }
        if (t0 + m < A.T) {
            float* dst = A.y + ob + (size_t)jb * A.y_ps + (size_t)(t0 + m) * A.ldy;
            // (partial sums are handed to another workgroup: write-through stores and, below, cache-bypassing loads -- a
            // __threadfence() here writes back the whole L2 of the XCD, 50 us for this kernel)
            if constexpr (SPLIT) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else *dst = v;
        }
    }
    if constexpr (SPLIT) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this workgroup's partial sums have landed before its arrival is counted
        __syncthreads();
        if (tid == 0) {
            int* cn = A.cnt + ((size_t)b * gridDim.x + blockIdx.x) * A.ntiles + tile;
            const int last = __hip_atomic_fetch_add(cn, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.split - 1;
            if (last) __hip_atomic_store(cn, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // every slice has arrived: ready for the next call
            reinterpret_cast<int*>(lds)[0] = last;          // (the reduction buffer was consumed before the barrier above)
        }
        __syncthreads();
        if (!reinterpret_cast<const int*>(lds)[0]) return;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = wave + NW * rr, m = 16 * (r >> 2) + 4 * (lane >> 4) + (r & 3);
            if (t0 + m >= A.T) continue;
            const float* pp = A.y + ob + (size_t)(t0 + m) * A.ldy;
            float v = 0.f;
            for (int p = 0; p < A.split; ++p) v += __hip_atomic_load(pp + (size_t)p * A.y_ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const size_t o = (size_t)b * A.yf_bs + A.yf_off + (size_t)(t0 + m) * A.ldy + n;
            v += bn;
            if (A.resid) v += A.resid[o];              // (SPLIT: the residual is indexed like yf and may BE yf: one thread reads and writes an element)
            A.yf[o] = conv_lds_act(v, A.act);
        }
    }
