// publish_line: does it matter HOW MANY store instructions assemble one 128-byte line of a hand-off buffer?  (profiles/decode_publish_lines.md)
//   256 workgroups x (8 consumer waves + 1 loader wave), all resident, the one-launch decode step's LDS footprint.  Per round every workgroup
//   publishes ONE aligned 128-byte line of sixteen {value, tag} granules (write-through, sc1) where phase BC of the step puts its sixteen
//   (plane wg % 4, granules [16 (wg / 4), +16) of a 4 x 1024 buffer), and every workgroup gathers all 32 KB with the step's gather<1, 4>:
//   one 16-byte sc1 load per lane and plane, the last plane polled as the sentinel, the other three read behind it, their tags checked.
//   Only the way the line is written varies:
//     0  sixteen single-lane 8-byte stores, two per wave (lane 0: granule w, lane 1: granule w + 8) -- what phase BC does
//     1  eight two-lane stores (one per wave, 16 bytes)
//     2  four four-lane stores (waves 0..3, 32 bytes each)
//     3  ONE instruction of 16 lanes x 8 bytes by the wave that arrives last at an LDS counter; values staged through LDS
//     4  ONE instruction of 8 lanes x 16 bytes, staged the same way
//     5  ONE instruction of 16 lanes x 8 bytes by wave 0 without staging (what the staging itself costs: 3 against 5)
//   Reported per run: the time from the LAST store of a round (any workgroup, stamped behind the store's issue) to the LAST workgroup whose
//   eight waves have the round in LDS (stamped behind its barrier), median / mean / p90 over the stamped rounds, idle and beside a loader
//   wave per workgroup that streams 16 KiB LDS-DMA fills from HBM, one in flight.  Every spin is bounded; exit code 1 on a time-out or a
//   wrong value.
// hipcc --offload-arch=gfx950 -O3 -o publish_line publish_line.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
constexpr int kG = 256, kCW = 8, kThreads = (kCW + 1) * 64, kSlot = 16384, kRing = 8;
constexpr int kWarm = 16, kRounds = 128 + kWarm;            // rounds per launch; the first kWarm are not stamped
constexpr int kPlane = 1024, kPlanes = 4, kBufGran = kPlane * kPlanes;      // granules of one buffer; four buffers in rotation
constexpr int kPad = 23872;                                  // the step's other LDS (hidden units, phase input, attention scratch, control)
constexpr unsigned kSpinLimit = 300000u;
// LDS behind the ring and the pad
constexpr int kOffStage = kRing * kSlot + kPad;              // float[16]
constexpr int kOffCtl = kOffStage + 64;                      // [0] barrier arrivals, [1] staging arrivals, [2] abort, [3] consumers done
constexpr int kOffStamp = kOffCtl + 64;                      // unsigned[kRounds - kWarm][kCW + 1]: store issued by wave w | round ready
constexpr size_t kLds = kOffStamp + (size_t)(kRounds - kWarm) * (kCW + 1) * 4;

struct Args {
    unsigned long long* gran;   // [4][kBufGran]
    const char* w;
    size_t w_bytes;
    unsigned* stamps;           // [kG][kRounds - kWarm][kCW + 1], low 32 bits of the 100 MHz wall clock
    int* err;                   // [0] time-outs, [1] wrong values
    unsigned salt;
    int stream;
};

__device__ __forceinline__ float val_of(unsigned tag, int g) { return (float)((tag * 2654435761u + (unsigned)g * 40503u) >> 8); }
__device__ __forceinline__ unsigned lds_ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_st(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void put8(__amdgpu_buffer_rsrc_t rs, int gi, unsigned tag, float v) {
    u32x2 g = {__float_as_uint(v), tag};
    __builtin_amdgcn_raw_buffer_store_b64(g, rs, gi * 8, 0, 16);
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_line(const Args A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* stage = reinterpret_cast<float*>(smem + kOffStage);
    unsigned* ctl = reinterpret_cast<unsigned*>(smem + kOffCtl);
    unsigned* stamp = reinterpret_cast<unsigned*>(smem + kOffStamp);
    if (threadIdx.x < 16) ctl[threadIdx.x] = 0u;
    for (int i = threadIdx.x; i < (kRounds - kWarm) * (kCW + 1); i += kThreads) stamp[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wg = blockIdx.x;
    if (wave == kCW) {          // the loader: 16 KiB fills of this workgroup's 1 / 256 of the source, one in flight, until the consumers are done
        if (!A.stream) return;
        const size_t region = A.w_bytes / kG;
        const unsigned nslots = (unsigned)(region / kSlot);
        for (unsigned fill = 0; fill < 200000u; ++fill) {
            if (lds_ld(ctl + 3) || lds_ld(ctl + 2)) break;
            const char* src = A.w + (size_t)wg * region + (size_t)(fill % nslots) * kSlot + lane * 16;
            char* dst = smem + (fill & (kRing - 1)) * kSlot;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i * 1024),
                                                 (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 2);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        return;
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(A.gran, 0, 4u * kBufGran * 8u, 0x00020000);
    const int line = (wg % kPlanes) * kPlane + (wg / kPlanes) * 16;      // this workgroup's sixteen granules inside a buffer
    const int t0 = 2 * (wave * 64 + lane);
    unsigned bar = 0;
    bool dead = false;
    for (int r = 0; r < kRounds && !dead; ++r) {
        const unsigned tag = A.salt + (unsigned)r + 1u;
        const int b0 = (r & 3) * kBufGran;
        unsigned* const st = r >= kWarm ? stamp + (r - kWarm) * (kCW + 1) : nullptr;
        // ---- publish ----
        const int g0 = wave, g1 = wave + kCW;
        if (MODE == 0) {
            if (lane == 0) put8(rs, b0 + line + g0, tag, val_of(tag, line + g0));
            if (lane == 1) put8(rs, b0 + line + g1, tag, val_of(tag, line + g1));
            if (st && lane == 0) st[wave] = (unsigned)wall_clock64();
        } else if (MODE == 1) {
            if (lane < 2) put8(rs, b0 + line + 2 * wave + lane, tag, val_of(tag, line + 2 * wave + lane));
            if (st && lane == 0) st[wave] = (unsigned)wall_clock64();
        } else if (MODE == 2) {
            if (wave < 4) {
                if (lane < 4) put8(rs, b0 + line + 4 * wave + lane, tag, val_of(tag, line + 4 * wave + lane));
                if (st && lane == 0) st[wave] = (unsigned)wall_clock64();
            }
        } else if (MODE == 5) {
            if (wave == 0) {
                if (lane < 16) put8(rs, b0 + line + lane, tag, val_of(tag, line + lane));
                if (st && lane == 0) st[wave] = (unsigned)wall_clock64();
            }
        } else {                // 3, 4: staged; the wave whose arrival is the eighth of the round stores the line
            if (lane == 0) stage[g0] = val_of(tag, line + g0);
            if (lane == 1) stage[g1] = val_of(tag, line + g1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            unsigned old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(ctl + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old == (unsigned)r * kCW + kCW - 1) {
                if (MODE == 3) {
                    if (lane < 16) put8(rs, b0 + line + lane, tag, stage[lane]);
                } else if (lane < 8) {
                    const float2 v = *reinterpret_cast<const float2*>(stage + 2 * lane);
                    u32x4 g = {__float_as_uint(v.x), tag, __float_as_uint(v.y), tag};
                    __builtin_amdgcn_raw_buffer_store_b128(g, rs, (b0 + line + 2 * lane) * 8, 0, 16);
                }
                if (st && lane == 0) st[wave] = (unsigned)wall_clock64();
            }
        }
        // ---- gather<1, 4>: sentinel = the last plane, then the other three ----
        u32x4 v[kPlanes];
        const int voff = (b0 + t0) * 8;
        unsigned spins = 0;
        while (true) {
            v[kPlanes - 1] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (kPlanes - 1) * kPlane * 8, 16);
            if (__all(v[kPlanes - 1].y == tag && v[kPlanes - 1].w == tag)) break;
            __builtin_amdgcn_s_sleep(3);
            if ((++spins & 63u) == 0u && lds_ld(ctl + 2)) { dead = true; break; }
            if (spins > kSpinLimit) { dead = true; lds_st(ctl + 2, 1u); if (lane == 0) atomicAdd(A.err, 1); break; }
        }
        while (!dead) {
            unsigned bad = 0;
#pragma unroll
            for (int p = 0; p < kPlanes - 1; ++p) v[p] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, p * kPlane * 8, 16);
#pragma unroll
            for (int p = 0; p < kPlanes; ++p) bad |= (v[p].y ^ tag) | (v[p].w ^ tag);
            if (!__any(bad != 0u)) break;
            __builtin_amdgcn_s_sleep(3);
            if ((++spins & 63u) == 0u && lds_ld(ctl + 2)) { dead = true; break; }
            if (spins > kSpinLimit) { dead = true; lds_st(ctl + 2, 1u); if (lane == 0) atomicAdd(A.err, 1); break; }
        }
        if (!dead) {
            int wrong = 0;
#pragma unroll
            for (int p = 0; p < kPlanes; ++p)
                wrong += (__uint_as_float(v[p].x) != val_of(tag, p * kPlane + t0)) + (__uint_as_float(v[p].z) != val_of(tag, p * kPlane + t0 + 1));
            if (wrong) atomicAdd(A.err + 1, wrong);
        }
        // ---- barrier of the consumer waves (LDS counter), then the round is ready ----
        bar += kCW;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        unsigned bs = 0;
        while (!dead && lds_ld(ctl) < bar) {
            if (lds_ld(ctl + 2) || ++bs > 40000000u) { dead = true; lds_st(ctl + 2, 1u); }
        }
        if (st && wave == 0 && lane == 0 && !dead) st[kCW] = (unsigned)wall_clock64();
    }
    if (wave == 0 && lane == 0) lds_st(ctl + 3, 1u);
    // the stamps leave LDS when the rounds are over (eight waves of 64 lanes copy them)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bar += kCW;
    if (lane == 0) __hip_atomic_fetch_add(ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    unsigned bs = 0;
    while (!dead && lds_ld(ctl) < bar) { if (lds_ld(ctl + 2) || ++bs > 40000000u) dead = true; }
    if (dead) return;
    constexpr int nst = (kRounds - kWarm) * (kCW + 1);
    for (int i = wave * 64 + lane; i < nst; i += kCW * 64) A.stamps[(size_t)wg * nst + i] = stamp[i];
}

template <int MODE>
static float launch(const Args& A) {
    CK(hipFuncSetAttribute((const void*)k_line<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_line<MODE>), dim3(kG), dim3(kThreads), kLds, 0, A);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return ms * 1000.f / kRounds;
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 3;
    const size_t wbytes = (size_t)1 << 30;
    char* w;
    CK(hipMalloc(&w, wbytes));
    CK(hipMemset(w, 1, wbytes));
    constexpr int nst = (kRounds - kWarm) * (kCW + 1);
    Args A;
    A.w = w; A.w_bytes = wbytes;
    CK(hipMalloc(&A.gran, (size_t)4 * kBufGran * 8)); CK(hipMemset(A.gran, 0, (size_t)4 * kBufGran * 8));
    CK(hipMalloc(&A.stamps, (size_t)kG * nst * 4));
    CK(hipMalloc(&A.err, 8)); CK(hipMemset(A.err, 0, 8));
    std::vector<unsigned> hs((size_t)kG * nst);
    static const char* names[6] = {"16 x 1 lane x 8 B", "8 x 2 lanes x 8 B", "4 x 4 lanes x 8 B", "1 x 16 lanes x 8 B (staged)", "1 x 8 lanes x 16 B (staged)",
                                   "1 x 16 lanes x 8 B (wave 0)"};
    printf("last store of a round -> last workgroup ready, us over %d rounds (100 MHz clock); us/round from events\n", kRounds - kWarm);
    printf("%-30s %-7s %-4s %8s %8s %8s %10s   %s\n", "line written as", "stream", "rep", "median", "mean", "p90", "us/round", "timeouts wrong");
    unsigned launch_no = 0;
    int failed = 0;
    for (int stream = 0; stream < 2 && !failed; ++stream) {
        for (int rep = -1; rep < reps && !failed; ++rep) {      // rep -1: warm-up of every mode, not printed
            for (int mode = 0; mode < 6 && !failed; ++mode) {
                A.stream = stream;
                A.salt = (++launch_no) << 12;
                CK(hipMemset(A.stamps, 0, (size_t)kG * nst * 4));
                float us = 0.f;
                switch (mode) {
                    case 0: us = launch<0>(A); break;
                    case 1: us = launch<1>(A); break;
                    case 2: us = launch<2>(A); break;
                    case 3: us = launch<3>(A); break;
                    case 4: us = launch<4>(A); break;
                    default: us = launch<5>(A); break;
                }
                int he[2];
                CK(hipMemcpy(he, A.err, 8, hipMemcpyDeviceToHost));
                CK(hipMemcpy(hs.data(), A.stamps, hs.size() * 4, hipMemcpyDeviceToHost));
                if (he[0] || he[1]) failed = 1;
                if (rep < 0 && !failed) continue;
                std::vector<float> dt;
                for (int r = 0; r < kRounds - kWarm; ++r) {
                    // (differences of 32-bit stamps against the round's first store: wrap-safe)
                    const unsigned ref = hs[(size_t)r * (kCW + 1) + 0] ? hs[(size_t)r * (kCW + 1) + 0] : hs[(size_t)r * (kCW + 1) + kCW];
                    int last_store = -(1 << 30), last_ready = -(1 << 30);
                    for (int g = 0; g < kG; ++g) {
                        const unsigned* s = hs.data() + ((size_t)g * (kRounds - kWarm) + r) * (kCW + 1);
                        for (int k = 0; k < kCW; ++k)
                            if (s[k]) last_store = std::max(last_store, (int)(s[k] - ref));
                        if (s[kCW]) last_ready = std::max(last_ready, (int)(s[kCW] - ref));
                    }
                    dt.push_back((last_ready - last_store) * 0.01f);
                }
                std::sort(dt.begin(), dt.end());
                double mean = 0;
                for (float d : dt) mean += d;
                mean /= dt.size();
                printf("%-30s %-7s %-4d %8.2f %8.2f %8.2f %10.2f   %d %d\n", names[mode], stream ? "beside" : "idle", rep, dt[dt.size() / 2], mean,
                       dt[dt.size() * 9 / 10], us, he[0], he[1]);
                fflush(stdout);
            }
        }
    }
    return failed;
}
