// Batched-decode projection on NF4 weights: C[M <= 32, N] = epilogue( A[M, K] . bf16(NF4_CODE[code[n, k]] * absmax[n, k / 64])^T ) as a pure WEIGHT STREAM
// through the bf16 MFMA -- gemv_mb.hip's form (see its header for why that form wins at 2..32 rows) on the one stored copy of the codes and absmax values that
// bagel_quantize_nf4 writes.  It serves the 5..32 requests bagel_gemv_nf4_bf16 (quant.hip) reads the codes four rows at a time for.
//
// ARITHMETIC.  The weight is rounded to bf16 exactly ONCE, after the fp32 multiply NF4_CODE[code] * absmax (pack2bf: hardware RNE) -- bit-equal to
// bagel_dequantize_nf4_bf16 and oracle/nf4.py::dequantize_nf4, what bitsandbytes multiplies with for more than one activation row and what the NF4 load mode's
// prefill / denoise GEMMs see; oracle/nf4.py::linear_nf4 states it.  The product accumulates in fp32 on mfma_f32_16x16x32_bf16.  The batch-<=4 kernel
// gemv_nf4_kernel keeps its fp32 weight, so the two routes differ by one bf16 rounding per weight (relative 2^-9, random sign).
//
//   * K is counted in k-groups of 128 weights = 64 code bytes per weight row.  Lane (r = lane % 16, q = lane / 16) loads the 16 bytes holding weights
//     128 g + 32 q .. + 32 of row 16 block + r (one global_load_dwordx4: half an absmax block, so ONE fp32 absmax per lane and group, index 2 g + q / 2) and
//     de-quantises them in registers into the A fragments of FOUR MFMAs: MFMA j takes weights 128 g + 32 q + 8 j .. + 8 = dword j of the load, the even element
//     of a byte in its high nibble.  The B operand (activations) uses the same k bijection: lane (r, q), MFMA j holds x[m = r][128 g + 32 q + 8 j .. + 8];
//   * the lookup: the 16-float code book in LDS (64 lanes hit 16 different banks, equal indices broadcast: conflict-free), 4 * code extracted per byte with two
//     mask operations per dword and one v_bfe per weight, one ds_read_b32, one v_mul_f32 and half a v_cvt_pk_bf16_f32 per weight -- paid once for all M rows;
//   * the 8 waves of a workgroup PARTITION the groups (mbnf4_wave_groups, host_plan.h); a wave loads the activation fragments of its GP = 1, 2 or 4 groups ONCE
//     (16 VGPRs per group and block of 16 requests) and keeps them for every column block; the code chunks of the next blocks are in flight while one is de-quantised;
//   * groups past a wave's range (a slice seam, a wave without work, gpw = 3 on the GP = 4 instantiation) are SKIPPED on a wave-uniform count: nothing is
//     loaded or multiplied for them, so they add exactly nothing whatever the bits of a neighbouring weight;
//   * the eight K partials of a block meet in LDS (1 KB per wave, block and request block) and are summed in wave order by one wave, which runs the epilogue
//     with gemv_mb.hip's rounding points: bias, bf16-round before the residual add, bf16-round g, u and silu(g);
//   * rows longer than 32 groups (the down projection: K = 18944 = 148 groups) are cut over KS workgroups as well; those write raw fp32 slabs [KS][16 MB][N]
//     and a small second kernel sums them in slice order and applies the epilogue (SwiGLU16 included) -- no atomics, deterministic.
// No fused RMSNorm: the session runs bagel_rmsnorm in front (the registers belong to the de-quantiser, and 3 x 2 instantiations stay 3 x 2).
// Control flow depends on the launch geometry only, never on data: no flags, no waits.  Vector stores only.
#include "common.h"
#include <stdlib.h>
#include <type_traits>

#define EPI_NONE 0
#define EPI_SWIGLU16 3

// the bitsandbytes NF4 code book (quant.hip, oracle/nf4.py)
__constant__ float MBNF4_CODE_DEV[16] = {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f,
                                         -0.18477343022823334f, -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f,
                                         0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f,
                                         0.7229568362236023f, 1.0f};

struct MbNf4Params {
    const bf16_t* A; long lda;
    const unsigned char* Wq; long ldq;      // codes, bytes per row
    const float* absmax;                    // [N, K / 64]
    const bf16_t* bias;
    const bf16_t* R; long ldr;
    bf16_t* C; long ldc;
    float* part;      // KS > 1: fp32 slabs [KS][slab_rows][N]
    int M, N, K, epi;
    int gpw, gps;     // k-groups per wave / per slice (mbnf4_plan)
    int KS;           // K slices over workgroups (gridDim.y)
    int slab_rows;    // rows of one fp32 slab: 16 x MB
};

template <int I, int N, class F>
__device__ __forceinline__ void mbnf4_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        mbnf4_for<I + 1, N>(f);
    }
}

// lane owns C[m][n .. n + 3]: bias, then bf16 rounding in front of the residual add (mb_epilogue of gemv_mb.hip without the activations)
__device__ __forceinline__ void mbnf4_epilogue(const MbNf4Params& p, f32x4_t a, int m, int n) {
    float o[4] = {a[0], a[1], a[2], a[3]};
    if (p.bias) {
        const u32x2_t bv = *(const u32x2_t*)(p.bias + n);
        o[0] += lo2f(bv[0]); o[1] += hi2f(bv[0]); o[2] += lo2f(bv[1]); o[3] += hi2f(bv[1]);
    }
    if (p.R) {
        const u32x2_t rv = *(const u32x2_t*)(p.R + (long)m * p.ldr + n);
        o[0] = bfround(o[0]) + lo2f(rv[0]); o[1] = bfround(o[1]) + hi2f(rv[0]);
        o[2] = bfround(o[2]) + lo2f(rv[1]); o[3] = bfround(o[3]) + hi2f(rv[1]);
    }
    const u32x2_t v = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
    *(u32x2_t*)(p.C + (long)m * p.ldc + n) = v;
}
// lane owns outputs oc .. oc + 3 of the gate/up pair: g, u and silu(g) are bf16 values
__device__ __forceinline__ void mbnf4_swiglu(const MbNf4Params& p, f32x4_t ag, f32x4_t au, int m, int oc) {
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = bfround(silu_f(bfround(ag[e]))) * bfround(au[e]);
    const u32x2_t v = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
    *(u32x2_t*)(p.C + (long)m * p.ldc + oc) = v;
}

// GP: k-groups a wave holds.  MB: request blocks of 16 (1: M <= 16, 2: 17..32): every de-quantised fragment feeds MB MFMAs.
// Registers: MB x GP x 16 activation + PF x GP x (4 code + 1 absmax) + 4 of the fragment being built.  LDS: the K partials [CH][8 waves][MB][64 lanes] f32x4 =
// 32 MB KB (dynamic) + the 64-byte code book.
template <int GP, int MB>
__global__ __launch_bounds__(512) void gemv_mb_nf4_kernel(const MbNf4Params p) {
    constexpr int CH = 4;                                      // blocks between two reductions (even: a SwiGLU pair never straddles a chunk)
    constexpr int PF = (GP == 4 && MB == 2) ? 1 : 2;           // blocks in flight ahead of the de-quantiser (4 groups x 2 request blocks: 128 activation registers)
    extern __shared__ __attribute__((aligned(16))) char mbnf4_smem[];
    __shared__ __attribute__((aligned(64))) float lut[16];
    f32x4_t* part = (f32x4_t*)mbnf4_smem;                      // [CH * 8 * MB * 64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const bool swiglu = p.epi == EPI_SWIGLU16;
    const bool fused_swiglu = swiglu && p.KS == 1;             // sliced rows: the slabs hold plain sums, the reduce kernel pairs them
    const int G = p.K >> 7, nb = p.K >> 6;
    int g0, ng;
    mbnf4_wave_groups(p.gpw, p.gps, G, blockIdx.y, wave, &g0, &ng);
    g0 = __builtin_amdgcn_readfirstlane(g0);
    ng = __builtin_amdgcn_readfirstlane(ng);                   // <= GP (the host picks GP >= gpw)
    // this workgroup's blocks: units (a block; SwiGLU16: a gate/up pair of blocks) [u0, u1) of the launch's even split over gridDim.x
    const int unit = swiglu ? 2 : 1;
    const int nunits = (p.N >> 4) / unit;
    const int bA = (int)((long)nunits * blockIdx.x / gridDim.x) * unit;
    const int bB = (int)((long)nunits * (blockIdx.x + 1) / gridDim.x) * unit;
    if (bA >= bB) return;                                      // (whole workgroup: no barrier is skipped by a part of it)
    if (tid < 16) lut[tid] = MBNF4_CODE_DEV[tid];

    // ---- (1) this wave's activation fragments (group i = k-group g0 + i, live while i < ng) and the first blocks' code chunks ----
    bf16x8_t xf[MB][GP][4];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = 16 * mb + r < p.M ? 16 * mb + r : p.M - 1;      // requests >= M compute a duplicate that is never stored
        const bf16_t* xa = p.A + (long)m * p.lda + (long)g0 * 128 + q * 32;
#pragma unroll
        for (int i = 0; i < GP; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                xf[mb][i][j] = i < ng ? *(const bf16x8_t*)(xa + i * 128 + j * 8) : (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
    }
    const unsigned char* wrow = p.Wq + (long)r * p.ldq + (long)g0 * 64 + q * 16;      // + block * 16 rows
    const float* arow = p.absmax + (long)r * nb + 2 * g0 + (q >> 1);
    const long wblk = 16 * p.ldq, ablk = 16L * nb;
    u32x4_t wf[PF][GP];
    float am[PF][GP];
    auto load_block = [&](auto SLOT, int b) {
        constexpr int slot = decltype(SLOT)::value;
        const unsigned char* wb = wrow + (long)b * wblk;
        const float* ab = arow + (long)b * ablk;
#pragma unroll
        for (int i = 0; i < GP; ++i)
            if (i < ng) {
                wf[slot][i] = *(const u32x4_t*)(wb + i * 64);
                am[slot][i] = ab[2 * i];
            }
    };
    load_block(std::integral_constant<int, 0>{}, bA);
    if constexpr (PF > 1) load_block(std::integral_constant<int, PF - 1>{}, bA + 1 < bB ? bA + 1 : bB - 1);
    __syncthreads();                                           // the code book is in LDS
    const char* lutb = (const char*)lut;

    // ---- (2) the stream.  Per block and live group: 32 lookups -> 4 A fragments -> 4 x MB MFMAs; block b lives in register set (b - bA) % PF and every chunk of it is
    //      refilled right after it was copied out with the same group of block b + PF (across chunk seams too: the stream never stops for a reduction).  Every
    //      CH blocks the eight K partials meet in LDS: wave j sums output j (a block; fused SwiGLU16: gate block 2 j + up block 2 j + 1) and finishes it. ----
    for (int c0 = bA; c0 < bB; c0 += CH) {
        const int cb = bB - c0 < CH ? bB - c0 : CH;             // blocks of this chunk
        mbnf4_for<0, CH>([&](auto GI) {
            constexpr int g = decltype(GI)::value, slot = g % PF;      // (c0 - bA) % CH == 0 and CH % PF == 0
            if (g >= cb) return;
            f32x4_t acc[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) acc[mb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            const int bn = c0 + g + PF;                        // the block to prefetch into this register set
            const bool more = bn < bB;
            const unsigned char* wn = wrow + (long)(more ? bn : bB - 1) * wblk;
            const float* an = arow + (long)(more ? bn : bB - 1) * ablk;
            mbnf4_for<0, GP>([&](auto II) {
                constexpr int i = decltype(II)::value;
                if (i >= ng) return;                           // wave-uniform: a group outside this wave's range adds exactly nothing
                const u32x4_t w = wf[slot][i];
                const float a = am[slot][i];
                if (more) {
                    wf[slot][i] = *(const u32x4_t*)(wn + i * 64);
                    am[slot][i] = an[2 * i];
                }
                // all 32 lookups of the group are issued before the first product waits for one: at two waves per SIMD nothing else hides the LDS latency
                float ce[4][4], co[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {                  // dword j = weights 8 j .. 8 j + 7 of the lane's 32
                    unsigned ev = (w[j] >> 2) & 0x3C3C3C3Cu, od = (w[j] << 2) & 0x3C3C3C3Cu;             // 4 * code of the even / odd elements, one per byte
                    // (opaque to the optimiser: it otherwise folds the masks into a shift + and PER WEIGHT, 16 operations per dword where 4 + 8 byte extracts do)
                    asm volatile("" : "+v"(ev), "+v"(od));
#pragma unroll
                    for (int b = 0; b < 4; ++b) {              // byte b = elements 8 j + 2 b (high nibble) and 8 j + 2 b + 1 (low nibble)
                        ce[j][b] = *(const float*)(lutb + ((ev >> (8 * b)) & 0xFFu));
                        co[j][b] = *(const float*)(lutb + ((od >> (8 * b)) & 0xFFu));
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    u32x4_t d;
#pragma unroll
                    for (int b = 0; b < 4; ++b) d[b] = pack2bf(ce[j][b] * a, co[j][b] * a);      // the ONE rounding of the weight: bf16(code * absmax), as bagel_dequantize_nf4_bf16
                    const bf16x8_t wa = __builtin_bit_cast(bf16x8_t, d);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, xf[mb][i][j], acc[mb], 0, 0, 0);
                }
            });
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) part[((g * 8 + wave) * MB + mb) * 64 + lane] = acc[mb];
        });
        __syncthreads();
        const int nout = fused_swiglu ? cb >> 1 : cb;
        // (output j, request block mb) pairs dealt over the 8 waves
        for (int t = wave; t < nout * MB; t += 8) {
            const int j = t % nout, mb = t / nout;
            const int m = 16 * mb + r;
            if (fused_swiglu) {
                f32x4_t ag = part[(((2 * j) * 8) * MB + mb) * 64 + lane], au = part[(((2 * j + 1) * 8) * MB + mb) * 64 + lane];
#pragma unroll
                for (int w = 1; w < 8; ++w) {
                    ag = ag + part[(((2 * j) * 8 + w) * MB + mb) * 64 + lane];
                    au = au + part[(((2 * j + 1) * 8 + w) * MB + mb) * 64 + lane];
                }
                if (m < p.M) mbnf4_swiglu(p, ag, au, m, ((c0 >> 1) + j) * 16 + q * 4);
            } else {
                f32x4_t a = part[((j * 8) * MB + mb) * 64 + lane];
#pragma unroll
                for (int w = 1; w < 8; ++w) a = a + part[((j * 8 + w) * MB + mb) * 64 + lane];
                const int n = (c0 + j) * 16 + q * 4;
                if (p.KS > 1) *(f32x4_t*)(p.part + ((long)blockIdx.y * (16 * MB) + m) * p.N + n) = a;      // all 16 x MB rows: the slab has them
                else if (m < p.M) mbnf4_epilogue(p, a, m, n);
            }
        }
        if (c0 + CH < bB) __syncthreads();                     // the partials are consumed before the next chunk overwrites them
    }
}

// KS > 1: C = epilogue(sum over the K slices, in slice order)
__global__ __launch_bounds__(256) void gemv_mb_nf4_reduce_kernel(const MbNf4Params p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const bool swiglu = p.epi == EPI_SWIGLU16;
    const int nq = (swiglu ? p.N >> 1 : p.N) >> 2;
    if (idx >= p.M * nq) return;
    const int m = idx / nq, oc = (idx - m * nq) * 4;
    if (swiglu) {
        const int ng = (oc >> 4) * 32 + (oc & 15);             // gate column; up = + 16
        f32x4_t ag = *(const f32x4_t*)(p.part + (long)m * p.N + ng), au = *(const f32x4_t*)(p.part + (long)m * p.N + ng + 16);
        for (int s = 1; s < p.KS; ++s) {
            ag = ag + *(const f32x4_t*)(p.part + ((long)s * p.slab_rows + m) * p.N + ng);
            au = au + *(const f32x4_t*)(p.part + ((long)s * p.slab_rows + m) * p.N + ng + 16);
        }
        mbnf4_swiglu(p, ag, au, m, oc);
    } else {
        f32x4_t a = *(const f32x4_t*)(p.part + (long)m * p.N + oc);
        for (int s = 1; s < p.KS; ++s) a = a + *(const f32x4_t*)(p.part + ((long)s * p.slab_rows + m) * p.N + oc);
        mbnf4_epilogue(p, a, m, oc);
    }
}

// Geometry (slices, groups per wave, grid): mbnf4_plan in host_plan.cpp.  BAGEL_MB_NF4_WGS overrides the workgroup count (tuning / tests).
static int mbnf4_wgs() {
    static int wgs_env = -1;
    if (wgs_env < 0) {
        const char* e = getenv("BAGEL_MB_NF4_WGS");
        wgs_env = (e && atoi(e) > 0) ? atoi(e) : 0;
    }
    if (wgs_env) return wgs_env;
    int cus = 0;
    return bagel_device_cus(&cus) == BAGEL_OK ? cus : 256;
}

template <int GP, int MB>
static int mbnf4_launch(const MbNf4Params& p, dim3 grid, hipStream_t stream) {
    constexpr int smem = 4 * 8 * MB * 1024;                    // the K partials of a chunk
    if constexpr (smem > 48 * 1024) {
        if (int rc = bagel_enable_lds((const void*)gemv_mb_nf4_kernel<GP, MB>, smem, "gemv_mb_nf4_kernel")) return rc;
    }
    hipLaunchKernelGGL((gemv_mb_nf4_kernel<GP, MB>), grid, dim3(512), smem, stream, p);
    return bagel_check_launch("gemv_mb_nf4_kernel");
}

extern "C" int bagel_gemv_mb_nf4_bf16(const void* A, int64_t lda, const void* Wq, int64_t ldq_bytes, const float* absmax, const void* bias, const void* R,
                                      int64_t ldr, void* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* workspace,
                                      int64_t workspace_bytes, hipStream_t stream) {
    BAGEL_REQUIRE(A && Wq && absmax && C, "gemv_mb_nf4: null pointer");
    MbNf4Geometry g;                                                // shape checks, slices, groups per wave and grid: host_plan.cpp
    if (int rc = mbnf4_plan(M, N, K, epilogue, mbnf4_wgs(), &g)) return rc;
    BAGEL_REQUIRE(epilogue != EPI_SWIGLU16 || (!bias && !R), "gemv_mb_nf4: SwiGLU16 takes no bias / residual");
    BAGEL_REQUIRE(lda >= K && (lda % 8) == 0 && ldq_bytes >= K / 2 && (ldq_bytes % 16) == 0, "gemv_mb_nf4: lda/ldq must cover a row and keep it 16-byte aligned");
    BAGEL_REQUIRE((ldc % 4) == 0 && (ldr % 4) == 0, "gemv_mb_nf4: ldc/ldr must be multiples of 4");
    BAGEL_REQUIRE((((uintptr_t)A | (uintptr_t)Wq) & 15) == 0 && ((uintptr_t)absmax & 3) == 0 &&
                  (((uintptr_t)C | (uintptr_t)R | (uintptr_t)bias) & 7) == 0, "gemv_mb_nf4: alignment");
    MbNf4Params p;
    p.A = (const bf16_t*)A; p.lda = lda;
    p.Wq = (const unsigned char*)Wq; p.ldq = ldq_bytes; p.absmax = absmax;
    p.bias = (const bf16_t*)bias; p.R = (const bf16_t*)R; p.ldr = ldr; p.C = (bf16_t*)C; p.ldc = ldc;
    p.M = M; p.N = N; p.K = K; p.epi = epilogue;
    p.gpw = g.gpw; p.gps = g.gps; p.KS = g.KS; p.slab_rows = 16 * g.MB;
    if (p.KS > 1)
        BAGEL_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= (int64_t)p.KS * p.slab_rows * N * 4,
                      "gemv_mb_nf4: workspace: K=%d runs as %d slices and needs 16-byte aligned fp32 room of %lld bytes (bagel_gemv_mb_nf4_workspace_bytes)", K,
                      p.KS, (long long)p.KS * p.slab_rows * N * 4);
    p.part = (float*)workspace;
    const dim3 grid(g.gx, p.KS);
    int rc;
    if (g.MB == 1) rc = g.GP == 1 ? mbnf4_launch<1, 1>(p, grid, stream) : (g.GP == 2 ? mbnf4_launch<2, 1>(p, grid, stream) : mbnf4_launch<4, 1>(p, grid, stream));
    else rc = g.GP == 1 ? mbnf4_launch<1, 2>(p, grid, stream) : (g.GP == 2 ? mbnf4_launch<2, 2>(p, grid, stream) : mbnf4_launch<4, 2>(p, grid, stream));
    if (rc) return rc;
    if (p.KS > 1) {
        const long nq = (epilogue == EPI_SWIGLU16 ? N / 2 : N) / 4;
        hipLaunchKernelGGL(gemv_mb_nf4_reduce_kernel, dim3(ceil_div((long)M * nq, 256)), dim3(256), 0, stream, p);
        return bagel_check_launch("gemv_mb_nf4_reduce_kernel");
    }
    return BAGEL_OK;
}
