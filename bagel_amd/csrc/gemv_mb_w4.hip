// Batched-decode projection on MXFP4 weights: C[M <= 32, N] = epilogue( sa[m] * sum_k Aq[m, k] * E2M1(code[n, k]) * 2^(sb[n, k / 32] - 127) ) as a pure
// WEIGHT STREAM through the block-scaled MFMA -- gemv_mb.hip's form (see its header for why that form wins at 2..32 rows) on the one stored copy of the
// codes and scale bytes that bagel_quantize_rows_mxfp4 writes.  It serves the 5..32 requests bagel_gemv_w4_bf16 refuses (that kernel re-quantises all M rows
// in every workgroup's prologue and keeps M x K bytes of them in LDS).  oracle/mxfp4.py::gemv_w4 states the arithmetic for any row count.
//
//   * Aq / sa are e4m3 rows with one fp32 scale per row, written by a launch of their own (bagel_rmsnorm_fp8 where a norm precedes the projection,
//     bagel_quantize_rows_fp8 otherwise): a row's scale needs the whole row, which no workgroup of a K-partitioned stream sees;
//   * K is counted in 128-deep k-steps (one v_mfma_scale_f32_16x16x128_f8f6f4) and handed out in scale groups of four steps: a lane's scale dword holds the
//     block-scale bytes of its weight row for four steps, and the byte is selected by an immediate of the instruction.  The 8 waves of a workgroup PARTITION
//     the groups (mbw4_wave_steps, host_plan.h); a wave loads the activation fragments of its NS = 4 or 8 steps ONCE (B operand: lane = (request lane % 16,
//     chunk q = lane / 16) holds bytes 16 q .. and 64 + 16 q .. of the step: 8 VGPRs per step and block of 16 requests) and keeps them for every column block;
//   * per column block (16 weight rows) a wave issues NS fragment loads of 1 KB (row lane % 16, 16 bytes = 32 codes at chunk lane / 16: row-major codes ARE
//     the FP4 A-operand layout, mxfp4.hip) + NS / 4 scale dwords, PLAIN loads (mxfp4.hip and gemv_mb.hip both measured non-temporal loads slower on row-major
//     fragments).  A 4-bit fragment is a quarter of a bf16 one, so the stream runs TWO blocks ahead: every register quad is refilled right behind the MFMAs
//     that consumed it with the same fragment of block + 2 -- 2 NS KB per wave in flight for the whole life of the workgroup (8 steps x 2 request blocks:
//     one block ahead, the register file holds no more);
//   * the eight K partials of a block meet in LDS (1 KB per wave, block and request block) and are summed in wave order by one wave, which runs the epilogue
//     with the rounding points of gemv_w4_kernel / gemm.hip: scale by sa[m] first, bf16-round before the residual add, bf16-round g, u and silu(g);
//   * rows longer than 16 scale groups (the down projection: K = 18944 = 148 steps = 37 groups) are cut over KS workgroups as well; those write raw fp32 slabs
//     [KS][16 MB][N] and a small second kernel sums them in slice order and applies the epilogue (SwiGLU16 included) -- no atomics, deterministic.
// Control flow depends on the launch geometry only, never on data: no flags, no waits.  Vector stores only.
#include "common.h"
#include <stdlib.h>
#include <type_traits>

#define EPI_NONE 0
#define EPI_SWIGLU16 3

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

struct MbW4Params {
    const unsigned char* A; long lda;       // e4m3 bytes
    const float* sa;                        // one scale per A row
    const unsigned char* Wq; long ldq;      // codes, bytes per row
    const unsigned char* Ws; long lds;      // permuted scale bytes, bytes per row
    const bf16_t* bias;
    const bf16_t* R; long ldr;
    bf16_t* C; long ldc;
    float* part;      // KS > 1: fp32 slabs [KS][slab_rows][N]
    int M, N, K, epi;
    int gpw, gps;     // scale groups per wave / per slice (mbw4_plan)
    int KS;           // K slices over workgroups (gridDim.y)
    int slab_rows;    // rows of one fp32 slab: 16 x MB
};

template <int I, int N, class F>
__device__ __forceinline__ void mbw4_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        mbw4_for<I + 1, N>(f);
    }
}

// lane owns C[m][n .. n + 3]: activation scale first, then bias, bf16 rounding in front of the residual add
__device__ __forceinline__ void mbw4_epilogue(const MbW4Params& p, f32x4_t a, float sm, int m, int n) {
    float o[4] = {a[0] * sm, a[1] * sm, a[2] * sm, a[3] * sm};
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
__device__ __forceinline__ void mbw4_swiglu(const MbW4Params& p, f32x4_t ag, f32x4_t au, float sm, int m, int oc) {
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float g = bfround(ag[e] * sm);
        const float u = bfround(au[e] * sm);
        o[e] = bfround(silu_f(g)) * u;
    }
    const u32x2_t v = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
    *(u32x2_t*)(p.C + (long)m * p.ldc + oc) = v;
}

// NS: k-steps a wave holds (4 x scale groups per wave).  MB: request blocks of 16 (1: M <= 16, 2: 17..32): every weight fragment feeds MB MFMAs.
// Registers: MB x NS x 8 activation + PF x (NS x 4 weight + NS / 4 scale).  LDS (dynamic): the K partials [CH][8 waves][MB][64 lanes] f32x4 = 32 MB KB.
template <int NS, int MB>
__global__ __launch_bounds__(512) void gemv_mb_w4_kernel(const MbW4Params p) {
    constexpr int CH = 4;                                      // blocks between two reductions (even: a SwiGLU pair never straddles a chunk)
    constexpr int PF = (NS == 8 && MB == 2) ? 1 : 2;           // blocks in flight ahead of the MFMAs (8 steps x 2 request blocks: 128 activation registers leave room for one)
    constexpr int NG = NS / 4;
    extern __shared__ __attribute__((aligned(16))) char mbw4_smem[];
    f32x4_t* part = (f32x4_t*)mbw4_smem;                       // [CH * 8 * MB * 64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const bool swiglu = p.epi == EPI_SWIGLU16;
    const bool fused_swiglu = swiglu && p.KS == 1;             // sliced rows: the slabs hold plain sums, the reduce kernel pairs them
    const int nsteps = p.K >> 7, ngroups = (nsteps + 3) >> 2;
    int s0, ns;
    mbw4_wave_steps(p.gpw, p.gps, nsteps, blockIdx.y, wave, &s0, &ns);
    s0 = __builtin_amdgcn_readfirstlane(s0);
    ns = __builtin_amdgcn_readfirstlane(ns);
    // this workgroup's blocks: units (a block; SwiGLU16: a gate/up pair of blocks) [u0, u1) of the launch's even split over gridDim.x
    const int unit = swiglu ? 2 : 1;
    const int nunits = (p.N >> 4) / unit;
    const int bA = (int)((long)nunits * blockIdx.x / gridDim.x) * unit;
    const int bB = (int)((long)nunits * (blockIdx.x + 1) / gridDim.x) * unit;
    if (bA >= bB) return;                                      // (whole workgroup: no barrier is skipped by a part of it)

    // fragment i = k-step s0 + i (s0 % 4 == 0: fragment i's scale byte is byte i % 4 of dword i / 4).  Steps past the wave's range (a K tail, a slice seam, a wave
    // without work) re-read the row's last step / group -- inside the row -- against activations of 0: they add exactly 0 (pad scale bytes are 2^0).
    int koff[NS], goff[NG];
#pragma unroll
    for (int i = 0; i < NS; ++i) koff[i] = (s0 + i < nsteps ? s0 + i : nsteps - 1);
#pragma unroll
    for (int j = 0; j < NG; ++j) goff[j] = ((s0 >> 2) + j < ngroups ? (s0 >> 2) + j : ngroups - 1) * 16;

    // ---- (1) this wave's activation fragments and row scales, the first two blocks' weight fragments ----
    i32x8_t xf[MB][NS];
    float sm[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = 16 * mb + r < p.M ? 16 * mb + r : p.M - 1;      // requests >= M compute a duplicate that is never stored
        const unsigned char* xa = p.A + (long)m * p.lda + q * 16;
        sm[mb] = p.sa[m];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const u32x4_t x0 = *(const u32x4_t*)(xa + (long)koff[i] * 128);
            const u32x4_t x1 = *(const u32x4_t*)(xa + (long)koff[i] * 128 + 64);
            const bool live = i < ns;
            xf[mb][i] = live ? (i32x8_t){(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]}
                             : (i32x8_t){0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    const unsigned char* wrow = p.Wq + (long)r * p.ldq + q * 16;       // + block * 16 rows
    const unsigned char* srow = p.Ws + (long)r * p.lds + q * 4;
    const long wblk = 16 * p.ldq, sblk = 16 * p.lds;
    u32x4_t wf[PF][NS];
    unsigned sc[PF][NG];
    auto load_block = [&](auto SLOT, int b) {
        constexpr int slot = decltype(SLOT)::value;
        const unsigned char* wb = wrow + (long)b * wblk;
        const unsigned char* sb = srow + (long)b * sblk;
#pragma unroll
        for (int i = 0; i < NS; ++i) wf[slot][i] = *(const u32x4_t*)(wb + (long)koff[i] * 64);
#pragma unroll
        for (int j = 0; j < NG; ++j) sc[slot][j] = *(const unsigned*)(sb + goff[j]);
    };
    if (ns > 0) {
        load_block(std::integral_constant<int, 0>{}, bA);
        if constexpr (PF > 1) load_block(std::integral_constant<int, PF - 1>{}, bA + 1 < bB ? bA + 1 : bB - 1);
    }

    // ---- (2) the stream.  Per block NS x MB MFMAs; block b lives in register set (b - bA) % PF and every quad of it is refilled in place, right behind the MFMAs
    //      that consumed it, with the same fragment of block b + PF (across chunk seams too: the stream never stops for a reduction).  Every CH blocks the eight K
    //      partials meet in LDS: wave j sums output j (a block; fused SwiGLU16: gate block 2 j + up block 2 j + 1) and finishes it. ----
    for (int c0 = bA; c0 < bB; c0 += CH) {
        const int cb = bB - c0 < CH ? bB - c0 : CH;             // blocks of this chunk
        mbw4_for<0, CH>([&](auto GI) {
            constexpr int g = decltype(GI)::value, slot = g % PF;      // (c0 - bA) % CH == 0 and CH % PF == 0
            if (g >= cb) return;
            f32x4_t acc[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) acc[mb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            if (ns > 0) {
                const int bn = c0 + g + PF;                    // the block to prefetch into this register set
                const bool more = bn < bB;
                const unsigned char* wn = wrow + (long)(more ? bn : bB - 1) * wblk;
                const unsigned char* sn = srow + (long)(more ? bn : bB - 1) * sblk;
                unsigned scur[NG];
#pragma unroll
                for (int j = 0; j < NG; ++j) scur[j] = sc[slot][j];
                if (more) {
#pragma unroll
                    for (int j = 0; j < NG; ++j) sc[slot][j] = *(const unsigned*)(sn + goff[j]);
                }
                mbw4_for<0, NS>([&](auto II) {
                    constexpr int i = decltype(II)::value;
                    const i32x8_t wa = {(int)wf[slot][i][0], (int)wf[slot][i][1], (int)wf[slot][i][2], (int)wf[slot][i][3], 0, 0, 0, 0};
                    // A = weights (FP4: cbsz 4, block scale = byte i % 4 of the group's dword), B = activations (e4m3: blgp 0, scale 2^0)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
                        acc[mb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa, xf[mb][i], acc[mb], 4, 0, i & 3, (int)scur[i >> 2], 0, 127);
                    if (more) wf[slot][i] = *(const u32x4_t*)(wn + (long)koff[i] * 64);
                });
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) part[((g * 8 + wave) * MB + mb) * 64 + lane] = acc[mb];
        });
        __syncthreads();
        const int nout = fused_swiglu ? cb >> 1 : cb;
        // (output j, request block mb) pairs dealt over the 8 waves
        for (int t = wave; t < nout * MB; t += 8) {
            const int j = t % nout, mb = t / nout;
            const int m = 16 * mb + r;
            float smv = sm[0];
#pragma unroll
            for (int k = 1; k < MB; ++k) smv = mb == k ? sm[k] : smv;
            if (fused_swiglu) {
                f32x4_t ag = part[(((2 * j) * 8) * MB + mb) * 64 + lane], au = part[(((2 * j + 1) * 8) * MB + mb) * 64 + lane];
#pragma unroll
                for (int w = 1; w < 8; ++w) {
                    ag = ag + part[(((2 * j) * 8 + w) * MB + mb) * 64 + lane];
                    au = au + part[(((2 * j + 1) * 8 + w) * MB + mb) * 64 + lane];
                }
                if (m < p.M) mbw4_swiglu(p, ag, au, smv, m, ((c0 >> 1) + j) * 16 + q * 4);
            } else {
                f32x4_t a = part[((j * 8) * MB + mb) * 64 + lane];
#pragma unroll
                for (int w = 1; w < 8; ++w) a = a + part[((j * 8 + w) * MB + mb) * 64 + lane];
                const int n = (c0 + j) * 16 + q * 4;
                if (p.KS > 1) *(f32x4_t*)(p.part + ((long)blockIdx.y * (16 * MB) + m) * p.N + n) = a;      // all 16 x MB rows: the slab has them
                else if (m < p.M) mbw4_epilogue(p, a, smv, m, n);
            }
        }
        if (c0 + CH < bB) __syncthreads();                     // the partials are consumed before the next chunk overwrites them
    }
}

// KS > 1: C = epilogue(sa[m] * sum over the K slices, in slice order)
__global__ __launch_bounds__(256) void gemv_mb_w4_reduce_kernel(const MbW4Params p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const bool swiglu = p.epi == EPI_SWIGLU16;
    const int nq = (swiglu ? p.N >> 1 : p.N) >> 2;
    if (idx >= p.M * nq) return;
    const int m = idx / nq, oc = (idx - m * nq) * 4;
    const float sm = p.sa[m];
    if (swiglu) {
        const int ng = (oc >> 4) * 32 + (oc & 15);             // gate column; up = + 16
        f32x4_t ag = *(const f32x4_t*)(p.part + (long)m * p.N + ng), au = *(const f32x4_t*)(p.part + (long)m * p.N + ng + 16);
        for (int s = 1; s < p.KS; ++s) {
            ag = ag + *(const f32x4_t*)(p.part + ((long)s * p.slab_rows + m) * p.N + ng);
            au = au + *(const f32x4_t*)(p.part + ((long)s * p.slab_rows + m) * p.N + ng + 16);
        }
        mbw4_swiglu(p, ag, au, sm, m, oc);
    } else {
        f32x4_t a = *(const f32x4_t*)(p.part + (long)m * p.N + oc);
        for (int s = 1; s < p.KS; ++s) a = a + *(const f32x4_t*)(p.part + ((long)s * p.slab_rows + m) * p.N + oc);
        mbw4_epilogue(p, a, sm, m, oc);
    }
}

// Geometry (slices, groups per wave, grid): mbw4_plan in host_plan.cpp.  BAGEL_MB_W4_WGS overrides the workgroup count (tuning / tests).
static int mbw4_wgs() {
    static int wgs_env = -1;
    if (wgs_env < 0) {
        const char* e = getenv("BAGEL_MB_W4_WGS");
        wgs_env = (e && atoi(e) > 0) ? atoi(e) : 0;
    }
    if (wgs_env) return wgs_env;
    int cus = 0;
    return bagel_device_cus(&cus) == BAGEL_OK ? cus : 256;
}

template <int NS, int MB>
static int mbw4_launch(const MbW4Params& p, dim3 grid, hipStream_t stream) {
    constexpr int smem = 4 * 8 * MB * 1024;                    // the K partials of a chunk
    if constexpr (smem > 48 * 1024) {
        if (int rc = bagel_enable_lds((const void*)gemv_mb_w4_kernel<NS, MB>, smem, "gemv_mb_w4_kernel")) return rc;
    }
    hipLaunchKernelGGL((gemv_mb_w4_kernel<NS, MB>), grid, dim3(512), smem, stream, p);
    return bagel_check_launch("gemv_mb_w4_kernel");
}

extern "C" int bagel_gemv_mb_w4_bf16(const void* Aq, int64_t lda_bytes, const float* sa, const void* Wq, int64_t ldq_bytes, const void* Ws,
                                     int64_t lds_bytes, const void* bias, const void* R, int64_t ldr, void* C, int64_t ldc, int32_t M, int32_t N,
                                     int32_t K, int32_t epilogue, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
    BAGEL_REQUIRE(Aq && sa && Wq && Ws && C, "gemv_mb_w4: null pointer");
    MbW4Geometry g;                                                 // shape checks, slices, groups per wave and grid: host_plan.cpp
    if (int rc = mbw4_plan(M, N, K, epilogue, mbw4_wgs(), &g)) return rc;
    BAGEL_REQUIRE(epilogue != EPI_SWIGLU16 || (!bias && !R), "gemv_mb_w4: SwiGLU16 takes no bias / residual");
    BAGEL_REQUIRE(lda_bytes >= K && (lda_bytes % 16) == 0 && ldq_bytes >= K / 2 && (ldq_bytes % 16) == 0, "gemv_mb_w4: lda/ldq must cover a row and keep it 16-byte aligned");
    BAGEL_REQUIRE(lds_bytes >= ((K / 128 + 3) / 4) * 16 && (lds_bytes % 4) == 0, "gemv_mb_w4: lds_bytes too small");
    BAGEL_REQUIRE((ldc % 4) == 0 && (ldr % 4) == 0, "gemv_mb_w4: ldc/ldr must be multiples of 4");
    BAGEL_REQUIRE((((uintptr_t)Aq | (uintptr_t)Wq) & 15) == 0 && (((uintptr_t)Ws | (uintptr_t)sa) & 3) == 0 &&
                  (((uintptr_t)C | (uintptr_t)R | (uintptr_t)bias) & 7) == 0, "gemv_mb_w4: alignment");
    MbW4Params p;
    p.A = (const unsigned char*)Aq; p.lda = lda_bytes; p.sa = sa;
    p.Wq = (const unsigned char*)Wq; p.ldq = ldq_bytes; p.Ws = (const unsigned char*)Ws; p.lds = lds_bytes;
    p.bias = (const bf16_t*)bias; p.R = (const bf16_t*)R; p.ldr = ldr; p.C = (bf16_t*)C; p.ldc = ldc;
    p.M = M; p.N = N; p.K = K; p.epi = epilogue;
    p.gpw = g.gpw; p.gps = g.gps; p.KS = g.KS; p.slab_rows = 16 * g.MB;
    if (p.KS > 1)
        BAGEL_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= (int64_t)p.KS * p.slab_rows * N * 4,
                      "gemv_mb_w4: K=%d runs as %d slices and needs a 16-byte aligned fp32 workspace of %lld bytes (bagel_gemv_mb_w4_workspace_bytes)", K, p.KS,
                      (long long)p.KS * p.slab_rows * N * 4);
    p.part = (float*)workspace;
    const dim3 grid(g.gx, p.KS);
    if (int rc = g.NS == 4 ? (g.MB == 1 ? mbw4_launch<4, 1>(p, grid, stream) : mbw4_launch<4, 2>(p, grid, stream))
                           : (g.MB == 1 ? mbw4_launch<8, 1>(p, grid, stream) : mbw4_launch<8, 2>(p, grid, stream))) return rc;
    if (p.KS > 1) {
        const long nq = (epilogue == EPI_SWIGLU16 ? N / 2 : N) / 4;
        hipLaunchKernelGGL(gemv_mb_w4_reduce_kernel, dim3(ceil_div((long)M * nq, 256)), dim3(256), 0, stream, p);
        return bagel_check_launch("gemv_mb_w4_reduce_kernel");
    }
    return BAGEL_OK;
}
