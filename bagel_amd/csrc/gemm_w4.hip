// Large-M GEMM on MXFP4 weights: the whole-model load mode weight_store = "mxfp4" (the large-M sibling of mxfp4.hip's decode kernel; both read
// ONE stored copy of the codes and scale bytes that bagel_quantize_rows_mxfp4 writes).  oracle/mxfp4.py states the arithmetic:
//
//   C[c_rows[i], :] = epilogue( sa[a_rows[i]] * sum_k Aq[a_rows[i], k] * (E2M1(code[n, k]) * 2^(sb[n, k/32] - 127)) )
//
// Aq = e4m3 bytes with one fp32 scale per row (bagel_quantize_rows_fp8 / bagel_rmsnorm_fp8), the product on
// v_mfma_scale_f32_16x16x128_f8f6f4 with the weights as the FP4 operand and their E8M0 bytes as its block scale: the de-quantisation IS the
// MFMA, there is no bf16 image of W anywhere.
//
// Structure (gemm_tn_kernel of gemm.hip with a 4-bit W image): 128 x 256 x 128 tile, 2 x 2 waves of 64 x 128, two LDS stages filled by
// 16-byte LDS-DMA, counted vmcnt so the next tile's DMA stays in flight across the barrier.  Per 128-deep k-tile an A row is 128 bytes
// (8 chunks, source-side XOR swizzle by (row / 2) % 8 as in the bf16 kernel) and a W row is 64 bytes (4 chunks: one DMA instruction covers
// 16 rows; swizzle by (row / 4) % 4, which spreads the 16 rows of a fragment read over all 64 banks).  Operand layouts as probed for
// gemv_w4_kernel: an FP4 lane (row, q) holds elements 32q .. 32q+31 = chunk q of the W row; an e4m3 lane holds 16q .. 16q+15 and
// 64+16q .. 64+16q+15 = chunks q and q + 4 of the A row.  The scale bytes never enter LDS: a lane keeps one dword per weight fragment
// (its four next k-tiles, the device order of permute_scales) and fetches the next group's dwords one group ahead.
// Swapped operands (D = Wfrag x Afrag): a lane owns 4 consecutive n of one output row -> 8-byte stores, in-register SwiGLU pairing.
#include "common.h"
#include <stdlib.h>
#include <type_traits>

#define EPI_NONE 0
#define EPI_SWIGLU16 3

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

struct GemmW4Params {
    const unsigned char* A; long lda;       // e4m3 bytes
    const float* sa;                        // per physical A row
    const unsigned char* Wq; long ldq;      // codes, bytes per row
    const unsigned char* Ws; long lds;      // permuted scale bytes, bytes per row
    const bf16_t* bias;
    const int* a_rows;
    const int* c_rows;
    const bf16_t* R; long ldr;
    bf16_t* C; long ldc;
    int M, N, K, epi;
    int tiles_m, tiles_n;
};

// 16 bytes per lane global -> LDS (destination = wave-uniform base + 16 * lane).  Inline asm: hipcc does not see the LDS write, so it
// puts no vmcnt(0) in front of the fragment reads; completion is enforced by the counted waits of the k loop.
__device__ __forceinline__ void w4g_glds16(const void* gsrc, unsigned lds_dst_uniform) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst_uniform)
                 : "memory");
}

template <int BM, int BN, int WM, int WN, int OCC, bool SWIGLU>
__global__ __launch_bounds__(WM* WN * 64) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void gemm_w4_kernel(const GemmW4Params p) {
    constexpr int NW = WM * WN;
    constexpr int MB = BM / WM / 16;   // 16-row activation fragments per wave
    constexpr int NB = BN / WN / 16;   // 16-row weight fragments per wave
    constexpr int A_BYTES = BM * 128;
    constexpr int B_BYTES = BN * 64;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int LA = BM / 8 / NW;    // DMA instructions per wave: 8 A rows each
    constexpr int LB = BN / 16 / NW;   //                           16 W rows each
    static_assert(BM % (8 * NW) == 0 && BN % (16 * NW) == 0 && (NB % 2) == 0, "tile/wave mismatch");

    extern __shared__ __attribute__((aligned(16))) char w4g_smem[];
    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(const __attribute__((address_space(3))) char*)w4g_smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // ---- XCD-aware tile mapping (bijective for any grid size), bands of 4 M tiles ----
    const int nblk = p.tiles_m * p.tiles_n;
    int bid = blockIdx.x;
    {
        const int q8 = nblk >> 3, r8 = nblk & 7;
        const int xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    }
    constexpr int GM = 4;
    const int band = bid / (GM * p.tiles_n);
    const int band_rows = min(GM, p.tiles_m - band * GM);
    const int inb = bid - band * GM * p.tiles_n;
    const int tm = band * GM + inb % band_rows;
    const int tn = inb / band_rows;
    const int m0 = tm * BM, n0 = tn * BN;
    const int* __restrict__ a_rows = p.a_rows;
    const int* __restrict__ c_rows = p.c_rows;

    // ---- per-lane DMA sources: rows past M / N re-read the last row (never stored) ----
    const unsigned char* pa[LA];
    const unsigned char* pb[LB];
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int row = (wave + i * NW) * 8 + (lane >> 3);
        const int gch = (lane & 7) ^ ((row >> 1) & 7);
        int m = m0 + row;
        m = m < p.M ? m : p.M - 1;
        const long prow = a_rows ? (long)a_rows[m] : (long)m;
        pa[i] = p.A + prow * p.lda + gch * 16;
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
        const int row = (wave + i * NW) * 16 + (lane >> 2);
        const int gch = (lane & 3) ^ ((row >> 2) & 3);
        int n = n0 + row;
        n = n < p.N ? n : p.N - 1;
        pb[i] = p.Wq + (long)n * p.ldq + gch * 16;
    }

    // ---- fragment read offsets ----
    const int fr = lane & 15, q = lane >> 4;
    const int swa = fr >> 1;
    const int a_off = (wm * (BM / WM) + fr) * 128;
    const int a_c0 = (q ^ swa) * 16, a_c1 = ((q + 4) ^ swa) * 16;
    const int b_off = A_BYTES + (wn * (BN / WN) + fr) * 64 + ((q ^ (fr >> 2)) * 16);

    // ---- scale dwords: fragment j's row, lane group q, group g of four k-tiles ----
    const unsigned char* ps[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        int n = n0 + wn * (BN / WN) + j * 16 + fr;
        n = n < p.N ? n : p.N - 1;
        ps[j] = p.Ws + (long)n * p.lds + q * 4;
    }

    f32x4_t acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K >> 7;
    auto issue = [&](int stage, int kt) {
        const unsigned sb = smem_base + stage * STAGE;
#pragma unroll
        for (int i = 0; i < LA; ++i) w4g_glds16(pa[i] + (long)kt * 128, sb + (wave + i * NW) * 1024);
#pragma unroll
        for (int i = 0; i < LB; ++i) w4g_glds16(pb[i] + (long)kt * 64, sb + A_BYTES + (wave + i * NW) * 1024);
    };

    unsigned sc[NB], scn[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) scn[j] = *(const unsigned*)(ps[j]);

    auto compute = [&](const char* sb, auto U) {
        constexpr int u = decltype(U)::value;       // the byte selector of the block scale is an immediate of the instruction
        i32x8_t af[MB];
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const u32x4_t x0 = *(const u32x4_t*)(sb + a_off + i * 2048 + a_c0);
            const u32x4_t x1 = *(const u32x4_t*)(sb + a_off + i * 2048 + a_c1);
            af[i] = (i32x8_t){(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const u32x4_t w = *(const u32x4_t*)(sb + b_off + j * 1024);
            const i32x8_t wf = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < MB; ++i)     // A operand = weights (FP4: cbsz 4, scale byte u of the group's dword), B = activations (e4m3, 2^0)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, af[i], acc[i][j], 4, 0, u, (int)sc[j], 0, 127);
        }
    };

    // one k-tile: start the next tile's DMA, retire this one's (counted: the next stays in flight across the barrier), multiply
    auto step = [&](int kt, auto U) {
        constexpr int st = decltype(U)::value & 1;
        if (kt + 1 < nk) {
            issue(st ^ 1, kt + 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LA + LB) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_barrier" ::: "memory");
        compute(w4g_smem + st * STAGE, U);
        // every ds_read of this stage has returned before any wave may overwrite it
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };

    issue(0, 0);
    for (int kt = 0; kt < nk; kt += 4) {            // one scale group = four k-tiles
#pragma unroll
        for (int j = 0; j < NB; ++j) sc[j] = scn[j];
        if (kt + 4 < nk) {
#pragma unroll
            for (int j = 0; j < NB; ++j) scn[j] = *(const unsigned*)(ps[j] + (long)((kt >> 2) + 1) * 16);
        }
        step(kt, std::integral_constant<int, 0>{});
        if (kt + 1 < nk) step(kt + 1, std::integral_constant<int, 1>{});
        if (kt + 2 < nk) step(kt + 2, std::integral_constant<int, 2>{});
        if (kt + 3 < nk) step(kt + 3, std::integral_constant<int, 3>{});
    }

    // ---- epilogue: lane owns C[m][n .. n+3], n = fragment base + 4 q; activation scale first, then gemm.hip's rounding points ----
    const int nsub = q * 4;
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        const int m = m0 + wm * (BM / WM) + i * 16 + fr;
        if (m >= p.M) continue;
        const long arow = a_rows ? (long)a_rows[m] : (long)m;
        const long prow = c_rows ? (long)c_rows[m] : (long)m;
        const float sm = p.sa[arow];
        if (SWIGLU) {
#pragma unroll
            for (int j = 0; j < NB; j += 2) {
                const int nb0 = n0 + wn * (BN / WN) + j * 16;     // gate rows; up = +16
                if (nb0 + nsub >= p.N) continue;
                const int oc = (nb0 >> 1) + nsub;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = bfround(acc[i][j][e] * sm);
                    const float uu = bfround(acc[i][j + 1][e] * sm);
                    o[e] = bfround(silu_f(g)) * uu;
                }
                const u32x2_t v = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
                *(u32x2_t*)(p.C + prow * p.ldc + oc) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int n = n0 + wn * (BN / WN) + j * 16 + nsub;
                if (n >= p.N) continue;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = acc[i][j][e] * sm;
                if (p.bias) {
                    const u32x2_t bv = *(const u32x2_t*)(p.bias + n);
                    o[0] += lo2f(bv[0]); o[1] += hi2f(bv[0]); o[2] += lo2f(bv[1]); o[3] += hi2f(bv[1]);
                }
                if (p.R) {
                    const u32x2_t rv = *(const u32x2_t*)(p.R + prow * p.ldr + n);
                    o[0] = bfround(o[0]) + lo2f(rv[0]); o[1] = bfround(o[1]) + hi2f(rv[0]);
                    o[2] = bfround(o[2]) + lo2f(rv[1]); o[3] = bfround(o[3]) + hi2f(rv[1]);
                }
                const u32x2_t v = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
                *(u32x2_t*)(p.C + prow * p.ldc + n) = v;
            }
        }
    }
}

// Tile shapes: 128 x 256 (waves of 64 x 128: 512 LDS bytes read per MFMA, two workgroups per CU) is the default; 128 x 128 (waves of 64 x 64, three
// workgroups per CU) is kept for same-box A/B runs (BAGEL_GEMM_W4_TILE=1) and serves N <= 128.
template <int BN, int OCC, bool SWIGLU>
static int launch_gemm_w4_tile(GemmW4Params& p, hipStream_t stream) {
    constexpr int BM = 128, WM = 2, WN = 2;
    constexpr int smem = 2 * (BM * 128 + BN * 64);
    p.tiles_m = ceil_div(p.M, BM);
    p.tiles_n = ceil_div(p.N, BN);
    if (int rc = bagel_enable_lds((const void*)gemm_w4_kernel<BM, BN, WM, WN, OCC, SWIGLU>, smem, "gemm_w4_kernel")) return rc;
    hipLaunchKernelGGL((gemm_w4_kernel<BM, BN, WM, WN, OCC, SWIGLU>), dim3(p.tiles_m * p.tiles_n), dim3(WM * WN * 64), smem, stream, p);
    return bagel_check_launch("gemm_w4_kernel");
}

template <bool SWIGLU>
static int launch_gemm_w4(GemmW4Params& p, hipStream_t stream) {
    static int tile = -1;
    if (tile < 0) {
        const char* e = getenv("BAGEL_GEMM_W4_TILE");     // tuning knob; the default is what the probe measures
        tile = (e && atoi(e) > 0) ? atoi(e) : 0;
    }
    if (tile == 1 || p.N <= 128) return launch_gemm_w4_tile<128, 3, SWIGLU>(p, stream);
    return launch_gemm_w4_tile<256, 2, SWIGLU>(p, stream);
}

extern "C" int bagel_gemm_w4_bf16(const void* Aq, int64_t lda_bytes, const float* sa, const void* Wq, int64_t ldq_bytes, const void* Ws,
                                  int64_t lds_bytes, const void* bias, const int32_t* a_rows, const int32_t* c_rows, int32_t M, const void* R,
                                  int64_t ldr, void* C, int64_t ldc, int32_t N, int32_t K, int32_t epilogue, hipStream_t stream) {
    BAGEL_REQUIRE(Aq && sa && Wq && Ws && C, "gemm_w4: null pointer");
    BAGEL_REQUIRE(K > 0 && (K % 128) == 0, "gemm_w4: K=%d must be a multiple of 128", K);
    BAGEL_REQUIRE(N > 0 && (N % 8) == 0, "gemm_w4: N=%d must be a multiple of 8", N);
    BAGEL_REQUIRE(epilogue == EPI_NONE || epilogue == EPI_SWIGLU16, "gemm_w4: epilogue %d not in {none, swiglu16}", epilogue);
    BAGEL_REQUIRE(epilogue != EPI_SWIGLU16 || ((N % 32) == 0 && !bias && !R), "gemm_w4: swiglu needs N%%32==0, no bias/residual");
    BAGEL_REQUIRE(lda_bytes >= K && (lda_bytes % 16) == 0 && ldq_bytes >= K / 2 && (ldq_bytes % 16) == 0, "gemm_w4: lda/ldq must cover a row and keep it 16-byte aligned");
    BAGEL_REQUIRE(lds_bytes >= ((K / 128 + 3) / 4) * 16 && (lds_bytes % 4) == 0, "gemm_w4: lds_bytes too small");
    BAGEL_REQUIRE((ldc % 4) == 0 && (ldr % 4) == 0, "gemm_w4: ldc/ldr must be multiples of 4");
    BAGEL_REQUIRE((((uintptr_t)Aq | (uintptr_t)Wq) & 15) == 0 && (((uintptr_t)Ws | (uintptr_t)sa | (uintptr_t)a_rows | (uintptr_t)c_rows) & 3) == 0 &&
                  (((uintptr_t)C | (uintptr_t)R | (uintptr_t)bias) & 7) == 0, "gemm_w4: alignment");
    if (M <= 0) return BAGEL_OK;
    GemmW4Params p;
    p.A = (const unsigned char*)Aq; p.lda = lda_bytes; p.sa = sa;
    p.Wq = (const unsigned char*)Wq; p.ldq = ldq_bytes; p.Ws = (const unsigned char*)Ws; p.lds = lds_bytes;
    p.bias = (const bf16_t*)bias; p.a_rows = a_rows; p.c_rows = c_rows;
    p.R = (const bf16_t*)R; p.ldr = ldr; p.C = (bf16_t*)C; p.ldc = ldc;
    p.M = M; p.N = N; p.K = K; p.epi = epilogue;
    if (epilogue == EPI_SWIGLU16) return launch_gemm_w4<true>(p, stream);
    return launch_gemm_w4<false>(p, stream);
}
