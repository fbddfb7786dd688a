// Host-side launch planning of libbagel_hip.so: the schedules that plain C++ computes before a launch, and the error convention they
// report through.  No HIP header and no device type: host_plan.cpp builds with a plain C++17 compiler, so tests/host_plan_fuzz.cpp
// runs every planner under ASan + UBSan on the CPU.  common.h includes this file; the .hip launchers see the same declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>
// the public C ABI: every translation unit sees the prototypes of the entry points it defines, so a definition that drifts from include/bagel_hip.h is a
// COMPILE error ("conflicting types") instead of a ctypes call with the wrong arguments at run time
#include "../../include/bagel_hip.h"

#define BAGEL_OK 0
#define BAGEL_ERR_ARG (-1)
#define BAGEL_ERR_LAUNCH (-2)
#define BAGEL_ERR_UNSUPPORTED (-3)

int bagel_set_error(int code, const char* fmt, ...);      // runtime.hip (the fuzz program brings its own)

#define BAGEL_REQUIRE(cond, ...)                                  \
    do {                                                          \
        if (!(cond)) return bagel_set_error(BAGEL_ERR_ARG, __VA_ARGS__); \
    } while (0)

// ---- attention2.hip: the work list bagel_attn_plan writes and attn2_kernel walks ----
struct AttnItem {        // 16 ints = 64 bytes, written by the host planner
    int q_row0;          // absolute row (q / out buffers) of the item's first query row
    int nrows;           // live query rows: <= 256 (head-per-wave form: <= 32)
    int h;               // query head (head-per-wave: first head of the KV group)
    int g;               // KV head
    int flags;           // bit 0 head-per-wave, bit 1 causal, bit 2 partial output; bits 8..15 = G (waves that are live in head-per-wave form)
    int q_rel0;          // index of the first query row inside its sample's new segment (causal mask)
    int kn_row0;         // absolute row of new-segment key 0 in k_new
    int l_new;           // keys in the sample's new segment
    int kc_row0;         // absolute row of context key 0 in k_ctx
    int l_ctx;           // context keys
    int vtn_col0;        // V^T column of new-segment key 0
    int vtc_col0;        // V^T column of context key 0
    int t0, t1;          // 64-key tile range [t0, t1) over the sample's tile list [context tiles | new tiles]
    int part;            // partial slot (flags bit 2)
    int pad;
};
#define ATTN2_HPW 1
#define ATTN2_CAUSAL 2
#define ATTN2_PARTIAL 4

struct AttnComb {        // 8 ints: one key-split item = `nslots` consecutive partial slots -> one output tile
    int q_row0, nrows, h, flags, slot0, nslots, pad0, pad1;
};

// ---- gemm.hip: K-split of the persistent GEMM's last round (policy / force: BAGEL_GEMM_SPLIT_POLICY / _FORCE, read by the launcher) ----
int pq_leftover_split(int nblk, int wgs, int nk, size_t ws_bytes, int policy, int force, int* n_full_out);

// ---- gemv_mb.hip: instantiation (NS fragments per wave), k-steps per wave, K slices (gridDim.y) and workgroups per slice (gridDim.x) ----
struct MbGeometry { int NS, per, KS, gx; };
void mb_geometry(int N, int K, int wgs, int MB, int* per, int* KS, int* gx_out);
// the shape verdict of bagel_gemv_mb_bf16 on `wgs` workgroups: 0 and the geometry, or the refusal the launcher reports
int mb_plan(int M, int N, int K, int epilogue, bool has_norm, int wgs, MbGeometry* g);

// ---- gemv_mb_w4.hip: the same stream on MXFP4 codes.  K is counted in 128-deep k-steps and handed out in scale groups of four (one scale dword per lane):
//      a slice (gridDim.y) takes gps groups, each of its 8 waves gpw of them (NS = 4 gpw fragments per wave: the instantiation) ----
#ifdef __HIPCC__
#define BAGEL_HD __host__ __device__
#else
#define BAGEL_HD
#endif
struct MbW4Geometry { int NS, gpw, gps, KS, gx, MB; };
// k-steps [*s0, *s0 + *ns) of wave `wave` of slice `slice` (*ns == 0: the wave has no work; *s0 is a multiple of 4 either way): the kernel and the fuzz program share it
BAGEL_HD static inline void mbw4_wave_steps(int gpw, int gps, int nsteps, int slice, int wave, int* s0, int* ns) {
    const int G = (nsteps + 3) >> 2;
    int g0 = slice * gps + wave * gpw, g1 = g0 + gpw;
    const int gend = (slice + 1) * gps < G ? (slice + 1) * gps : G;
    g1 = g1 < gend ? g1 : gend;
    *s0 = 4 * g0;
    const int s1 = 4 * g1 < nsteps ? 4 * g1 : nsteps;
    *ns = g0 < g1 ? s1 - 4 * g0 : 0;
}
// the shape verdict of bagel_gemv_mb_w4_bf16 on `wgs` workgroups: 0 and the geometry, or the refusal the launcher reports (g is then untouched)
int mbw4_plan(int M, int N, int K, int epilogue, int wgs, MbW4Geometry* g);

// ---- gemv_mb_nf4.hip: the same stream on NF4 codes.  K is counted in k-groups of 128 weights (64 code bytes per weight row: one 16-byte load per lane, two
//      absmax blocks); a slice (gridDim.y) takes gps groups, each of its 8 waves gpw of them (GP = 1, 2 or 4 >= gpw fragments per wave: the instantiation) ----
struct MbNf4Geometry { int GP, gpw, gps, KS, gx, MB; };
// k-groups [*g0, *g0 + *ng) of wave `wave` of slice `slice` out of the row's G = K / 128 (*ng == 0: the wave has no work): the kernel and the fuzz program share it
BAGEL_HD static inline void mbnf4_wave_groups(int gpw, int gps, int G, int slice, int wave, int* g0, int* ng) {
    const int a = slice * gps + wave * gpw;
    int gend = (slice + 1) * gps;
    gend = gend < G ? gend : G;
    int b = a + gpw;
    b = b < gend ? b : gend;
    *g0 = a;
    *ng = a < b ? b - a : 0;
}
// the shape verdict of bagel_gemv_mb_nf4_bf16 on `wgs` workgroups: 0 and the geometry, or the refusal the launcher reports (g is then untouched)
int mbnf4_plan(int M, int N, int K, int epilogue, int wgs, MbNf4Geometry* g);

// ---- engine.hip: per-phase unit form and the LDS ring beside the activation vector and the sync block ----
#define ENG_MAXPH 4
#define ENG_MAX_SLOTS 8
#define ENG_MAX_DPAIRS 32                 // split-K pairs one workgroup may own (partials live in LDS)
#define ENG_SYNC_BYTES 2560
#define ENG_LDS_MAX (160 * 1024)
struct EngGeometry {
    int kind[ENG_MAXPH], ngr[ENG_MAXPH], gq[ENG_MAXPH];      // see EngPhase
    int xs_bytes, slot_bytes, nslot, nloaders, depth, waves, n_wg;
};
// validates ptrs / dims as bagel_decode_engine_bf16 documents them; want_slots / waves / loaders / depth: the BAGEL_ENGINE_* knobs, read by the launcher
int eng_geometry(const void* const* ptrs, const int64_t* dims, int n_phases, int n_wg, int want_slots, int waves, int loaders, int depth,
                 EngGeometry* out);
