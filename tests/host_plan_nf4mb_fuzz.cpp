// Stand-alone fuzz of the launch planner of the NF4 batched-decode stream (mbnf4_plan / mbnf4_wave_groups, bagel_amd/csrc/host_plan.cpp + host_plan.h):
// links that one file and nothing else -- no HIP, no Python, no shared library -- so it runs under ASan + UBSan on the CPU
// (tests/test_host_plan_nf4mb_cpu.py builds and runs it).  Exhaustive over its grid; aborts on the first violated invariant.
#include "../bagel_amd/csrc/host_plan.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static char g_err[512];
int bagel_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                    \
            fprintf(stderr, "\n");                                           \
            abort();                                                         \
        }                                                                    \
    } while (0)

static bool untouched(const MbNf4Geometry& g) { return g.GP == -1 && g.gpw == -1 && g.gps == -1 && g.KS == -1 && g.gx == -1 && g.MB == -1; }

static long fuzz_plans() {
    static const int Ms[] = {1, 5, 16, 17, 32}, wgss[] = {1, 8, 64, 256, 304}, Ns[] = {16, 32, 48, 64, 4608, 37888};
    long n = 0;
    std::vector<int> cover;
    for (int K = 128; K <= 32768; K += 128) {
        const int G = K / 128;
        for (int N : Ns) {
            int64_t ws_bytes = -1;
            CHECK(bagel_gemv_mb_nf4_workspace_bytes(N, K, &ws_bytes) == 0 && ws_bytes >= 0, "workspace_bytes(%d, %d)", N, K);
            for (int M : Ms) for (int epi = 0; epi <= 3; epi += 3) for (int wgs : wgss) {
                MbNf4Geometry g = {-1, -1, -1, -1, -1, -1};
                const int rc = mbnf4_plan(M, N, K, epi, wgs, &g);
                if (epi == 3 && N % 32) {                                      // SwiGLU pairs whole 32-row blocks: a refusal, never a partial plan
                    CHECK(rc == BAGEL_ERR_ARG && untouched(g), "M %d N %d K %d: SwiGLU on N %% 32 != 0 gave rc %d", M, N, K, rc);
                    continue;
                }
                CHECK(rc == 0, "M %d N %d K %d epi %d wgs %d: rc %d (%s)", M, N, K, epi, wgs, rc, g_err);
                CHECK((g.GP == 1 || g.GP == 2 || g.GP == 4) && g.gpw >= 1 && g.gpw <= g.GP && g.MB == (M > 16 ? 2 : 1), "M %d K %d: GP %d gpw %d MB %d", M, K, g.GP,
                      g.gpw, g.MB);
                CHECK(g.KS >= 1 && g.gps >= 1 && g.gps <= 8 * g.gpw, "M %d K %d wgs %d: %d slices of %d groups, %d per wave", M, K, wgs, g.KS, g.gps, g.gpw);
                CHECK(g.gx >= 1 && g.gx <= N / (epi == 3 ? 32 : 16) && (long)g.gx * g.KS <= (wgs > g.KS ? wgs : g.KS), "M %d N %d K %d wgs %d: grid %d x %d", M, N, K, wgs, g.gx, g.KS);
                // every k-group exactly once across the waves and slices, no wave past its instantiation, no slice empty
                cover.assign(G, 0);
                for (int s = 0; s < g.KS; ++s) {
                    int in_slice = 0;
                    for (int w = 0; w < 8; ++w) {
                        int g0 = -1, ng = -1;
                        mbnf4_wave_groups(g.gpw, g.gps, G, s, w, &g0, &ng);
                        CHECK(g0 >= 0 && ng >= 0 && ng <= g.GP, "K %d slice %d wave %d: groups [%d, +%d)", K, s, w, g0, ng);
                        CHECK(ng == 0 || g0 + ng <= G, "K %d slice %d wave %d: [%d, +%d) leaves the row", K, s, w, g0, ng);
                        for (int i = 0; i < ng; ++i) ++cover[g0 + i];
                        in_slice += ng;
                    }
                    CHECK(in_slice > 0, "K %d: slice %d of %d is empty", K, s, g.KS);
                }
                for (int k = 0; k < G; ++k) CHECK(cover[k] == 1, "M %d N %d K %d wgs %d: k-group %d covered %d times", M, N, K, wgs, k, cover[k]);
                CHECK(g.KS == 1 || ws_bytes >= (int64_t)g.KS * 16 * g.MB * N * 4, "M %d N %d K %d wgs %d: %d slices need more than workspace_bytes = %lld", M, N, K, wgs,
                      g.KS, (long long)ws_bytes);
                int32_t per, sg, ks, gx;
                CHECK(bagel_gemv_mb_nf4_geometry(M, N, K, epi, wgs, &per, &sg, &ks, &gx) == 0 && per == g.gpw && sg == g.gps && ks == g.KS && gx == g.gx,
                      "the entry point disagrees");
                ++n;
            }
        }
    }
    return n;
}

static long fuzz_refusals() {
    struct { int M, N, K, epi, wgs; } bad[] = {{0, 64, 256, 0, 256}, {33, 64, 256, 0, 256}, {-1, 64, 256, 0, 256}, {8, 64, 192, 0, 256}, {8, 64, 0, 0, 256},
                                               {8, 64, -128, 0, 256}, {8, 40, 256, 0, 256}, {8, 0, 256, 0, 256}, {8, 48, 256, 3, 256}, {8, 64, 256, 1, 256},
                                               {8, 64, 256, 2, 256}, {8, 64, 256, 4, 256}, {8, 64, 256, 0, 0}, {8, 64, 256, 0, -3}};
    long n = 0;
    for (auto& b : bad) {
        MbNf4Geometry g = {-1, -1, -1, -1, -1, -1};
        g_err[0] = 0;
        CHECK(mbnf4_plan(b.M, b.N, b.K, b.epi, b.wgs, &g) == BAGEL_ERR_ARG && untouched(g) && g_err[0], "M %d N %d K %d epi %d wgs %d was not refused cleanly", b.M, b.N,
              b.K, b.epi, b.wgs);
        int32_t o[4] = {-7, -7, -7, -7};
        CHECK(bagel_gemv_mb_nf4_geometry(b.M, b.N, b.K, b.epi, b.wgs, &o[0], &o[1], &o[2], &o[3]) == BAGEL_ERR_ARG && o[0] == -7 && o[1] == -7 && o[2] == -7 && o[3] == -7,
              "the entry point wrote a partial geometry");
        ++n;
    }
    int64_t bytes = -7;
    CHECK(bagel_gemv_mb_nf4_workspace_bytes(64, 192, &bytes) == BAGEL_ERR_ARG && bytes == -7, "workspace_bytes accepted K = 192");
    CHECK(bagel_gemv_mb_nf4_workspace_bytes(64, 256, nullptr) == BAGEL_ERR_ARG, "workspace_bytes accepted a null pointer");
    CHECK(mbnf4_plan(8, 64, 256, 0, 256, nullptr) == BAGEL_ERR_ARG, "a null geometry was accepted");
    return n;
}

int main() {
    const long plans = fuzz_plans();
    const long refusals = fuzz_refusals();
    // the 7B shapes as host_plan.cpp documents them (256 workgroups)
    MbNf4Geometry g;
    CHECK(mbnf4_plan(32, 4608, 3584, 0, 256, &g) == 0 && g.KS == 1 && g.GP == 4 && g.gpw == 4 && g.gps == 28 && g.gx == 256 && g.MB == 2, "7B qkv");
    CHECK(mbnf4_plan(16, 37888, 3584, 3, 256, &g) == 0 && g.KS == 1 && g.GP == 4 && g.gx == 256 && g.MB == 1, "7B gate/up");
    CHECK(mbnf4_plan(32, 3584, 18944, 0, 256, &g) == 0 && g.KS == 10 && g.gps == 15 && g.GP == 2 && g.gx == 25, "7B down: %d x %d, %d groups", g.KS, g.gx, g.gps);
    printf("ok: %ld plans, %ld refusals\n", plans, refusals);
    return 0;
}
