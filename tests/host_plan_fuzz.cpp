// Stand-alone fuzz of the host-side launch planners (bagel_amd/csrc/host_plan.cpp): links that file and nothing else -- no HIP, no Python, no shared
// library -- so it runs under ASan + UBSan on the CPU (tests/test_host_plan_cpu.py builds and runs it).  Fixed seed; aborts on the first violated invariant.
#include "../bagel_amd/csrc/host_plan.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <random>
#include <string>
#include <tuple>
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

static std::mt19937 rng(20261018u);
static int rnd(int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); }      // inclusive
template <typename T, size_t n> static T pick(const T (&a)[n]) { return a[rng() % n]; }
static int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- attention plans ----------------------------------------------------------------------------------------------------------------
struct Geo {
    std::vector<int32_t> q_len, ctx_len;      // ctx_len empty + has_ctx false: no context pointers
    bool has_ctx;
    int nq, nkv, causal, n_workers, split_min;
};

static std::string show(const Geo& g) {
    std::string s = "q_len [";
    for (int v : g.q_len) s += std::to_string(v) + " ";
    s += g.has_ctx ? "] ctx_len [" : "] no ctx [";
    for (int v : g.ctx_len) s += std::to_string(v) + " ";
    return s + "] heads " + std::to_string(g.nq) + "/" + std::to_string(g.nkv) + " causal " + std::to_string(g.causal) + " workers " +
           std::to_string(g.n_workers) + " split_min " + std::to_string(g.split_min);
}

static void check_attn(const Geo& g) {
    const int B = (int)g.q_len.size(), G = g.nq / g.nkv;
    std::vector<int32_t> q_start(B + 1), ctx_start(B + 1), vt_new(B + 1), vt_ctx(B + 1);      // + 1: a non-null pointer at batch 0
    int row = rnd(0, 3), crow = 0, col = 0, ccol = 0;
    for (int b = 0; b < B; ++b) {
        q_start[b] = row; row += g.q_len[b] + rnd(0, 2);                       // packed rows, small gaps
        vt_new[b] = col; col += cdiv(g.q_len[b] > 0 ? g.q_len[b] : 1, 64) * 64;
        const int C = g.has_ctx ? g.ctx_len[b] : 0;
        ctx_start[b] = crow; crow += C;
        vt_ctx[b] = ccol; ccol += cdiv(C > 0 ? C : 1, 64) * 64;
    }
    std::vector<int32_t> ctx_len(g.ctx_len);
    ctx_len.push_back(0);
    std::vector<int32_t> q_len(g.q_len);
    q_len.push_back(0);
    auto plan_into = [&](int32_t* buf, int64_t ints) {
        return bagel_attn_plan(q_start.data(), q_len.data(), g.has_ctx ? ctx_start.data() : nullptr, g.has_ctx ? ctx_len.data() : nullptr, vt_new.data(),
                               g.has_ctx ? vt_ctx.data() : nullptr, B, g.nq, g.nkv, g.causal, g.n_workers, g.split_min, buf, ints);
    };
    const std::string what = show(g);
    // the capacity ops.AttnPlan.__init__ allocates (bagel_amd/ops.py: items_max / cap) -- the caller's half of the contract
    long tiles_q = 0;
    for (int b = 0; b < B; ++b) tiles_q += g.q_len[b] > 0 ? cdiv(g.q_len[b], 256) : 0;
    const long items_max = 2 * tiles_q * g.nq + 4L * g.n_workers;
    const long cap = 8 + g.n_workers + 1 + 16 + 16 * items_max + 8L * g.n_workers;
    static std::vector<int32_t> big(1 << 22);
    CHECK(plan_into(big.data(), (int64_t)big.size()) == 0, "%s: %s", what.c_str(), g_err);
    const int n_items = big[1], n_comb = big[2], n_slots = big[3], off_items = big[4], off_comb = big[5];
    const long need = (long)off_comb + 8L * n_comb;
    CHECK(need <= cap, "%s: the plan needs %ld ints, ops.AttnPlan allocates %ld", what.c_str(), need, cap);
    // exactly `need` ints on the heap: succeeds, same plan, and an overrun is ASan's to see; one int short: refused, nothing written
    {
        int32_t* exact = new int32_t[need];
        CHECK(plan_into(exact, need) == 0, "%s: exact-size buffer refused: %s", what.c_str(), g_err);
        CHECK(memcmp(exact, big.data(), need * 4) == 0, "%s: the plan depends on the buffer size", what.c_str());
        delete[] exact;
        int32_t* shorter = new int32_t[need - 1];
        for (long i = 0; i < need - 1; ++i) shorter[i] = 0x5a5a5a5a;
        CHECK(plan_into(shorter, need - 1) != 0, "%s: a buffer one int short was accepted", what.c_str());
        for (long i = 0; i < need - 1; ++i) CHECK(shorter[i] == 0x5a5a5a5a, "%s: a refused call wrote plan[%ld]", what.c_str(), i);
        delete[] shorter;
    }
    const int32_t* p = big.data();
    CHECK(p[0] == g.n_workers && off_items % 16 == 0 && off_items >= 8 + g.n_workers + 1 && off_comb == off_items + 16 * n_items, "%s: header", what.c_str());
    CHECK(p[8] == 0 && p[8 + g.n_workers] == n_items, "%s: worker_off ends at %d, n_items %d", what.c_str(), p[8 + g.n_workers], n_items);
    for (int w = 0; w < g.n_workers; ++w) CHECK(p[8 + w] <= p[8 + w + 1], "%s: worker_off not monotone at %d", what.c_str(), w);
    const AttnItem* items = (const AttnItem*)(p + off_items);
    const AttnComb* combs = (const AttnComb*)(p + off_comb);
    std::map<std::tuple<int, int, int>, std::vector<int>> cover;            // (sample, head, query tile) -> times each key tile is visited
    std::vector<int> slot_written(n_slots, 0), slot_read(n_slots, 0), slot_comb(n_slots, -1);
    for (int c = 0; c < n_comb; ++c) {
        CHECK(combs[c].nslots >= 2 && combs[c].slot0 >= 0 && combs[c].slot0 + combs[c].nslots <= n_slots, "%s: combine %d slots", what.c_str(), c);
        for (int s = combs[c].slot0; s < combs[c].slot0 + combs[c].nslots; ++s) { ++slot_read[s]; slot_comb[s] = c; }
    }
    for (int i = 0; i < n_items; ++i) {
        const AttnItem& it = items[i];
        int b = -1;
        for (int j = 0; j < B; ++j) if (g.q_len[j] > 0 && it.q_row0 >= q_start[j] && it.q_row0 < q_start[j] + g.q_len[j]) b = j;
        CHECK(b >= 0, "%s: item %d row %d belongs to no sample", what.c_str(), i, it.q_row0);
        const int Lq = g.q_len[b], C = g.has_ctx ? g.ctx_len[b] : 0, rel = it.q_row0 - q_start[b], qt = rel / 256;
        const bool hpw = it.flags & ATTN2_HPW, partial = it.flags & ATTN2_PARTIAL;
        const int nrows = Lq - rel < 256 ? Lq - rel : 256;
        const int vis = g.causal ? (256 * qt + nrows < Lq ? 256 * qt + nrows : Lq) : Lq;
        const int tiles = cdiv(C, 64) + cdiv(vis, 64);                      // key tiles the mask can reach from this query tile
        CHECK(rel % 256 == 0 && it.q_rel0 == rel && it.nrows == nrows && it.nrows >= 1 && it.nrows <= (hpw ? 32 : 256), "%s: item %d rows", what.c_str(), i);
        CHECK(0 <= it.t0 && it.t0 < it.t1 && it.t1 <= tiles, "%s: item %d tiles [%d, %d) of %d", what.c_str(), i, it.t0, it.t1, tiles);
        CHECK(it.kn_row0 == q_start[b] && it.l_new == Lq && it.l_ctx == C && it.vtn_col0 == vt_new[b], "%s: item %d sample fields", what.c_str(), i);
        CHECK(C == 0 || (it.kc_row0 == ctx_start[b] && it.vtc_col0 == vt_ctx[b]), "%s: item %d context fields", what.c_str(), i);
        CHECK(((it.flags >> 8) & 255) == G && !(it.flags & ATTN2_CAUSAL) == !g.causal && it.g == it.h / G && it.h >= 0 && it.h < g.nq, "%s: item %d heads", what.c_str(), i);
        CHECK(!hpw || (G > 1 && G <= 8 && it.h % G == 0), "%s: item %d head-per-wave form", what.c_str(), i);
        if (partial) {
            CHECK(it.part >= 0 && it.part < n_slots, "%s: item %d slot %d", what.c_str(), i, it.part);
            ++slot_written[it.part];
            const AttnComb& c = combs[slot_comb[it.part] < 0 ? 0 : slot_comb[it.part]];
            CHECK(slot_comb[it.part] >= 0 && c.q_row0 == it.q_row0 && c.h == it.h && c.nrows == it.nrows && c.flags == (it.flags & ~ATTN2_PARTIAL),
                  "%s: item %d and the combine of its slot disagree", what.c_str(), i);
        } else {
            CHECK(it.part == -1 && it.t0 == 0 && it.t1 == tiles, "%s: whole item %d covers [%d, %d) of %d", what.c_str(), i, it.t0, it.t1, tiles);
        }
        for (int h = it.h; h < it.h + (hpw ? G : 1); ++h) {
            std::vector<int>& v = cover[{b, h, qt}];
            v.resize(tiles, 0);
            for (int t = it.t0; t < it.t1; ++t) ++v[t];
        }
    }
    for (int s = 0; s < n_slots; ++s) CHECK(slot_written[s] == 1 && slot_read[s] == 1, "%s: slot %d written %d read %d times", what.c_str(), s, slot_written[s], slot_read[s]);
    long want = 0;
    for (int b = 0; b < B; ++b) want += g.q_len[b] > 0 ? (long)cdiv(g.q_len[b], 256) * g.nq : 0;
    CHECK((long)cover.size() == want, "%s: %zu (sample, head, query tile) triples covered, %ld exist", what.c_str(), cover.size(), want);
    for (auto& kv : cover)
        for (size_t t = 0; t < kv.second.size(); ++t)
            CHECK(kv.second[t] == 1, "%s: sample %d head %d query tile %d key tile %zu visited %d times", what.c_str(), std::get<0>(kv.first),
                  std::get<1>(kv.first), std::get<2>(kv.first), t, kv.second[t]);
}

static void fuzz_attn() {
    static const int heads[][2] = {{1, 1}, {4, 2}, {16, 2}, {28, 4}, {32, 2}};
    static const int workers[] = {8, 64, 256, 512}, splits[] = {0, 2, 16};
    for (int it = 0; it < 2000; ++it) {
        Geo g;
        const int B = rnd(0, 6), mode = rnd(0, 2);                             // context: absent / all zero / some
        for (int b = 0; b < B; ++b) g.q_len.push_back(rnd(0, 6) == 0 ? 0 : rnd(1, 1500));
        g.has_ctx = mode != 0;
        if (g.has_ctx) for (int b = 0; b < B; ++b) g.ctx_len.push_back(mode == 1 || rnd(0, 2) == 0 ? 0 : rnd(1, 10000));
        const int hi = rnd(0, 4);
        g.nq = heads[hi][0]; g.nkv = heads[hi][1];
        g.causal = rnd(0, 1); g.n_workers = pick(workers); g.split_min = pick(splits);
        check_attn(g);
    }
    // the benchmark's launches (tests/test_attn_plan_cpu.py): stream-batched denoise, 3-stream edit, one denoise stream, the causal prefill, SigLIP
    check_attn({{4098, 4098, 4098, 4098, 4098, 4098, 4098, 4098}, {32, 32, 32, 32, 0, 0, 0, 0}, true, 28, 4, 0, 256, 0});
    check_attn({{4098, 4098, 4098}, {9032, 9000, 32}, true, 28, 4, 0, 256, 0});
    check_attn({{4098, 4098, 4098, 4098}, {32, 32, 32, 32}, true, 28, 4, 0, 256, 0});
    check_attn({{4936}, {0}, true, 28, 4, 1, 256, 0});
    check_attn({{4900}, {0}, true, 16, 16, 0, 256, 0});
}

// ---- K-split of the persistent GEMM's last round ---------------------------------------------------------------------------------------
static long fuzz_pq() {
    static const int wgss[] = {8, 64, 256, 304}, nks[] = {1, 2, 15, 16, 18, 56, 296}, forces[] = {0, 3};
    static const size_t wss[] = {0, (size_t)64 << 20, (size_t)128 << 20};
    long n = 0;
    for (int nblk = 1; nblk <= 2048; ++nblk)
        for (int wgs : wgss) for (int nk : nks) for (size_t ws : wss) for (int policy = 0; policy < 2; ++policy) for (int force : forces) {
            int n_full = -1;
            const int s = pq_leftover_split(nblk, wgs, nk, ws, policy, force, &n_full);
            const int rest = nblk - n_full;
            CHECK(n_full >= 0 && n_full % wgs == 0 && n_full <= nblk && rest < wgs, "pq: nblk %d wgs %d: n_full %d", nblk, wgs, n_full);
            CHECK(s >= 1, "pq: nblk %d wgs %d nk %d: split %d", nblk, wgs, nk, s);
            CHECK(s == 1 || (s <= nk / 4 && (size_t)rest * s * (256 * 1024) <= ws), "pq: nblk %d wgs %d nk %d ws %zu policy %d force %d: split %d", nblk, wgs,
                  nk, ws, policy, force, s);
            int32_t nf2 = -1, s2 = -1;
            CHECK(bagel_gemm_leftover_split(nblk, wgs, nk, (int64_t)ws, policy, force, &nf2, &s2) == 0 && nf2 == n_full && s2 == s, "pq: the entry point disagrees");
            ++n;
        }
    return n;
}

// ---- batched-decode weight stream --------------------------------------------------------------------------------------------------------
static long fuzz_mb() {
    static const int Ms[] = {1, 16, 17, 32}, wgss[] = {1, 8, 255, 256, 304}, Ns[] = {32, 544, 3584};
    long n = 0;
    for (int K = 32; K <= 32768; K += 32)
        for (int M : Ms) for (int N : Ns) for (int epi = 0; epi <= 3; epi += 3) for (int norm = 0; norm < 2; ++norm) {
            int64_t ws_bytes = -1;
            CHECK(bagel_gemv_mb_workspace_bytes(N, K, &ws_bytes) == 0 && ws_bytes >= 0, "mb: workspace_bytes(%d, %d)", N, K);
            int verdict = 1;
            for (int wgs : wgss) {
                MbGeometry g = {-1, -1, -1, -1};
                const int rc = mb_plan(M, N, K, epi, norm != 0, wgs, &g);
                CHECK(rc == 0 || rc == BAGEL_ERR_UNSUPPORTED, "mb: M %d N %d K %d: rc %d (%s)", M, N, K, rc, g_err);
                CHECK(verdict == 1 || verdict == rc, "mb: M %d N %d K %d: the verdict depends on the workgroup count", M, N, K);
                verdict = rc;
                CHECK(8L * g.KS * g.per * 32 >= K && g.KS >= 1 && g.per >= 1, "mb: M %d K %d wgs %d: %d slices x %d steps do not cover the row", M, K, wgs, g.KS, g.per);
                if (rc != 0) continue;
                CHECK((g.NS == 4 || g.NS == 10 || g.NS == 14 || g.NS == 19) && g.per <= g.NS && K / 32 >= g.NS && (M <= 16 || g.NS <= 14),
                      "mb: M %d K %d wgs %d: NS %d per %d", M, K, wgs, g.NS, g.per);
                CHECK(g.gx >= 1 && g.gx <= N / (epi == 3 ? 32 : 16), "mb: M %d N %d K %d wgs %d: gx %d", M, N, K, wgs, g.gx);
                CHECK(g.KS == 1 || (!norm && epi != 3), "mb: a sliced row was served with norm / SwiGLU");
                const int slab_rows = M > 16 ? 32 : 16;
                CHECK(g.KS == 1 || ws_bytes >= (int64_t)g.KS * slab_rows * N * 4, "mb: M %d N %d K %d wgs %d: %d slices need more than workspace_bytes = %lld", M, N, K,
                      wgs, g.KS, (long long)ws_bytes);
                int32_t per, ks, gx;
                CHECK(bagel_gemv_mb_geometry(M, N, K, epi, norm, wgs, &per, &ks, &gx) == 0 && per == g.per && ks == g.KS && gx == g.gx, "mb: the entry point disagrees");
                ++n;
            }
        }
    MbGeometry g;                                                              // the 7B down projection as gemv_mb.hip documents it
    CHECK(mb_plan(16, 3584, 18944, 0, false, 256, &g) == 0 && g.KS == 8 && g.gx == 32 && g.per == 10 && g.NS == 10, "mb: 7B down: %d x %d x %d", g.KS, g.gx, g.per);
    return n;
}

// ---- decode engine -----------------------------------------------------------------------------------------------------------------------
static long fuzz_engine() {
    static const int wgs[] = {8, 256, 304};
    long accepted = 0;
    for (int it = 0; it < 20000; ++it) {
        const int nph = rnd(1, 4);
        const void* ptrs[6 * ENG_MAXPH];
        int64_t dims[4 * ENG_MAXPH];
        int K = 8 * rnd(1, rnd(0, 3) ? 640 : 4096);                            // mostly the lengths a model has, some up to 32 768
        for (int i = 0; i < nph; ++i) {
            const bool norm = rnd(0, 1), swiglu = rnd(0, 5) == 0;
            int N = 2 * rnd(1, rnd(0, 3) ? 2560 : 16384);
            if (i + 1 < nph && rnd(0, 7)) N = swiglu ? (N + 31) / 32 * 32 : (N + 7) / 8 * 8;       // mostly a legal K for the next phase
            else if (swiglu && rnd(0, 7)) N = (N + 31) / 32 * 32;
            const void** q = ptrs + 6 * i;
            q[0] = i ? ptrs[6 * i - 1] : (const void*)0x10000; q[1] = (const void*)(uintptr_t)(0x100000 * (i + 1));
            q[2] = (!swiglu && rnd(0, 1)) ? (const void*)0x2000 : nullptr; q[3] = norm ? (const void*)0x3000 : nullptr;
            q[4] = (!swiglu && rnd(0, 1)) ? (const void*)(uintptr_t)(0x20000 * (i + 1)) : nullptr; q[5] = (const void*)(uintptr_t)(0x20000 * (i + 1));
            dims[4 * i] = N; dims[4 * i + 1] = K; dims[4 * i + 2] = K + 8 * rnd(0, 1); dims[4 * i + 3] = swiglu ? 3 : rnd(0, 2);
            K = swiglu ? N / 2 : N;
        }
        const bool knobs = rnd(0, 3) == 0;                                     // the BAGEL_ENGINE_* defaults, or anything
        EngGeometry g;
        const int rc = eng_geometry(ptrs, dims, nph, pick(wgs), knobs ? rnd(-1, 10) : ENG_MAX_SLOTS, knobs ? rnd(0, 9) : 8, knobs ? rnd(0, 3) : 2,
                                    knobs ? rnd(0, 5) : 2, &g);
        if (rc != 0) continue;
        ++accepted;
        CHECK(g.xs_bytes + g.nslot * g.slot_bytes + ENG_SYNC_BYTES <= ENG_LDS_MAX, "engine: %d + %d x %d bytes of LDS", g.xs_bytes, g.nslot, g.slot_bytes);
        CHECK(g.nloaders >= 1 && g.nloaders < g.waves && g.waves <= 8 && g.nslot % g.nloaders == 0 && g.nslot <= ENG_MAX_SLOTS, "engine: %d slots, %d loaders, %d waves",
              g.nslot, g.nloaders, g.waves);
        CHECK(g.depth >= 1 && g.depth * (g.slot_bytes / 1024) <= 63 && g.depth < g.nslot / g.nloaders, "engine: depth %d, %d-byte slots", g.depth, g.slot_bytes);
        for (int i = 0; i < nph; ++i) {
            const int unit = g.kind[i] == 2 ? g.gq[i] : g.ngr[i];
            CHECK(2 * unit * 1024 <= g.slot_bytes && 64L * 8 * g.ngr[i] >= dims[4 * i + 1] && 4 * g.gq[i] >= g.ngr[i], "engine: phase %d units", i);
        }
    }
    return accepted;
}

int main() {
    fuzz_attn();
    const long npq = fuzz_pq(), nmb = fuzz_mb(), neng = fuzz_engine();
    CHECK(neng >= 2000, "engine: only %ld of 20000 random chains were accepted: the fuzz does not reach the geometry", neng);
    printf("host_plan_fuzz: 2005 attention plans, %ld K-split points, %ld served gemv_mb geometries, %ld accepted engine chains: ok\n", npq, nmb, neng);
    return 0;
}
