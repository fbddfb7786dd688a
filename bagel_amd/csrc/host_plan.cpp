// Host-side launch planning (see host_plan.h): plain C++17, no HIP.  Every function here is pure -- arguments in, a schedule or a refusal out;
// environment knobs and device queries stay with the launchers, which pass their values in.
#include "host_plan.h"
#include <algorithm>
#include <vector>

// ---------------------------------------------------------------------------------------------------------
// Planner of the persistent attention kernel (attention2.hip).  Layout of the plan buffer (int32):
//   [0] n_workers  [1] n_items  [2] n_comb  [3] n_slots  [4] offset of the item table  [5] offset of the combine table
//   [6] makespan (tile steps of the busiest worker)  [7] total tile steps
//   [8 .. 8 + n_workers]  worker_off      then (16-int aligned) items[n_items][16], comb[n_comb][8]
// Worker w is assumed to run on XCD w % 8 (the hardware deals workgroup ids round-robin; an assumption for speed only).
// ---------------------------------------------------------------------------------------------------------
namespace {
struct PItem { AttnItem it; int cost; };
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
}

extern "C" int bagel_attn_plan(const int32_t* q_start, const int32_t* q_len, const int32_t* ctx_start, const int32_t* ctx_len,
                               const int32_t* vt_new_col, const int32_t* vt_ctx_col, int32_t batch, int32_t nq, int32_t nkv,
                               int32_t causal, int32_t n_workers, int32_t split_min_tiles, int32_t* plan, int64_t plan_ints) {
    BAGEL_REQUIRE(q_start && q_len && vt_new_col && plan, "attn_plan: null pointer");
    BAGEL_REQUIRE(nq > 0 && nkv > 0 && nq % nkv == 0, "attn_plan: bad head counts %d/%d", nq, nkv);
    BAGEL_REQUIRE(n_workers > 0 && n_workers % 8 == 0, "attn_plan: the worker count must be a multiple of the 8 XCDs");
    const int G = nq / nkv, wpx = n_workers / 8;
    if (split_min_tiles <= 0) split_min_tiles = 16;
    // ---- items of every (sample, KV head) pair, query tiles ascending ----
    std::vector<std::vector<PItem>> pairs;
    for (int b = 0; b < batch; ++b) {
        const int Lq = q_len[b], C = ctx_len ? ctx_len[b] : 0;
        if (Lq <= 0) continue;
        const int nt_ctx = cdiv(C, 64);
        const int nqt = cdiv(Lq, 256);
        for (int g = 0; g < nkv; ++g) {
            std::vector<PItem> v;
            for (int qt = 0; qt < nqt; ++qt) {
                const int nrows = std::min(256, Lq - 256 * qt);
                const int vis = causal ? std::min(Lq, 256 * qt + nrows) : Lq;        // new-segment keys any row of the tile may see
                const int T = nt_ctx + cdiv(vis, 64);
                const bool hpw = nrows <= 32 && G <= 8 && G > 1;
                AttnItem it = {};
                it.q_row0 = q_start[b] + 256 * qt; it.nrows = nrows; it.g = g;
                it.flags = (hpw ? ATTN2_HPW : 0) | (causal ? ATTN2_CAUSAL : 0) | (G << 8);
                it.q_rel0 = 256 * qt; it.kn_row0 = q_start[b]; it.l_new = Lq;
                it.kc_row0 = (C > 0 && ctx_start) ? ctx_start[b] : 0; it.l_ctx = C;
                it.vtn_col0 = vt_new_col[b]; it.vtc_col0 = (C > 0 && vt_ctx_col) ? vt_ctx_col[b] : 0;
                it.t0 = 0; it.t1 = T; it.part = -1;
                if (hpw) { it.h = g * G; v.push_back({it, T}); }
                else for (int j = 0; j < G; ++j) { it.h = g * G + j; v.push_back({it, T}); }
            }
            pairs.push_back(std::move(v));
        }
    }
    // ---- virtual pairs: when the pairs do not fill the 8 XCDs evenly, every pair is dealt into interleaved sets of items ----
    const int npairs = (int)pairs.size();
    std::vector<std::vector<PItem>> vps;
    if (npairs > 0) {
        int gcd8 = 8;
        while (npairs % gcd8) gcd8 >>= 1;
        const int qsplit = 8 / gcd8;
        for (auto& pr : pairs)
            for (int s = 0; s < qsplit; ++s) {
                std::vector<PItem> v;
                for (size_t j = s; j < pr.size(); j += qsplit) v.push_back(pr[j]);
                if (!v.empty()) vps.push_back(std::move(v));
            }
    }
    // ---- virtual pairs -> XCDs: heaviest first onto the least loaded XCD ----
    std::vector<long> vcost(vps.size(), 0);
    for (size_t i = 0; i < vps.size(); ++i) for (auto& x : vps[i]) vcost[i] += x.cost;
    std::vector<int> order(vps.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return vcost[a] > vcost[b2]; });
    std::vector<std::vector<int>> xcd_vps(8);
    long xload[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i : order) {
        int best = 0;
        for (int x = 1; x < 8; ++x) if (xload[x] < xload[best]) best = x;
        xcd_vps[best].push_back(i);
        xload[best] += vcost[i];
    }
    // ---- inside an XCD: longest-processing-time dealing of its item stream (virtual pair after virtual pair, heavy items first inside
    //      one) onto its `wpx` workers -- every item goes to the least loaded worker, which for equal costs is plain round-robin: the 32
    //      workers then sit on the same (sample, KV head) pair at the same time.  An item that would push its worker more than `slack`
    //      tile steps past the XCD's mean load is held back; the held-back items are cut along the key axis into contiguous tile ranges
    //      that fill the workers up to the mean (stream-K over the leftovers, chunks of >= min_chunk tiles), each range a sub-item
    //      that writes partials. ----
    std::vector<std::vector<AttnItem>> wl(n_workers);
    std::vector<long> wload(n_workers, 0);
    std::vector<AttnComb> combs;
    int n_slots = 0;
    const int min_chunk = std::max(split_min_tiles / 2, 1);
    for (int x = 0; x < 8; ++x) {
        std::vector<PItem> stream;
        for (int i : xcd_vps[x]) {
            std::vector<PItem> v = vps[i];
            std::stable_sort(v.begin(), v.end(), [](const PItem& a, const PItem& b2) { return a.cost > b2.cost; });
            stream.insert(stream.end(), v.begin(), v.end());
        }
        if (stream.empty()) continue;
        long tot = 0;
        for (auto& pi : stream) tot += pi.cost;
        const long mean = (tot + wpx - 1) / wpx;
        const long slack = 2;
        auto least = [&]() { int best = x; for (int j = 1; j < wpx; ++j) if (wload[j * 8 + x] < wload[best]) best = j * 8 + x; return best; };
        std::vector<PItem> held;
        for (auto& pi : stream) {
            const int w = least();
            const bool splittable = pi.cost >= split_min_tiles && pi.cost >= 2 * min_chunk;
            if (wload[w] + pi.cost > mean + slack && splittable) { held.push_back(pi); continue; }
            wl[w].push_back(pi.it);
            wload[w] += pi.cost;
        }
        // the held-back items as one stream of tiles: every cut gives the currently least loaded worker what it lacks to the mean
        for (auto& pi : held) {
            const int T = pi.it.t1 - pi.it.t0;
            std::vector<std::pair<int, int>> cuts;      // (worker, tiles)
            int left = T;
            while (left > 0) {
                const int w = least();
                long want = mean - wload[w];
                if (want < min_chunk) want = min_chunk;
                int n = (int)std::min<long>(want, left);
                if (left - n < min_chunk) n = left;                     // no crumbs
                cuts.push_back({w, n});
                wload[w] += n;
                left -= n;
            }
            if (cuts.size() == 1) { wl[cuts[0].first].push_back(pi.it); continue; }
            AttnComb c = {pi.it.q_row0, pi.it.nrows, pi.it.h, pi.it.flags, n_slots, (int)cuts.size(), 0, 0};
            combs.push_back(c);
            int at = pi.it.t0;
            for (auto& cw : cuts) {
                AttnItem sub = pi.it;
                sub.t0 = at; sub.t1 = at + cw.second; at += cw.second;
                sub.flags |= ATTN2_PARTIAL;
                sub.part = n_slots++;
                wl[cw.first].push_back(sub);
            }
        }
    }
    int n_items = 0;
    long total = 0, makespan = 0;
    for (int w = 0; w < n_workers; ++w) { n_items += (int)wl[w].size(); total += wload[w]; makespan = std::max(makespan, wload[w]); }
    const int off_items = ((8 + n_workers + 1) + 15) / 16 * 16;
    const int off_comb = off_items + 16 * n_items;
    const long need = (long)off_comb + 8L * (long)combs.size();
    BAGEL_REQUIRE(need <= plan_ints, "attn_plan: the plan needs %ld ints, the buffer holds %ld", need, (long)plan_ints);
    plan[0] = n_workers; plan[1] = n_items; plan[2] = (int)combs.size(); plan[3] = n_slots; plan[4] = off_items; plan[5] = off_comb;
    plan[6] = (int)makespan; plan[7] = (int)std::min<long>(total, 0x7fffffff);
    int at = 0;
    AttnItem* items = (AttnItem*)(plan + off_items);
    for (int w = 0; w < n_workers; ++w) {
        plan[8 + w] = at;
        for (auto& it : wl[w]) items[at++] = it;
    }
    plan[8 + n_workers] = at;
    for (int i = 8 + n_workers + 1; i < off_items; ++i) plan[i] = 0;
    AttnComb* cb = (AttnComb*)(plan + off_comb);
    for (size_t i = 0; i < combs.size(); ++i) cb[i] = combs[i];
    return BAGEL_OK;
}

// How a tile count that leaves the last round of the persistent kernel nearly empty is scheduled (LLM prefill of the understanding
// request: M = 4936 -> 20 row tiles; o / down have 280 tiles = 1.09 rounds of 256 CUs, qkv 360 = 1.41): the FULL rounds run as they
// are, the leftover tiles are cut along K into `ksplit` parts each so that they fill the chip once more with work items 1 / ksplit as
// long, and a small pass adds the parts up and applies the epilogue.  Returns the split (1 = do not split).
// policy: 0 = the round-3 rule (fill the chip ONCE with the leftovers), 1 = the round-5 cost model; force: experiment, this many parts for every launch with leftovers
int pq_leftover_split(int nblk, int wgs, int nk, size_t ws_bytes, int policy, int force, int* n_full_out) {
    const int n_full = nblk / wgs * wgs, rest = nblk - n_full;
    *n_full_out = n_full;
    if (rest == 0) return 1;
    if (force > 1) {
        int sf = force;
        if (sf > nk / 4) sf = nk / 4;
        while (sf > 1 && (size_t)rest * sf * (32 * 512 * 16) > ws_bytes) --sf;
        return sf < 2 ? 1 : sf;
    }
    if (policy == 0) {
        if (2 * rest > wgs + wgs / 4) return 1;                                // the last round is > 5/8 full anyway
        if (n_full == 0 && (2 * rest > wgs || nk < 16)) return 1;              // a single round: split only when it fills less than half the chip
        int s = wgs / rest;                                                    // parts per leftover tile: fill the chip once
        if (s > nk / 4) s = nk / 4;                                            // a part keeps >= 4 k-tiles (prologue + steady state)
        while (s > 1 && (size_t)rest * s * (32 * 512 * 16) > ws_bytes) --s;     // 256 KB of fp32 per part
        return s < 2 ? 1 : s;
    }
    // Round 5: the parts of the leftover tiles may take SEVERAL passes over the chip (rest * s > wgs), priced with a small model calibrated on the bench's own
    // launches: a 64-deep k-tile step of a 256 x 256 tile takes 1.52 us (gate+up at M = 32 768: 8.9 TFLOP in 6.32 ms = 4 144 steps), an item pays ~6 us of
    // pipeline fill + epilogue, a part costs 512 KB of fp32 partial traffic (written here, read by the reduce pass: ~0.13 us when the chip shares it) and the
    // reduce pass one more launch.  Un-split, the leftovers cost one whole tile time with (wgs - rest) CUs idle.  Example: the 3-stream edit forward has
    // 672 o / down tiles = 2.63 rounds; o (K = 3 584) is left alone (a 3-way split costs 137 us against 90), down (K = 18 944) is cut three ways: two passes of
    // third-length items = 380 us against 455.
    const double t_step = 1.52, t_item = 6.0, t_part = 0.13, t_reduce = 6.0;
    const double whole = nk * t_step + t_item;
    if (n_full == 0 && nk < 16) return 1;
    int best = 1;
    double best_cost = whole * 0.85;                                           // a split has to win 15 % of the leftover round to be worth a second launch
    for (int sp = 2; sp <= nk / 4 && sp <= 16; ++sp) {
        if ((size_t)rest * sp * (32 * 512 * 16) > ws_bytes) break;
        const int passes = (rest * sp + wgs - 1) / wgs;
        const double cost = passes * ((double)nk / sp * t_step + t_item) + rest * sp * t_part + t_reduce;
        // several passes (rest * sp > wgs) have to win a quarter of the round, not 15 %: measured on the edit request, the modelled 16 % of the three-way split of
        // its `down` leftovers (160 tiles) came out as +1 % of the request (profiles/r05_gemm_split_policy.log)
        if (cost < (passes > 1 ? whole * 0.75 : best_cost)) { best_cost = cost; best = sp; }
    }
    return best;
}

extern "C" int bagel_gemm_leftover_split(int32_t nblk, int32_t wgs, int32_t nk, int64_t ws_bytes, int32_t policy, int32_t force, int32_t* n_full,
                                         int32_t* ksplit) {
    BAGEL_REQUIRE(n_full && ksplit, "gemm_leftover_split: null pointer");
    BAGEL_REQUIRE(nblk >= 0 && wgs >= 1 && nk >= 0 && ws_bytes >= 0, "gemm_leftover_split: bad argument");
    int nf = 0;
    *ksplit = pq_leftover_split(nblk, wgs, nk, (size_t)ws_bytes, policy, force, &nf);
    *n_full = nf;
    return BAGEL_OK;
}

// Geometry of gemv_mb.hip.  Instantiations: NS = 4 (short rows, K <= 1024: the tiny test models), 10, 14 (K = 3584 in one slice: 14 steps per wave at the 7B
// hidden size), 19.  The launch is PERSISTENT: one workgroup per CU (its ~170 registers x 8 waves leave no room for a second one), each
// taking an even share of the column blocks of its K slice, so the activation prologue is paid once per workgroup and launch.
// Rows too long for one slice (nsteps > 8 x 19) are cut over KS workgroups; KS and the workgroups per slice are chosen together so that
// the blocks divide evenly and the whole chip is used: the 7B down projection (592 steps, 224 blocks, 256 CUs) runs as 8 slices x 32
// workgroups x 7 blocks x 10 steps per wave -- 4 slices x 64 workgroups would leave 3 or 4 blocks per workgroup (makespan 4 of 3.5).
static const int MB_NS[] = {4, 10, 14, 19};

// Two request blocks (17..32 rows) keep 2 x NS activation fragments per wave: NS = 19 does not fit the register file beside them, so the longest
// one-slice row is 8 x 14 steps (K = 3584, the 7B hidden size) and longer rows take more, shorter slices.
static int mb_max_ns(int MB) { return MB > 1 ? 14 : 19; }

static int mb_ns_for(int per, int MB = 1) {
    for (int ns : MB_NS)
        if (per <= ns && ns <= mb_max_ns(MB)) return ns;
    return 0;
}

void mb_geometry(int N, int K, int wgs, int MB, int* per, int* KS, int* gx_out) {
    const int nsteps = K / 32, nblk = N / 16;
    const int NSM = mb_max_ns(MB);
    if (nsteps <= 8 * NSM) {                           // one slice: the fused norm / SwiGLU need the whole row in one workgroup
        *KS = 1;
        *per = (nsteps + 7) / 8;
        *gx_out = wgs < nblk ? wgs : nblk;
        return;
    }
    const int ks_min = (nsteps + 8 * NSM - 1) / (8 * NSM);
    int best_ks = ks_min, best_gx = 1;
    double best_cost = 1e30;
    for (int ks = ks_min; ks <= 4 * ks_min && ks <= wgs; ++ks) {
        const int pw = (nsteps + 8 * ks - 1) / (8 * ks);
        const int ns = mb_ns_for(pw, MB);
        if (ns == 0 || nsteps < ns) continue;
        int gx = wgs / ks;
        if (gx < 1) gx = 1;
        if (gx > nblk) gx = nblk;
        const int blocks = (nblk + gx - 1) / gx;       // of the busiest workgroup
        // time ~ the busiest workgroup's stream (blocks x fragments it LOADS, live or not) + a fixed cost per slice of slab traffic
        const double cost = (double)blocks * ns * (1.0 + 0.02 * ks);
        if (cost < best_cost) { best_cost = cost; best_ks = ks; best_gx = gx; }
    }
    *KS = best_ks;
    *per = (nsteps + 8 * best_ks - 1) / (8 * best_ks);
    *gx_out = best_gx;
}

int mb_plan(int M, int N, int K, int epilogue, bool has_norm, int wgs, MbGeometry* g) {
    BAGEL_REQUIRE(M >= 1 && M <= 32, "gemv_mb: M=%d not in [1,32]", M);
    BAGEL_REQUIRE(K > 0 && (K % 32) == 0, "gemv_mb: K %% 32 == 0 and 16-byte rows required");
    BAGEL_REQUIRE(epilogue >= 0 && epilogue <= 3, "gemv_mb: unknown epilogue %d", epilogue);
    const bool sw = epilogue == BAGEL_EPI_SWIGLU16;
    BAGEL_REQUIRE(N > 0 && N % (sw ? 32 : 16) == 0, "gemv_mb: N %% 16 (SwiGLU: N %% 32, no bias/residual)");
    BAGEL_REQUIRE(wgs >= 1, "gemv_mb: %d workgroups", wgs);
    const int MB = M > 16 ? 2 : 1;                                  // request blocks of 16 rows that share every weight fragment
    mb_geometry(N, K, wgs, MB, &g->per, &g->KS, &g->gx);
    g->NS = mb_ns_for(g->per, MB);                                  // the instantiation that runs; its fragments must fit the row
    if (g->NS == 0 || K / 32 < g->NS) return bagel_set_error(BAGEL_ERR_UNSUPPORTED, "gemv_mb: K=%d (%d steps per wave) has no instantiation", K, g->per);
    if (g->KS > 1 && (has_norm || sw)) return bagel_set_error(BAGEL_ERR_UNSUPPORTED, "gemv_mb: fused RMSNorm / SwiGLU need the whole row in one slice (K=%d)", K);
    if (sw && g->gx > N / 32) g->gx = N / 32;                       // units are gate/up PAIRS of blocks
    return BAGEL_OK;
}

extern "C" int bagel_gemv_mb_geometry(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t has_norm, int32_t workgroups, int32_t* per,
                                      int32_t* ks, int32_t* gx) {
    BAGEL_REQUIRE(per && ks && gx, "gemv_mb_geometry: null pointer");
    MbGeometry g;
    if (int rc = mb_plan(M, N, K, epilogue, has_norm != 0, workgroups, &g)) return rc;
    *per = g.per; *ks = g.KS; *gx = g.gx;
    return BAGEL_OK;
}

extern "C" int bagel_gemv_mb_workspace_bytes(int32_t N, int32_t K, int64_t* bytes) {
    BAGEL_REQUIRE(bytes && N > 0 && K > 0 && (K % 32) == 0 && (N % 16) == 0, "gemv_mb_workspace_bytes: bad argument");
    // the slice count depends on the device's CU count and on the row count (17..32 rows: slices of at most 8 x 14 steps, slabs of 32 rows): an upper
    // bound that holds for every geometry the launcher may pick (4 x the minimum slice count of the 32-row form, 32-row slabs)
    const int nsteps = K / 32;
    const int ks_min = (nsteps + 8 * 14 - 1) / (8 * 14);
    *bytes = nsteps <= 8 * 14 ? 0 : (int64_t)4 * ks_min * 32 * N * 4;
    return BAGEL_OK;
}

// Geometry of gemv_mb_w4.hip.  A row of K / 128 k-steps is G = ceil(steps / 4) scale groups; a wave holds the activation fragments of gpw = 1 or 2 groups
// (instantiations NS = 4, 8 k-steps: 8 VGPRs per step and request block), so one workgroup covers up to 16 groups (K <= 8192: every K = 3584 projection of the 7B
// model runs as 7 live waves x 1 group).  Longer rows are cut into KS slices of gps = ceil(G / KS) groups; as for gemv_mb, KS is chosen together with the
// workgroups per slice by the busiest workgroup's stream: the 7B down projection (148 steps = 37 groups, 224 blocks, 256 CUs) runs as 5 slices (8, 8, 8, 8, 5
// groups) x 51 workgroups x 4-5 blocks x 4 steps per wave.
static const int MBW4_MAX_GPW = 2;

static int mbw4_ks_min(int G) { return (G + 8 * MBW4_MAX_GPW - 1) / (8 * MBW4_MAX_GPW); }

int mbw4_plan(int M, int N, int K, int epilogue, int wgs, MbW4Geometry* g) {
    BAGEL_REQUIRE(g, "gemv_mb_w4: null geometry");
    BAGEL_REQUIRE(M >= 1 && M <= 32, "gemv_mb_w4: M=%d not in [1,32]", M);
    BAGEL_REQUIRE(K > 0 && (K % 128) == 0, "gemv_mb_w4: K=%d must be a multiple of 128", K);
    BAGEL_REQUIRE(epilogue == BAGEL_EPI_NONE || epilogue == BAGEL_EPI_SWIGLU16, "gemv_mb_w4: epilogue %d not in {none, swiglu16}", epilogue);
    const bool sw = epilogue == BAGEL_EPI_SWIGLU16;
    BAGEL_REQUIRE(N > 0 && N % (sw ? 32 : 16) == 0, "gemv_mb_w4: N=%d must be a multiple of 16 (SwiGLU: 32)", N);
    BAGEL_REQUIRE(wgs >= 1, "gemv_mb_w4: %d workgroups", wgs);
    const int nsteps = K / 128, G = (nsteps + 3) / 4;
    const int nunits = N / (sw ? 32 : 16);                          // what the workgroups of a slice share out: blocks (SwiGLU: gate/up pairs of blocks)
    MbW4Geometry o;
    o.MB = M > 16 ? 2 : 1;
    if (G <= 8 * MBW4_MAX_GPW) {
        o.KS = 1; o.gps = G; o.gpw = (G + 7) / 8;
        o.gx = wgs < nunits ? wgs : nunits;
    } else {
        const int ks_min = mbw4_ks_min(G);
        double best = 1e30;
        o.KS = ks_min; o.gps = (G + ks_min - 1) / ks_min; o.gx = 1;
        for (int ks = ks_min; ks <= 4 * ks_min; ++ks) {
            const int gps = (G + ks - 1) / ks;
            if ((long)(ks - 1) * gps >= G) continue;                // no empty slice
            const int gpw = (gps + 7) / 8;
            int gx = wgs / ks;
            gx = gx < 1 ? 1 : (gx > nunits ? nunits : gx);
            const int units = (nunits + gx - 1) / gx;               // of the busiest workgroup
            const double cost = (double)units * gpw * (1.0 + 0.02 * ks);
            if (cost < best) { best = cost; o.KS = ks; o.gps = gps; o.gx = gx; }
        }
        o.gpw = (o.gps + 7) / 8;
    }
    o.NS = 4 * o.gpw;
    *g = o;
    return BAGEL_OK;
}

extern "C" int bagel_gemv_mb_w4_geometry(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t workgroups, int32_t* per, int32_t* slice_steps,
                                         int32_t* ks, int32_t* gx) {
    BAGEL_REQUIRE(per && slice_steps && ks && gx, "gemv_mb_w4_geometry: null pointer");
    MbW4Geometry g;
    if (int rc = mbw4_plan(M, N, K, epilogue, workgroups, &g)) return rc;
    *per = g.NS; *slice_steps = 4 * g.gps; *ks = g.KS; *gx = g.gx;
    return BAGEL_OK;
}

extern "C" int bagel_gemv_mb_w4_workspace_bytes(int32_t N, int32_t K, int64_t* bytes) {
    BAGEL_REQUIRE(bytes && N > 0 && K > 0 && (K % 128) == 0 && (N % 16) == 0, "gemv_mb_w4_workspace_bytes: bad argument");
    // an upper bound for every M and workgroup count: the planner tries at most 4 x the minimum slice count, slabs have at most 32 rows
    const int G = (K / 128 + 3) / 4;
    *bytes = G <= 8 * MBW4_MAX_GPW ? 0 : (int64_t)4 * mbw4_ks_min(G) * 32 * N * 4;
    return BAGEL_OK;
}

// Geometry of gemv_mb_nf4.hip.  A row is G = K / 128 k-groups (64 code bytes and two absmax blocks per weight row); a wave holds the activation fragments of
// gpw <= 4 groups (instantiations GP = 1, 2, 4: 16 VGPRs per group and request block), so one workgroup covers up to 32 groups (K <= 4096: every K = 3584
// projection of the 7B model runs as 7 live waves x 4 groups).  Longer rows are cut into KS slices of gps = ceil(G / KS) groups; as for gemv_mb, KS is chosen
// together with the workgroups per slice by the busiest workgroup's stream (units x the fragments a wave of it holds): the 7B down projection (148 groups,
// 224 blocks, 256 CUs) runs as 10 slices (15 groups, the last 13) x 25 workgroups x 8-9 blocks x 2 groups per wave.
static const int MBNF4_MAX_GPW = 4;

static int mbnf4_ks_min(int G) { return (G + 8 * MBNF4_MAX_GPW - 1) / (8 * MBNF4_MAX_GPW); }
static int mbnf4_gp_for(int gpw) { return gpw <= 1 ? 1 : (gpw <= 2 ? 2 : 4); }

int mbnf4_plan(int M, int N, int K, int epilogue, int wgs, MbNf4Geometry* g) {
    BAGEL_REQUIRE(g, "gemv_mb_nf4: null geometry");
    BAGEL_REQUIRE(M >= 1 && M <= 32, "gemv_mb_nf4: M=%d not in [1,32]", M);
    BAGEL_REQUIRE(K > 0 && (K % 128) == 0, "gemv_mb_nf4: K=%d must be a multiple of 128", K);
    BAGEL_REQUIRE(epilogue == BAGEL_EPI_NONE || epilogue == BAGEL_EPI_SWIGLU16, "gemv_mb_nf4: epilogue %d not in {none, swiglu16}", epilogue);
    const bool sw = epilogue == BAGEL_EPI_SWIGLU16;
    BAGEL_REQUIRE(N > 0 && N % (sw ? 32 : 16) == 0, "gemv_mb_nf4: N=%d must be a multiple of 16 (SwiGLU: 32)", N);
    BAGEL_REQUIRE(wgs >= 1, "gemv_mb_nf4: %d workgroups", wgs);
    const int G = K / 128;
    const int nunits = N / (sw ? 32 : 16);                          // what the workgroups of a slice share out: blocks (SwiGLU: gate/up pairs of blocks)
    MbNf4Geometry o;
    o.MB = M > 16 ? 2 : 1;
    if (G <= 8 * MBNF4_MAX_GPW) {
        o.KS = 1; o.gps = G;
        o.gx = wgs < nunits ? wgs : nunits;
    } else {
        const int ks_min = mbnf4_ks_min(G);
        double best = 1e30;
        o.KS = ks_min; o.gps = (G + ks_min - 1) / ks_min; o.gx = 1;
        for (int ks = ks_min; ks <= 4 * ks_min; ++ks) {
            const int gps = (G + ks - 1) / ks;
            if ((long)(ks - 1) * gps >= G) continue;                // no empty slice
            int gx = wgs / ks;
            gx = gx < 1 ? 1 : (gx > nunits ? nunits : gx);
            const int units = (nunits + gx - 1) / gx;               // of the busiest workgroup
            const double cost = (double)units * ((gps + 7) / 8) * (1.0 + 0.02 * ks);
            if (cost < best) { best = cost; o.KS = ks; o.gps = gps; o.gx = gx; }
        }
    }
    o.gpw = (o.gps + 7) / 8;
    o.GP = mbnf4_gp_for(o.gpw);
    *g = o;
    return BAGEL_OK;
}

extern "C" int bagel_gemv_mb_nf4_geometry(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t workgroups, int32_t* per, int32_t* slice_groups,
                                          int32_t* ks, int32_t* gx) {
    BAGEL_REQUIRE(per && slice_groups && ks && gx, "gemv_mb_nf4_geometry: null pointer");
    MbNf4Geometry g;
    if (int rc = mbnf4_plan(M, N, K, epilogue, workgroups, &g)) return rc;
    *per = g.gpw; *slice_groups = g.gps; *ks = g.KS; *gx = g.gx;
    return BAGEL_OK;
}

extern "C" int bagel_gemv_mb_nf4_workspace_bytes(int32_t N, int32_t K, int64_t* bytes) {
    BAGEL_REQUIRE(bytes && N > 0 && K > 0 && (K % 128) == 0 && (N % 16) == 0, "gemv_mb_nf4_workspace_bytes: bad argument");
    // an upper bound for every M and workgroup count: the planner tries at most 4 x the minimum slice count, slabs have at most 32 rows
    const int G = K / 128;
    *bytes = G <= 8 * MBNF4_MAX_GPW ? 0 : (int64_t)4 * mbnf4_ks_min(G) * 32 * N * 4;
    return BAGEL_OK;
}

// Per-phase validation and LDS-ring geometry of the decode engine (engine.hip).
int eng_geometry(const void* const* ptrs, const int64_t* dims, int n_phases, int n_wg, int want_slots, int waves, int loaders, int depth,
                 EngGeometry* out) {
    BAGEL_REQUIRE(ptrs && dims, "decode_engine: null pointer");
    BAGEL_REQUIRE(n_phases >= 1 && n_phases <= ENG_MAXPH, "decode_engine: 1..%d phases (got %d)", ENG_MAXPH, n_phases);
    int max_k = 0, slot = 0, prev_n = 0, prev_epi = 0;
    for (int i = 0; i < n_phases; ++i) {
        const void* const* q = ptrs + 6 * i;
        const int64_t* d = dims + 4 * i;
        const void *A = q[0], *W = q[1], *bias = q[2], *norm_w = q[3], *R = q[4], *C = q[5];
        const int N = (int)d[0], K = (int)d[1], epi = (int)d[3];
        const int64_t ldw = d[2];
        BAGEL_REQUIRE(A && W && C, "decode_engine: phase %d: null A / W / C", i);
        BAGEL_REQUIRE(K > 0 && (K % 8) == 0 && (ldw % 8) == 0, "decode_engine: phase %d: K / ldw must be multiples of 8", i);
        BAGEL_REQUIRE(N > 0 && (N % 2) == 0, "decode_engine: phase %d: N = %d must be even", i, N);
        BAGEL_REQUIRE(epi >= 0 && epi <= 3, "decode_engine: phase %d: unknown epilogue %d", i, epi);
        BAGEL_REQUIRE(epi != BAGEL_EPI_SWIGLU16 || ((N % 32) == 0 && !bias && !R), "decode_engine: phase %d: swiglu needs N %% 32 == 0, no bias / residual", i);
        BAGEL_REQUIRE((((uintptr_t)A | (uintptr_t)W | (uintptr_t)norm_w) & 15) == 0, "decode_engine: phase %d: A / W / norm_w must be 16-byte aligned", i);
        BAGEL_REQUIRE((((uintptr_t)C | (uintptr_t)R) & 3) == 0, "decode_engine: phase %d: C / R must be 4-byte aligned", i);
        BAGEL_REQUIRE(!norm_w || (K >> 3) <= 512, "decode_engine: phase %d: the fused RMSNorm serves K <= 4096", i);
        BAGEL_REQUIRE(i == 0 || A == ptrs[6 * i - 1], "decode_engine: phase %d must read the previous phase's output", i);
        BAGEL_REQUIRE(i == 0 || K == (prev_epi == BAGEL_EPI_SWIGLU16 ? prev_n / 2 : prev_n),
                      "decode_engine: phase %d: K = %d does not match the previous phase's output length", i, K);
        prev_n = N; prev_epi = epi;
        const int ngr = out->ngr[i] = (K / 8 + 63) / 64;
        // the split-K form of bagel_gemv_bf16 (launch_gemv_any): long un-normalised rows, few of them
        const int kind = out->kind[i] = (!norm_w && K >= 8192 && N / 2 <= 8192) ? 2 : 0;
        const int gq = out->gq[i] = (ngr + 3) / 4;
        const int unit_groups = kind == 2 ? gq : ngr;
        BAGEL_REQUIRE(2 * unit_groups <= 60, "decode_engine: phase %d: K = %d gives %d KB units (at most 60 LDS-DMA instructions in flight)", i, K, 2 * unit_groups);
        if (kind == 2) {
            const long max_pairs = ((long)N / 2 + n_wg - 1) / n_wg;
            BAGEL_REQUIRE(max_pairs <= ENG_MAX_DPAIRS, "decode_engine: phase %d: %ld split-K pairs per workgroup (at most %d)", i, max_pairs, ENG_MAX_DPAIRS);
        }
        if (2 * unit_groups * 1024 > slot) slot = 2 * unit_groups * 1024;
        if (K > max_k) max_k = K;
    }
    out->xs_bytes = (max_k * 2 + 1023) / 1024 * 1024;
    out->slot_bytes = slot;
    int nslot = (ENG_LDS_MAX - out->xs_bytes - ENG_SYNC_BYTES) / slot;
    if (nslot > want_slots) nslot = want_slots;
    if (nslot > ENG_MAX_SLOTS) nslot = ENG_MAX_SLOTS;
    if (waves < 2) waves = 2;
    if (waves > 8) waves = 8;
    int nl = loaders;
    if (nl < 1) nl = 1;
    if (nl > 2) nl = 2;
    if (nl >= waves) nl = waves - 1;
    nslot -= nslot % nl;                                       // every loader owns the slots of its units
    BAGEL_REQUIRE(nslot >= 2 * nl && nslot >= 3, "decode_engine: the LDS ring holds %d slots of %d bytes beside a %d-byte activation vector", nslot, slot, out->xs_bytes);
    out->nslot = nslot;
    out->nloaders = nl;
    out->waves = waves;
    out->n_wg = n_wg;
    // units one loader keeps unpublished: fewer than its own slots, and `depth` of the largest unit must stay countable (<= 63 DMA instructions)
    if (depth < 1) depth = 1;
    if (depth > nslot / nl - 1) depth = nslot / nl - 1;
    while (depth > 1 && depth * (slot / 1024) > 63) --depth;
    out->depth = depth;
    return BAGEL_OK;
}
