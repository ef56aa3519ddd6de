// Host check of csrc/vq_search_plan.h, the launch plans of the nearest-code search, on the CPU: the planner is swept over
// devices of 32 .. 304 compute units, row counts up to 2^31 - 1, every padded dim, residual stacks, both metrics, the flags and
// the environment switches, and every plan must be sound by its own arithmetic (the legs cover the rows once, every split owns
// a tile, whatever a leg indexes lies inside the workspace the sizers promise, every kernel is chosen only where it exists).
// The plans that tests/test_gpu_launch_plans.py and DESIGN.md document for a 256-CU device are pinned at the end.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "vq_search_plan.h"

using namespace vqi;

static int fails = 0;
static long long plans = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (fails++ < 20) {                  \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

static const long long kLds = 160 * 1024;

static Call make_call(int H, long long M, int K, int D, int Q, int metric, unsigned flags, bool sq_err, bool lse, unsigned bits) {
    Call c = {};
    c.H = H; c.M = M; c.K = K; c.D = D; c.Q = Q; c.metric = metric; c.flags = flags;
    c.workspace_bytes = padded_dim(D) ? workspace_bytes(H, M, Q) : wide_workspace_bytes(H, M, wide_plan(H, M > 0 ? M : 1, K, D));
    c.out = (bits & 7) != 1; c.idx = c.cb = c.packed = true;
    c.best = (bits & 8) != 0; c.sq_err = sq_err; c.lse = lse;
    c.screen = (bits & 16) != 0;
    const bool vec = (bits & 96) != 32 && D % 4 == 0;
    c.vec_x = c.vec_fin = c.vec_res = c.vec_wide = vec;
    return c;
}

// what every plan must satisfy, whatever the device
static void check_plan(const Call &c, const Device &dev, const Switches &sw, const CallPlan &pl) {
    ++plans;
    const int cus = dev.cus, H = c.H, DP = padded_dim(c.D);
    const bool per_head = (c.flags & VQ_F_SQERR_PER_HEAD) && c.sq_err;
    const bool simple = (c.flags & VQ_F_FORCE_SIMPLE) || DP == 0;
#define AT "cus %d mhz %d H %d M %lld K %d D %d Q %d metric %d flags %u sq %d lse %d"
#define ATV cus, dev.clock_mhz, H, c.M, c.K, c.D, c.Q, c.metric, c.flags, (int)c.sq_err, (int)c.lse
    CHECK(pl.nlegs >= 0 && pl.nlegs <= kMaxLegs && (pl.nlegs == 0) == (c.M == 0), AT ": %d legs", ATV, pl.nlegs);
    long long next = 0;
    for (int i = 0; i < pl.nlegs; ++i) {
        const Leg &g = pl.leg[i];
        const long long R = g.rows;
        CHECK(g.row_begin == next && R > 0, AT ": leg %d covers [%lld, +%lld) after %lld", ATV, i, g.row_begin, R, next);
        next = g.row_begin + R;
        CHECK(g.DP == DP, AT ": leg %d DP %d", ATV, i, g.DP);
        if (i == 1) CHECK(g.kind == kLegStaged ? g.accumulate : g.accumulate == c.sq_err, AT ": second leg accumulate %d", ATV, (int)g.accumulate);
        if (i == 0 && g.kind != kLegStaged) CHECK(!g.accumulate, AT ": first leg accumulates", ATV);
        const long long W = c.workspace_bytes;
        switch (g.kind) {
            case kLegFused: {
                const SearchChoice &ch = g.choice;
                const int ntiles = tiles_of(c.K, DP), nsub = ntiles * sub_tiles(DP);
                CHECK(!simple, AT ": fused leg on the scalar / wide path", ATV);
                if (c.sq_err)
                    CHECK(ch.kind != kResident && loss_partials_per_head(ch, R, H, cus) * H * c.Q <= ws_loss_floats(H, R, c.Q) &&
                              ws_core_bytes(H, R, c.Q) <= W,
                          AT ": leg %d loss partials outside the workspace", ATV, i);
                if (ch.kind == kResident) {
                    CHECK((DP == 32 || DP == 64 || DP == 128) && pl.nlegs == 1 && !sw.no_resident && c.Q == 1 && g.res_img_floats > 0 &&
                              g.res_nbuf >= 1 && (long long)resident_lds_bytes(g.res_img_floats, g.res_nbuf) <= kLds && ch.waves == 8,
                          AT ": resident kernel", ATV);
                } else {
                    CHECK(g.res_img_floats == 0, AT ": image without the resident kernel", ATV);
                }
                if (ch.kind == kPair)
                    CHECK(DP == 512 && c.Q <= kPairMaxStages && (c.Q == 1 || !sw.pair_no_multi) && !sw.single_wave_512 && ntiles >= 8 && ch.waves == 8,
                          AT ": wave pairs", ATV);
                if (ch.kind == kPersist)
                    CHECK(DP == 256 && ch.waves == 8 && nsub >= kPersistMinSub && nsub <= kPersistMaxSub && !sw.no_persist && c.Q == 1 &&
                              !(ch.train && sw.no_persist_train) && one_block_grid_x(R, 8) * H >= 2ll * cus && c.vec_x,
                          AT ": persistent kernel", ATV);
                if (ch.kind == kOneBlock) CHECK(ch.waves == 4 || (ch.waves == 8 && DP != 512), AT ": %d waves", ATV, ch.waves);
                if (ch.screened) {
                    CHECK(ch.kind == kPersist && !ch.train && c.metric == VQ_METRIC_EUCLID && !c.best && !sw.no_screen &&
                              (ch.cached ? screen_list_bytes(H, R) : screen_bytes(H, R, ntiles)) <= ws_keys_bytes(H, R) && ws_keys_bytes(H, R) <= W &&
                              scr_image_bytes(ntiles) < (1ll << 31) && (long long)H * R < (1ll << 31) && ch.cached == c.screen,
                          AT ": screened sweep", ATV);
                    CHECK(ch.stagger == !sw.no_stagger && ch.resolve_split == !sw.resolve_no_split, AT ": screened switches", ATV);
                } else {
                    CHECK(!ch.cached && !ch.stagger && !ch.resolve_split, AT ": screen fields without the screened sweep", ATV);
                }
                // (a stack's staged tail adds per-head sums of its own; a single stage has them on the fused path only)
                if (c.lse || (per_head && c.Q == 1)) CHECK(pl.nlegs == 1, AT ": lse / per-head sums cut in two", ATV);
                break;
            }
            case kLegStaged:
                CHECK(c.Q >= 2 && !sw.no_residual_tail && i == pl.nlegs - 1 && g.keys.mfma && !simple, AT ": staged tail", ATV);
                CHECK((long long)H * R * c.D * 4 <= residual_tail_room(H, c.M, c.Q) && ws_core_bytes(H, c.M, c.Q) + (long long)H * R * c.D * 4 <= W &&
                          ws_core_bytes(H, R, 1) <= ws_core_bytes(H, c.M, c.Q),
                      AT ": staged rows outside their room", ATV);
                [[fallthrough]];
            case kLegKeys: {
                const KeysPlan &k = g.keys;
                const int ntiles = tiles_of(c.K, DP);
                CHECK(k.mfma && DP != 0 && k.DP == DP && (g.kind == kLegStaged || c.Q == 1), AT ": keys leg", ATV);
                CHECK(k.splits >= 1 && k.splits <= ntiles && (long long)k.tiles_per_split * (k.splits - 1) < ntiles &&
                          (long long)k.tiles_per_split * k.splits >= ntiles,
                      AT ": %d splits of %d tiles over %d", ATV, k.splits, k.tiles_per_split, ntiles);
                CHECK(!g.planes || (long long)k.splits * H * R * 8 <= ws_keys_bytes(H, R), AT ": planes outside the key area", ATV);
                CHECK(ws_core_bytes(H, R, 1) <= W, AT ": keys + partials outside the workspace", ATV);
                CHECK(k.choice.kind == kOneBlock ? (k.choice.waves == k.waves && (k.waves == 4 || (k.waves == 8 && DP != 512)))
                                                 : (k.choice.kind == kPair && DP == 512 && k.tiles_per_split >= 8 && !sw.single_wave_512),
                      AT ": keys-mode kernel", ATV);
                break;
            }
            case kLegWideFused:
            case kLegWideKeys: {
                const WidePlan &w = g.kind == kLegWideFused ? g.wide : g.keys.wide;
                CHECK(DP == 0 && pl.nlegs == 1 && !(c.flags & VQ_F_FORCE_SIMPLE) && c.Q == 1, AT ": wide leg", ATV);
                CHECK(w.nd == (c.D + kWideSlice - 1) / kWideSlice && w.kc % 32 == 0 && w.kc > 0 && w.mc % kWideRows == 0 && w.mc > 0 &&
                          (long long)H * (w.mc / kWideRows) * kWideWaves * (w.kc / 32) * 256 * 4 <= w.acc_bytes &&
                          2 * ((long long)H * w.mc * 4) <= w.xn_bytes && wide_workspace_bytes(H, c.M, w) <= W,
                      AT ": wide plan", ATV);
                if (g.kind == kLegWideFused)
                    CHECK(!c.sq_err && c.out && c.vec_wide && round_up(c.K, kTileCodes) <= kWideCodes, AT ": fused wide rows", ATV);
                else
                    CHECK(!g.planes && !g.keys.mfma && g.keys.wide_rows, AT ": wide keys", ATV);
                break;
            }
            case kLegScalar:
                CHECK((c.flags & VQ_F_FORCE_SIMPLE) && pl.nlegs == 1 && c.Q == 1 && !g.planes && !g.keys.mfma && !g.keys.wide_rows, AT ": scalar leg", ATV);
                break;
            case kLegNoStack:
            case kLegNoPerHead:
                CHECK(simple && pl.nlegs == 1 && (g.kind == kLegNoStack ? c.Q != 1 : per_head), AT ": refusal %d", ATV, (int)g.kind);
                break;
        }
    }
    CHECK(next == c.M, AT ": legs end at row %lld", ATV, next);
    if (pl.nlegs == 2) {  // a cut is a whole number of rounds and of row blocks of every head (whole_rounds)
        const int rpw = fused_rows_per_wg(DP);
        const long long r0 = pl.leg[0].rows;
        CHECK(DP != 0 && r0 % rpw == 0 && (r0 / rpw * H) % cus == 0, AT ": cut at row %lld", ATV, r0);
        CHECK(pl.leg[0].kind == kLegFused || pl.leg[0].kind == kLegKeys, AT ": first leg kind %d", ATV, (int)pl.leg[0].kind);
        CHECK(c.Q == 1 ? pl.leg[1].kind == kLegKeys || pl.leg[1].kind == kLegFused : pl.leg[1].kind == kLegStaged, AT ": second leg kind %d", ATV,
              (int)pl.leg[1].kind);
    }
}

static bool same_shape(const CallPlan &a, const CallPlan &b) {
    if (a.nlegs != b.nlegs) return false;
    for (int i = 0; i < a.nlegs; ++i) {
        const Leg &x = a.leg[i], &y = b.leg[i];
        if (x.kind != y.kind || x.row_begin != y.row_begin || x.rows != y.rows || x.accumulate != y.accumulate || x.planes != y.planes) return false;
        if (x.kind == kLegFused && (x.choice.kind != y.choice.kind || x.choice.waves != y.choice.waves || x.choice.screened != y.choice.screened ||
                                    x.choice.cached != y.choice.cached || x.choice.train != y.choice.train))
            return false;
        if ((x.kind == kLegKeys || x.kind == kLegStaged) && (x.keys.splits != y.keys.splits || x.keys.waves != y.keys.waves ||
                                                              x.keys.tiles_per_split != y.keys.tiles_per_split || x.keys.choice.kind != y.keys.choice.kind))
            return false;
    }
    return true;
}

static Switches switch_set(int which) {  // 0: none; 1 .. 10: that switch alone
    Switches sw = {};
    bool *const f[] = {&sw.single_wave_512, &sw.no_persist, &sw.no_persist_train, &sw.no_screen, &sw.pair_no_multi,
                       &sw.no_resident,     &sw.no_residual_tail, &sw.no_stagger, &sw.resolve_no_split};
    if (which >= 1 && which <= 9) *f[which - 1] = true;
    if (which == 10) sw.res_skew = 3;
    return sw;
}

// the plan depends on a switch only as documented
static void check_switch(const Call &c, const Device &dev, int which, const CallPlan &base, const CallPlan &pl) {
    bool any[4] = {}, staged = false, stack_on_pairs = false;  // (any: kernels of fused legs and of keys-mode searches)
    for (int i = 0; i < pl.nlegs; ++i) {
        const Leg &g = pl.leg[i];
        if (g.kind == kLegFused) any[g.choice.kind] = true;
        if (g.kind == kLegFused && g.choice.kind == kPair && c.Q > 1) stack_on_pairs = true;
        if ((g.kind == kLegKeys || g.kind == kLegStaged) && g.keys.choice.kind == kPair) any[kPair] = true;
        staged |= g.kind == kLegStaged;
    }
    bool base_pair = false, base_stack_on_pairs = false, base_res = false, base_persist = false, base_screened = false, base_staged = false;
    for (int i = 0; i < base.nlegs; ++i) {
        const Leg &g = base.leg[i];
        base_pair |= (g.kind == kLegFused && g.choice.kind == kPair) || ((g.kind == kLegKeys || g.kind == kLegStaged) && g.keys.choice.kind == kPair);
        base_stack_on_pairs |= g.kind == kLegFused && g.choice.kind == kPair && c.Q > 1;
        base_res |= g.kind == kLegFused && g.choice.kind == kResident;
        base_persist |= g.kind == kLegFused && g.choice.kind == kPersist;
        base_screened |= g.kind == kLegFused && g.choice.screened;
        base_staged |= g.kind == kLegStaged;
    }
    const char *names[] = {"none", "VQ_SINGLE_WAVE_512", "VQ_NO_PERSIST", "VQ_NO_PERSIST_TRAIN", "VQ_NO_SCREEN", "VQ_PAIR_NO_MULTI",
                           "VQ_NO_RESIDENT", "VQ_NO_RESIDUAL_TAIL", "VQ_NO_STAGGER", "VQ_RESOLVE_NO_SPLIT", "VQ_RES_SKEW"};
    bool ok = true;
    switch (which) {
        case 1: ok = !any[kPair] && (base_pair || same_shape(base, pl)); break;
        case 2: ok = !any[kPersist] && (base_persist || same_shape(base, pl)); break;
        case 3: ok = base_persist || same_shape(base, pl); break;
        case 4: ok = base_screened || same_shape(base, pl); break;
        case 5: ok = !stack_on_pairs && (base_stack_on_pairs || same_shape(base, pl)); break;  // (fused residual launches only)
        case 6: ok = !any[kResident] && (base_res || same_shape(base, pl)); break;
        case 7: ok = !staged && (base_staged || same_shape(base, pl)); break;
        default: ok = same_shape(base, pl); break;  // (stagger / resolve split / skew are fields of the screened and resident launches only)
    }
    CHECK(ok, "cus %d H %d M %lld K %d D %d Q %d flags %u: plan under %s", dev.cus, c.H, c.M, c.K, c.D, c.Q, c.flags, names[which]);
}

static void sweep() {
    const int CUS[] = {32, 64, 104, 128, 256, 304}, MHZ[] = {1500, 2400}, HS[] = {1, 2, 6, 8}, KS[] = {1, 32, 33, 300, 1024, 4096, 8192, 65536};
    const long long MS[] = {0, 1, 31, 32, 33, 255, 256, 257, 8192, 36000, 65536, 70000, 131073, 2147483647ll};
    const int DS[] = {1, 32, 33, 64, 128, 200, 256, 257, 512, 513, 700, 2048}, QS[] = {1, 2, 4, 27};
    const unsigned FLAGS[] = {0, VQ_F_STE, VQ_F_FORCE_SIMPLE, VQ_F_FORCE_SPLIT, VQ_F_SQERR_PER_HEAD, VQ_F_STE | VQ_F_SQERR_PER_HEAD, VQ_F_X_F16, VQ_F_X_BF16};
    unsigned n = 0;  // (thins the product: the out / best / screen / alignment bits and the switch rotate with the point)
    for (int cus : CUS)
        for (int mhz : MHZ)
            for (int H : HS)
                for (long long M : MS)
                    for (int K : KS)
                        for (int D : DS)
                            for (int Q : QS)
                                for (int metric = 0; metric < 2; ++metric)
                                    for (unsigned flags : FLAGS) {
                                        if ((flags & (VQ_F_X_F16 | VQ_F_X_BF16)) && (Q != 1 || D > 512)) continue;  // (refused before the plan)
                                        const Device dev = {cus, mhz};
                                        for (int v = 0; v < 3; ++v) {  // no sums; squared-error sums; log-sum-exp
                                            const bool sq = v == 1, lse = v == 2;
                                            if (lse && (Q != 1 || D > 512 || flags != 0)) continue;
                                            if (sq && (flags & (VQ_F_X_F16 | VQ_F_X_BF16))) continue;
                                            if (!sq && (flags & VQ_F_SQERR_PER_HEAD)) continue;
                                            n = n * 1664525u + 1013904223u;
                                            const Call c = make_call(H, M, K, D, Q, metric, flags, sq, lse, n >> 8);
                                            const CallPlan base = plan_call(c, dev, switch_set(0));
                                            check_plan(c, dev, switch_set(0), base);
                                            const int which = 1 + (int)((n >> 20) % 10);
                                            const Switches sw = switch_set(which);
                                            const CallPlan pl = plan_call(c, dev, sw);
                                            check_plan(c, dev, sw, pl);
                                            check_switch(c, dev, which, base, pl);
                                        }
                                    }
}

// ---- the plans documented for a 256-CU device (2400 MHz) --------------------------------------------------------------------
static CallPlan plan256(int H, long long M, int K, int D, int metric, int Q = 1, bool train = false, bool per_head = false) {
    Call c = make_call(H, M, K, D, Q, metric, (train ? VQ_F_STE : 0u) | (per_head ? VQ_F_SQERR_PER_HEAD : 0u), train, false, 0);
    return plan_call(c, Device{256, 2400}, switch_set(0));
}
static void print_plan(const char *what, const CallPlan &pl) {
    std::printf("%s:", what);
    for (int i = 0; i < pl.nlegs; ++i) {
        const Leg &g = pl.leg[i];
        std::printf(" [leg %d kind %d rows %lld+%lld acc %d", i, (int)g.kind, g.row_begin, g.rows, (int)g.accumulate);
        if (g.kind == kLegFused) std::printf(" kernel %d waves %d screened %d train %d img %d x%d", (int)g.choice.kind, g.choice.waves, (int)g.choice.screened, (int)g.choice.train, g.res_img_floats, g.res_nbuf);
        if (g.kind == kLegKeys || g.kind == kLegStaged)
            std::printf(" kernel %d waves %d splits %d x %d tiles planes %d", (int)g.keys.choice.kind, g.keys.waves, g.keys.splits, g.keys.tiles_per_split, (int)g.planes);
        std::printf("]");
    }
    std::printf("\n");
}
#define PIN(cond) CHECK(cond, "documented plan at 256 CUs, line %d", __LINE__)
static bool fused_then_keys(const CallPlan &p, long long rows0, SearchKind k0, int splits1) {
    return p.nlegs == 2 && p.leg[0].kind == kLegFused && p.leg[0].rows == rows0 && p.leg[0].choice.kind == k0 && p.leg[1].kind == kLegKeys &&
           p.leg[1].keys.splits == splits1;
}
static bool one_keys(const CallPlan &p, int splits, SearchKind k) {
    return p.nlegs == 1 && p.leg[0].kind == kLegKeys && p.leg[0].keys.splits == splits && p.leg[0].keys.choice.kind == k;
}
static bool one_fused(const CallPlan &p, SearchKind k, int waves) {
    return p.nlegs == 1 && p.leg[0].kind == kLegFused && p.leg[0].choice.kind == k && p.leg[0].choice.waves == waves;
}
struct DocCase { int H; long long M; int K, D, metric; };
static const DocCase kCases[] = {  // tests/test_gpu_launch_plans.py CASES
    {1, 70000, 1024, 256, 0}, {1, 131073, 1024, 256, 0}, {1, 66000, 8192, 256, 0}, {1, 40000, 4096, 256, 1}, {1, 40000, 4096, 512, 0}, {1, 70000, 8192, 64, 0},
    {1, 200000, 1024, 64, 1}, {1, 150000, 4096, 128, 0}, {8, 10000, 8192, 64, 0}, {4, 20000, 2048, 256, 1}, {6, 9000, 1024, 512, 0}};
struct ResCase { long long M; int K, D, Q, H; };
static const ResCase kResCases[] = {  // test_residual_stacks_with_awkward_row_counts
    {70000, 1024, 256, 4, 1}, {80000, 256, 256, 3, 1}, {140000, 512, 200, 2, 1}, {65536, 1024, 256, 3, 1}, {66000, 2048, 256, 3, 1}, {36000, 1024, 128, 3, 2},
    {34000, 1024, 400, 2, 1}, {35001, 4096, 64, 2, 2}, {8192, 1024, 256, 8, 1}};
static void dump_documented() {
    char what[128];
    for (const DocCase &d : kCases)
        for (int train = 0; train < 2; ++train) {
            std::snprintf(what, sizeof(what), "(%d, %lld, %d, %d, %d) train %d", d.H, d.M, d.K, d.D, d.metric, train);
            print_plan(what, plan256(d.H, d.M, d.K, d.D, d.metric, 1, train));
        }
    for (const ResCase &d : kResCases)
        for (int train = 0; train < 2; ++train) {
            std::snprintf(what, sizeof(what), "residual (M %lld, K %d, D %d, Q %d, H %d) train %d", d.M, d.K, d.D, d.Q, d.H, train);
            print_plan(what, plan256(d.H, d.M, d.K, d.D, 0, d.Q, train));
        }
    const long long sq[][3] = {{128 * 256 + 37, 200, 64}, {337, 120, 100}, {66 * 128 + 37, 256, 512}, {255 * 256 + 37, 1024, 256}};  // _sq_err_cases at 256 CUs, H = 2
    for (const auto &q : sq)
        for (int ph = 0; ph < 2; ++ph) {
            std::snprintf(what, sizeof(what), "sq_err (2, %lld, %lld, %lld) per_head %d", q[0], q[1], q[2], ph);
            Call c = make_call(2, q[0], (int)q[1], (int)q[2], 1, 0, ph ? VQ_F_SQERR_PER_HEAD : 0u, true, false, 0);
            print_plan(what, plan_call(c, Device{256, 2400}, switch_set(0)));
        }
    print_plan("cfg2 (1, 262144, 1024, 256)", plan256(1, 262144, 1024, 256, 0));
    print_plan("resident (2, 1000000, 256, 64)", plan256(2, 1000000, 256, 64, 0));
}
static bool fused_then_staged(const CallPlan &p, long long rows0, long long rows1) {
    return p.nlegs == 2 && p.leg[0].kind == kLegFused && p.leg[0].rows == rows0 && p.leg[1].kind == kLegStaged && p.leg[1].rows == rows1 &&
           p.leg[1].accumulate && p.leg[1].keys.waves == 4;
}
// (H, M, K, D, metric) of tests/test_gpu_launch_plans.py and DESIGN.md, eval and training (one squared-error sum over both legs)
static void documented() {
    for (int train = 0; train < 2; ++train) {
        const bool t = train != 0;
        CallPlan p = plan256(1, 70000, 1024, 256, 0, 1, t);  // 274 row blocks: 256 fused + 18 (35 four-wave workgroups) split 11 ways
        PIN(fused_then_keys(p, 65536, kOneBlock, 11) && p.leg[1].rows == 4464 && p.leg[1].keys.waves == 4 && p.leg[1].planes && p.leg[1].accumulate == t);
        p = plan256(1, 131073, 1024, 256, 0, 1, t);  // 513 row blocks: two rounds on persistent workgroups, ONE row split over the tiles
        PIN(fused_then_keys(p, 131072, kPersist, 32) && p.leg[1].rows == 1 && p.leg[0].choice.screened == !t && p.leg[0].choice.train == t);
        p = plan256(1, 66000, 8192, 256, 0, 1, t);  // 258 row blocks, long sweep
        PIN(fused_then_keys(p, 65536, kOneBlock, 128) && p.leg[1].rows == 464 && p.leg[1].keys.tiles_per_split == 2);
        PIN(one_keys(plan256(1, 40000, 4096, 256, 1, 1, t), 8, kOneBlock));  // 157 row blocks (< one round): K split 8 ways
        PIN(one_keys(plan256(1, 40000, 4096, 512, 0, 1, t), 4, kPair));      // wave pairs in keys mode
        PIN(one_keys(plan256(1, 70000, 8192, 64, 0, 1, t), 13, kOneBlock));
        p = plan256(1, 200000, 1024, 64, 1, 1, t);
        PIN(fused_then_keys(p, 196608, kOneBlock, 8) && p.leg[1].rows == 3392);
        PIN(one_keys(plan256(1, 150000, 4096, 128, 0, 1, t), 3, kOneBlock));
        PIN(one_keys(plan256(8, 10000, 8192, 64, 0, 1, t), 4, kOneBlock));  // 320 workgroups of 8 heads: K split 4 ways
        PIN(one_keys(plan256(4, 20000, 2048, 256, 1, 1, t), 4, kOneBlock));
        PIN(one_fused(plan256(6, 9000, 1024, 512, 0, 1, t), kPair, 8));  // heads that do not divide the CU count
        // residual stacks: whole rounds fused + the remainder stage by stage; short sweeps on 128-row workgroups; few rows all staged
        PIN(fused_then_staged(plan256(1, 70000, 1024, 256, 0, 4, t), 65536, 4464));
        PIN(one_fused(plan256(1, 80000, 256, 256, 0, 3, t), kOneBlock, 4));
        PIN(fused_then_staged(plan256(1, 140000, 512, 200, 0, 2, t), 131072, 8928));
        PIN(one_fused(plan256(1, 65536, 1024, 256, 0, 3, t), kOneBlock, 8));
        PIN(fused_then_staged(plan256(1, 66000, 2048, 256, 0, 3, t), 65536, 464));
        PIN(fused_then_staged(plan256(2, 36000, 1024, 128, 0, 3, t), 32768, 3232));
        p = plan256(1, 34000, 1024, 400, 0, 2, t);
        PIN(fused_then_staged(p, 32768, 1232) && p.leg[0].choice.kind == kPair);
        PIN(fused_then_staged(plan256(2, 35001, 4096, 64, 0, 2, t), 32768, 2233));
        p = plan256(1, 8192, 1024, 256, 0, 8, t);
        PIN(p.nlegs == 1 && p.leg[0].kind == kLegStaged && p.leg[0].accumulate && p.leg[0].keys.splits == 8);
    }
    // _sq_err_cases at 256 CUs, H = 2: each kernel kind that carries the squared-error sum, in total and per head
    for (unsigned flags : {0u, (unsigned)VQ_F_SQERR_PER_HEAD}) {
        const Device dev = {256, 2400};
        PIN(one_fused(plan_call(make_call(2, 128 * 256 + 37, 200, 64, 1, 0, flags, true, false, 0), dev, switch_set(0)), kOneBlock, 8));
        PIN(one_fused(plan_call(make_call(2, 337, 120, 100, 1, 0, flags, true, false, 0), dev, switch_set(0)), kOneBlock, 4));
        PIN(one_fused(plan_call(make_call(2, 66 * 128 + 37, 256, 512, 1, 0, flags, true, false, 0), dev, switch_set(0)), kPair, 8));
        const CallPlan p = plan_call(make_call(2, 255 * 256 + 37, 1024, 256, 1, 0, flags, true, false, 0), dev, switch_set(0));
        PIN(one_fused(p, kPersist, 8) && p.leg[0].choice.train && !p.leg[0].choice.screened);
    }
    // the flagship call (bench.py): one screened persistent launch; a small codebook with many rows: resident, a slab buffer per slab
    CallPlan p = plan256(1, 262144, 1024, 256, 0);
    PIN(one_fused(p, kPersist, 8) && p.leg[0].choice.screened && p.leg[0].choice.stagger && p.leg[0].choice.resolve_split);
    p = plan256(2, 1000000, 256, 64, 0);
    PIN(one_fused(p, kResident, 8) && p.leg[0].res_img_floats == 17408 && p.leg[0].res_nbuf == 4);
}

int main(int argc, char **) {
    if (argc > 1) {  // print the documented plans instead of checking them
        dump_documented();
        return 0;
    }
    sweep();
    documented();
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("search plan ok: %lld plans\n", plans);
    return 0;
}
