// Host check of csrc/vq_resolve_plan.h, the arithmetic every workgroup of vq_resolve_rows_kernel runs: for grids 1 .. 304,
// full-search counts 0 .. 700 and rescore counts 0 .. 300 000 every slice of every row is taken exactly once, every rescore
// batch by exactly one wave, a row's ticket is drawn S times, and S is 1 above half the grid.  The workgroups are walked the
// way the kernel walks them (resolve_wg_rows, resolve_wave_codes, resolve_wave_batches).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vq_resolve_plan.h"

static int fails = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            if (fails++ < 20) {            \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);  \
                std::printf("\n");         \
            }                              \
        }                                  \
    } while (0)

static void check_codes(unsigned K, unsigned S) {
    unsigned next = 0;
    for (unsigned s = 0; s < S; ++s)
        for (unsigned w = 0; w < kResolvePlanWaves; ++w) {
            unsigned kb, ke;
            resolve_wave_codes(K, S, s, w, kb, ke);
            CHECK(kb == next && ke >= kb && ke <= K, "K %u S %u slice %u wave %u: [%u, %u) after %u", K, S, s, w, kb, ke, next);
            CHECK((ke - kb) <= resolve_passes(K, S) * kResolvePassCodes, "K %u S %u: run longer than its passes", K, S);
            next = ke;
        }
    CHECK(next == K, "K %u S %u: codes end at %u", K, S, next);
}

static void check_case(unsigned grid, unsigned count, unsigned n1, unsigned K, bool allow) {
    const ResolvePlan pl = resolve_plan(count, n1, grid, K, allow);
    CHECK(pl.S >= 1 && pl.S <= kResolveMaxSplit, "grid %u count %u n1 %u: S %u", grid, count, n1, pl.S);
    if (2 * count > grid || !allow || count == 0) CHECK(pl.S == 1, "grid %u count %u n1 %u: S %u above half the grid", grid, count, n1, pl.S);
    if (pl.S > 1) {
        CHECK(count <= kResolveMaxSplitRows && (unsigned long long)count * pl.S <= grid, "grid %u count %u: S %u has no room", grid, count, pl.S);
        CHECK(resolve_passes(K, pl.S) < resolve_passes(K, 1), "grid %u count %u K %u: S %u saves no pass", grid, count, K, pl.S);
    }
    CHECK(pl.nbatch == (n1 + kResolveBatchRows - 1) / kResolveBatchRows, "nbatch");
    std::vector<unsigned char> taken((size_t)count * pl.S, 0), batch(pl.nbatch, 0);
    std::vector<unsigned> ticket(count, 0);
    for (unsigned wg = 0; wg < grid; ++wg) {
        unsigned first, step, slice;
        resolve_wg_rows(pl, count, grid, wg, first, step, slice);
        CHECK(step > 0 || first >= count, "grid %u count %u wg %u: step 0", grid, count, wg);
        for (unsigned e = first; e < count; e += step) {
            CHECK(slice < pl.S, "slice %u of %u", slice, pl.S);
            if (slice < pl.S) ++taken[(size_t)e * pl.S + slice];
            ++ticket[e];
            if (step == 0) break;
        }
        for (unsigned w = 0; w < kResolvePlanWaves; ++w) {
            unsigned bfirst, bstride;
            resolve_wave_batches(pl, grid, wg, w, bfirst, bstride);
            CHECK(bstride > 0, "batch stride 0");
            for (unsigned b = bfirst; b < pl.nbatch && bstride; b += bstride) ++batch[b];
        }
    }
    for (size_t i = 0; i < taken.size(); ++i)
        CHECK(taken[i] == 1, "grid %u count %u n1 %u K %u: slice %zu of row %zu taken %u times", grid, count, n1, K, i % pl.S, i / pl.S, taken[i]);
    for (unsigned e = 0; e < count; ++e) CHECK(ticket[e] == pl.S, "grid %u count %u: ticket of row %u drawn %u times, S %u", grid, count, e, ticket[e], pl.S);
    for (unsigned b = 0; b < pl.nbatch; ++b) CHECK(batch[b] == 1, "grid %u count %u n1 %u: batch %u taken %u times", grid, count, n1, b, batch[b]);
}

int main() {
    for (unsigned K = 1; K <= 3100; K += (K < 1100 ? 1 : 7))
        for (unsigned S = 1; S <= kResolveMaxSplit; ++S) check_codes(K, S);
    const unsigned n1s[] = {0, 1, 15, 16, 17, 2047, 2048, 2049, 9000, 300000};
    const unsigned Ks[] = {1024, 1030, 3072};
    unsigned long long split_cases = 0, cases = 0;
    for (unsigned grid = 1; grid <= 304; ++grid) {
        const unsigned h = grid / 2;
        const unsigned counts[] = {0, 1, 2, 3, 37, 74, h > 0 ? h - 1 : 0, h, h + 1, grid - 1, grid, grid + 1, 2 * grid + 3, 160, 161, 700};
        for (unsigned count : counts)
            for (unsigned n1 : n1s)
                for (unsigned K : Ks) {
                    check_case(grid, count, n1, K, true);
                    split_cases += resolve_plan(count, n1, grid, K).S > 1;
                    ++cases;
                }
        check_case(grid, h, 16, 1024, false);
    }
    // every full-search count and a scan of the rescore counts at the grids the kernel runs with and at the smallest ones
    const unsigned grids[] = {1, 2, 3, 8, 255, 256, 304};
    for (unsigned grid : grids)
        for (unsigned count = 0; count <= 700; ++count)
            for (unsigned n1 = 0; n1 <= 300000; n1 = n1 < 40 ? n1 + 1 : n1 * 3 + 1) check_case(grid, count, n1, 1024, true), ++cases;
    // the headline shape: 74 rows, 9 000 rescore rows, 256 workgroups -> two slices per row, 108 workgroups for 563 batches
    const ResolvePlan cfg2 = resolve_plan(74, 9000, 256, 1024);
    CHECK(cfg2.S == 2 && cfg2.busy == 148 && cfg2.sharers == 108, "cfg2: S %u busy %u sharers %u", cfg2.S, cfg2.busy, cfg2.sharers);
    CHECK(split_cases > 1000, "only %llu of the cases split a row", split_cases);
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("resolve plan ok: %llu cases, %llu of the sampled ones split\n", cases, split_cases);
    return 0;
}
