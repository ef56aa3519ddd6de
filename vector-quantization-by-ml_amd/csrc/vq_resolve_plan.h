// vq_resolve_plan.h -- who does what in the second pass of the screened sweep (vq_resolve_rows_kernel, vq_search_persist.inc).
// Plain arithmetic, the same on the host and on the device: every workgroup of the kernel derives the one plan from the two
// list counts, the grid size and K, and a host program can include this file alone (tests/test_resolve_plan_host.py).
//
// The kernel's work: `count` rows to search again in full (one row reads the whole packed image: ~20 us through one CU at
// K = 1024, a chain of chunk steps that is bound by latency, not by bandwidth) and ceil(n1 / kRsEntries) rescore batches (a
// wave each, about the length of one 64-code pass).  With few full searches most of the chip used to wait for the one
// workgroup per row.  So when the rows are few, each row's K codes are split over S workgroups ("slices"): workgroup
// e * S + s searches slice s of row e, and the last of the S to finish combines their results (a ticket per row; nobody
// waits).  The workgroups without a slice take the rescore batches.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VQ_PLAN_FN __host__ __device__ inline
#else
#define VQ_PLAN_FN inline
#endif

constexpr unsigned kResolvePlanWaves = 8;   // waves per workgroup of the kernel (kResolveWaves)
constexpr unsigned kResolvePassCodes = 64;  // codes per wave and pass (kExCodes)
constexpr unsigned kResolveBatchRows = 16;  // rows per rescore batch (kRsEntries)
constexpr unsigned kResolveMaxSplit = 8;    // slices per row at most
constexpr unsigned kResolveMaxSplitRows = 160;  // rows that can be split: the control block has a ticket and slots for so many

struct ResolvePlan {
    unsigned S;        // slices per full-search row; 1: rows are dealt grid-stride, one workgroup each, no tickets
    unsigned busy;     // workgroups 0 .. busy - 1 have a slice (S > 1) or at least one row (S == 1)
    unsigned sharers;  // the LAST `sharers` workgroups of the grid share the rescore batches (the whole grid when too few are free)
    unsigned nbatch;
};

// 64-code passes of one wave when a row's K codes are split over S workgroups of 8 waves
VQ_PLAN_FN unsigned resolve_passes(unsigned K, unsigned S) {
    const unsigned per_wave = (K + S * kResolvePlanWaves - 1) / (S * kResolvePlanWaves);
    return (per_wave + kResolvePassCodes - 1) / kResolvePassCodes;
}

// the codes [kbeg, kend) of wave `wave` of slice `s`: runs of whole passes in the order (slice, wave), so that the slices of a
// row cover 0 .. K - 1 exactly once and S == 1 is the one-workgroup split
VQ_PLAN_FN void resolve_wave_codes(unsigned K, unsigned S, unsigned s, unsigned wave, unsigned &kbeg, unsigned &kend) {
    const unsigned per = resolve_passes(K, S) * kResolvePassCodes;
    const unsigned long long b = (unsigned long long)(s * kResolvePlanWaves + wave) * per;
    kbeg = b < K ? (unsigned)b : K;
    kend = b + per < K ? (unsigned)(b + per) : K;
}

// `count` full-search rows, `n1` rescore rows (both already clamped to the list's capacity), `grid` workgroups, K codes;
// `allow_split` false: S = 1 whatever the counts (the A/B switch).
// S > 1 only when the rows are at most half the grid (and the control block has slots for them); among the S for which
//  * every slice has a workgroup of its own (count S <= grid), and
//  * the workgroups left over can take every rescore batch in one round of their 8 waves (a batch is about as long as one
//    pass, the shortest a slice can be: more rounds would make the batches, not the rows, the kernel's length),
// the one with the fewest passes per wave wins, the smallest S among equals (more slices than that only idle lanes).
VQ_PLAN_FN ResolvePlan resolve_plan(unsigned count, unsigned n1, unsigned grid, unsigned K, bool allow_split = true) {
    ResolvePlan pl;
    pl.nbatch = (n1 + kResolveBatchRows - 1) / kResolveBatchRows;
    pl.S = 1;
    if (allow_split && count > 0 && 2 * count <= grid && count <= kResolveMaxSplitRows) {
        unsigned best = resolve_passes(K, 1);
        for (unsigned s = 2; s <= kResolveMaxSplit && count * s <= grid; ++s) {
            if ((unsigned long long)(grid - count * s) * kResolvePlanWaves < pl.nbatch) break;
            const unsigned ps = resolve_passes(K, s);
            if (ps < best) {
                best = ps;
                pl.S = s;
            }
        }
    }
    const unsigned long long want = (unsigned long long)count * pl.S;
    pl.busy = want < grid ? (unsigned)want : grid;
    const unsigned nfree = grid - pl.busy;
    pl.sharers = nfree ? nfree : grid;
    return pl;
}

// full-search rows of workgroup `wg`: rows first, first + step, ... below `count`, and the slice of them it searches.  S > 1:
// the one row wg / S, slice wg % S (workgroups from `busy` on have none); S == 1: grid-stride, whole rows.
VQ_PLAN_FN void resolve_wg_rows(const ResolvePlan &pl, unsigned count, unsigned grid, unsigned wg, unsigned &first, unsigned &step,
                                unsigned &slice) {
    if (pl.S > 1) {
        slice = wg % pl.S;
        first = wg < pl.busy ? wg / pl.S : count;
        step = count;  // (> 0 here; first + step >= count: one row)
    } else {
        slice = 0;
        first = wg;
        step = grid;
    }
}

// rescore batches of one wave: workgroup `wg` of `grid`, wave `wave`.  Batches go to the sharers from the last workgroup
// downwards, one batch for every sharer before a second wave of any of them gets one: batch b belongs to sharer b % sharers
// (counted from the last workgroup), wave (b / sharers) % 8.  -> the first batch of the wave and the stride to its next ones;
// first >= nbatch: none.  A workgroup that has a slice or rows of its own takes its batches after them.
VQ_PLAN_FN void resolve_wave_batches(const ResolvePlan &pl, unsigned grid, unsigned wg, unsigned wave, unsigned &first, unsigned &stride) {
    const unsigned from_last = grid - 1u - wg;
    stride = pl.sharers * kResolvePlanWaves;
    first = from_last < pl.sharers ? from_last + wave * pl.sharers : pl.nbatch;
    if (first > pl.nbatch) first = pl.nbatch;
}
