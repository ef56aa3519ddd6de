// vq_search_plan.h -- how a nearest-code search is launched: the whole decision, as plain arithmetic.
// Everything a plan depends on is a handful of integers and bits: the device (Device), the environment switches (Switches) and
// the call (Call: sizes, flags and what of the caller's pointers the plans consult).  plan_call turns them into a CallPlan, a flat
// list of at most two legs; vq_search_host.inc describes a vq_args call in these terms and walks the legs.  No HIP, no
// environment, no device query, no pointer: a host program can include this file alone and run the plans of any device
// (tests/cabi/search_plan.cpp sweeps them on the CPU).  The geometry the plans share with the kernels and the workspace sizers
// (tile sizes, grid formulas, workspace sections) is defined here once.
#pragma once

#include <assert.h>

#include "../../include/vq_mi355x.h"

namespace vqi {

// ---- geometry ------------------------------------------------------------------------------------------------------------
constexpr int kTileCodes = 32;
constexpr int kPackSlack = 2048;  // floats of over-copy slack behind every packed image

constexpr int padded_dim(int D) { return D <= 32 ? 32 : D <= 64 ? 64 : D <= 128 ? 128 : D <= 256 ? 256 : D <= 512 ? 512 : 0; }

constexpr int round_up(int a, int b) { return (a + b - 1) / b * b; }

// A staged LDS tile always carries ~33 KB: 32 codes at Dp >= 256, 64 / 128 / 256 codes at Dp = 128 / 64 / 32, so
// the per-tile barrier and LDS-DMA issue are amortised over the same number of MFMAs at every dim.
constexpr int sub_tiles(int DP) { return DP >= 256 ? 1 : 256 / DP; }

// 32-code sub-tiles and tiles of a sweep over K codes at padded dim DP
constexpr int sub_tiles_of(int K) { return (K + kTileCodes - 1) / kTileCodes; }
constexpr int tiles_of(int K, int DP) { return (K + kTileCodes * sub_tiles(DP) - 1) / (kTileCodes * sub_tiles(DP)); }

// Rows per workgroup of the fused single-stage launch: 256 (8 waves x 32), 128 (4 wave pairs / 4 waves) at Dp = 512.
// (At Dp <= 128 two 8-wave workgroups share a CU, but a lone one already runs at ~0.93 of the CU's MFMA rate, so a CU is
//  still one slot of the rounds model below, to within a few percent.)
constexpr int fused_rows_per_wg(int DP) { return DP == 512 ? 128 : 256; }

// workgroups per head (grid.x) of each kernel kind
constexpr long long one_block_grid_x(long long M, int waves) { return (M + 32ll * waves - 1) / (32ll * waves); }
constexpr long long pair_grid_x(long long M) { return (M + 127) / 128; }  // 8 waves = 4 pairs = 128 rows per workgroup
inline long long persist_grid_x(long long M, int H, int cus) {  // one 8-wave workgroup per CU, the CUs shared by the heads
    const long long nblk = (M + 255) / 256;
    long long gx = cus / H;
    if (gx < 1) gx = 1;
    return gx > nblk ? nblk : gx;
}

// the wave-pair kernel (vq_search_pair.inc) holds the winners of every stage of a residual stack in LDS: PairGeo::max_stages()
constexpr int kPairMaxStages = 26;

// small codebooks resident in LDS (vq_search_resident.inc).  Floats the image of K codes takes: whole 1-KiB wave copies (the
// over-copy stays inside the image's slack); LDS of the kernel: image | 8 waves x nbuf slabs of 32 x 16 floats | winners of
// two blocks.
inline int resident_image_floats(int K, int DP) { return round_up(round_up(K, kTileCodes * sub_tiles(DP)) * (DP + 4), 256); }
constexpr size_t resident_lds_bytes(int img_floats, int nbuf) { return ((size_t)img_floats + 8 * nbuf * 512) * 4 + 2 * 8 * 32 * 4; }
#ifndef VQ_EXP_RESIDENT_MIN_ROWS_PER_CU
#define VQ_EXP_RESIDENT_MIN_ROWS_PER_CU 512  // rows per CU from which the resident-codebook kernel takes a small codebook
#endif

// ---- the workspace of a call -----------------------------------------------------------------------------------------------
// Layout: [keys: H*M int64][loss partials: floats][residual rows of a staged tail]
// one plane of keys + room for the planes of a K split (few rows: <= 512 x 256 extra keys; a planned split of a mid-size row
// count: a few planes) -- when the planes do not fit, the splits fall back to ONE plane combined with atomic MIN
constexpr long long kKeyPlanesExtraBytes = 8ll << 20;
constexpr long long ws_keys_bytes(int H, long long M) { return ((long long)H * M * 8 + 255) / 256 * 256 + kKeyPlanesExtraBytes; }
// residual stacks of many rows: room at the END of the workspace for the residual rows of a tail run stage by stage (plan_residual_tail)
constexpr long long kResidualTailBytes = 64ll << 20;
inline long long residual_tail_room(int H, long long M, int Q) {  // (the row width is not known here: 512 dims, capped)
    if (Q < 2) return 0;
    const long long all = ((long long)H * M * 512 * 4 + 255) / 256 * 256;
    return all < kResidualTailBytes ? all : kResidualTailBytes;
}
// loss partials: one float per wave, stage and 32 rows (16 rows for the wave-pair kernel of 256 < D <= 512)
constexpr long long ws_loss_floats(int H, long long M, int Q) { return (long long)H * ((M + 15) / 16 + 16) * Q + (long long)H * 8192 + 64; }
// keys + loss partials of a call, rounded to 256 bytes: what lies in front of the residual rows of a stack's staged tail
constexpr long long ws_core_bytes(int H, long long M, int Q) { return (ws_keys_bytes(H, M) + ws_loss_floats(H, M, Q) * 4 + 256 + 255) / 256 * 256; }
// vq_workspace_bytes
inline long long workspace_bytes(int H, long long M, int Q) { return ws_core_bytes(H, M, Q) + residual_tail_room(H, M, Q); }

// The screened sweep (vq_search_persist.inc).  The room of an image is still that of the bf16-pair image this one replaced
// (32 * 1040 + 128 bytes per tile and 4 behind): vq_screen_image_bytes is part of the ABI and callers have sized buffers by it.
constexpr int kScrTileRoom = kTileCodes * 1040 + 128;
constexpr int kScrCtrlBytes = 16384;  // the control block behind the images (its words: vq_search_persist.inc)
constexpr long long scr_image_bytes(int ntiles) { return ((long long)ntiles * kScrTileRoom + 4ll * ntiles + 255) / 256 * 256; }
// the screened sweep's share of the workspace: [fp16 screen images][control block, kScrCtrlBytes][rows for the second pass: one uint32 per
// row of the call, the full-search list from the front and the rescore list from the back].  A caller-cached screen image
// (vq_args.screen, vq_screen_image_bytes) is the first two; the row list, which needs no initialisation, stays in the workspace.
constexpr long long screen_list_bytes(int H, long long M) { return 4ll * H * M; }
constexpr long long screen_image_bytes(int H, int ntiles) { return (long long)H * scr_image_bytes(ntiles) + kScrCtrlBytes; }
constexpr long long screen_bytes(int H, long long M, int ntiles) { return screen_image_bytes(H, ntiles) + screen_list_bytes(H, M); }
// sub-tiles per sweep for which the screened (and the persistent) kernel exists: one row per sub-tile needs 32; beyond ~100 the
// finalize is < 1 % of a block
constexpr int kPersistMinSub = 32, kPersistMaxSub = 96;

// ---- the inputs of a plan, as values ---------------------------------------------------------------------------------------
struct Device {
    int cus;        // compute units (256 when no device can be asked)
    int clock_mhz;  // shader clock, what the plans price a sub-tile with (2400 when no device can be asked)
};

// one field per environment switch that affects a launch (A/B measurements and tests); set = the variable is in the environment
struct Switches {
    bool single_wave_512;   // VQ_SINGLE_WAVE_512: the one-wave-per-row-block kernel for D > 256
    bool no_persist;        // VQ_NO_PERSIST: the one-block-per-workgroup kernel instead of persistent workgroups
    bool no_persist_train;  // VQ_NO_PERSIST_TRAIN: the same for training-mode calls
    bool no_screen;         // VQ_NO_SCREEN: the fp32 sweep instead of the screened one
    bool pair_no_multi;     // VQ_PAIR_NO_MULTI: residual stacks at Dp = 512 on the one-wave kernel
    bool no_resident;       // VQ_NO_RESIDENT: the tile-streaming kernels for small codebooks
    bool no_residual_tail;  // VQ_NO_RESIDUAL_TAIL: residual stacks in one fused launch whatever the row count
    bool no_stagger;        // VQ_NO_STAGGER: all eight waves run the screened sweep's epilogue at the same place
    bool resolve_no_split;  // VQ_RESOLVE_NO_SPLIT: no split of the second pass's full searches
    int res_skew;           // VQ_RES_SKEW: start-up skew of the second wave per SIMD of the resident kernel (diagnostic)
};

struct Call {
    int H;
    long long M;
    int K, D, Q, metric;
    unsigned flags;  // VQ_F_*
    long long workspace_bytes;
    bool out, idx, best, sq_err, lse, cb, packed;  // which of the call's buffers exist
    bool screen;    // a cached screen image came with the call
    bool vec_x;     // float4 accesses: x with its strides and D (8-byte alignment for 2-byte rows)
    bool vec_fin;   // vec_x, and out / cb (with its stage stride) where they exist
    bool vec_res;   // the resident kernel's: x, out, cb with their row and head strides
    bool vec_wide;  // the fused last slice of wide rows: out with its strides and D, cb with its head stride
};

// ---- which kernel runs a search launch ---------------------------------------------------------------------------------
// Decided ONCE per launch (choose_search) and handed to everything that depends on it: the set-up of the screened sweep's
// images, launch_search, and the reduction of the loss partials that the chosen kernel writes.
enum SearchKind {
    kResident,  // small codebook resident in LDS (vq_search_resident.inc)
    kPersist,   // persistent workgroups at Dp = 256 (vq_search_persist.inc)
    kPair,      // dims split over wave pairs at Dp = 512 (vq_search_pair.inc)
    kOneBlock,  // one row block per workgroup (vq_search.inc)
};
struct SearchChoice {
    SearchKind kind;
    int waves;      // waves per workgroup of the chosen kernel
    bool train;     // kPersist: the deferred copy does the straight-through / squared-error arithmetic
    bool screened;  // kPersist: the fp16 screened sweep + the second pass over its listed rows
    bool cached;    // screened: the images and the control block are the caller's (vq_args.screen), no pack kernel runs
    bool stagger, resolve_split;  // screened: the switches of the sweep's epilogue and of the second pass
};

// loss partials per head and stage that the chosen kernel writes: one per wave of every workgroup of its grid
// (the resident kernel carries no loss)
inline long long loss_partials_per_head(const SearchChoice &c, long long M, int H, int cus) {
    const long long gx = c.kind == kPersist ? persist_grid_x(M, H, cus) : c.kind == kPair ? pair_grid_x(M) : one_block_grid_x(M, c.waves);
    return gx * c.waves;
}

// The wave-pair kernel runs wave B one tile behind wave A: one extra step per sweep.  Worth it from 8 tiles per sweep on.
// Residual stacks as long as the winners of every stage fit its LDS.
inline bool pairs_worth_it(int DP, int tiles_per_split, int Q, const Switches &sw) {
    return DP == 512 && tiles_per_split >= 8 && !sw.single_wave_512 && (Q == 1 || (!sw.pair_no_multi && Q <= kPairMaxStages));
}

// The kernel of a whole fused call (one launch, no K split), in order of precedence.  `waves` is the one-block kernel's
// workgroup size (the caller's plan), `res_img_floats` > 0: resident_image_for took the call.  The screened sweep may use the
// key area of the workspace, which a fused call does not need; with the caller's images only the row list has to fit it.
// (Keys-mode searches and the slices of wide rows get wave pairs or one block: pairs_worth_it alone.)
inline SearchChoice choose_search(int DP, int waves, const Call &a, int res_img_floats, const Device &dev, const Switches &sw) {
    SearchChoice c = {kOneBlock, waves, false, false, false, false, false};
    // Small codebook whose image fits the LDS beside the row slabs
    if (res_img_floats > 0 && (DP == 32 || DP == 64 || DP == 128)) {
        c.kind = kResident;
        c.waves = 8;
        return c;
    }
    // Plain call at Dp = 256 (one stage, aligned fp32 rows, >= 32 sub-tiles per sweep, several row blocks per CU): persistent
    // workgroups that copy block b's winners during block b + 1's sweep.
    const bool train = (a.flags & VQ_F_STE) || a.sq_err;
    const int ntiles = tiles_of(a.K, DP), nsub = ntiles * sub_tiles(DP);
    if (!sw.no_persist && DP == 256 && waves == 8 && a.Q == 1 && !a.lse && !(a.flags & (VQ_F_X_F16 | VQ_F_X_BF16)) && a.vec_x && a.vec_fin &&
        a.D % 4 == 0 && (a.out || a.sq_err) &&                    // (else nothing to copy)
        !(train && sw.no_persist_train) &&
        nsub >= kPersistMinSub && nsub <= kPersistMaxSub &&
        one_block_grid_x(a.M, waves) * a.H >= 2ll * dev.cus) {    // at least two blocks per resident workgroup
        c.kind = kPersist;
        c.train = train;
        // The screened sweep (vq_search_persist.inc, SCREEN): Euclid, inference, no winning distances requested, and its
        // images and row list fit the room.
        c.screened = !train && a.metric == VQ_METRIC_EUCLID && !a.best && !sw.no_screen &&
                     (a.screen ? screen_list_bytes(a.H, a.M) : screen_bytes(a.H, a.M, ntiles)) <= ws_keys_bytes(a.H, a.M) &&
                     scr_image_bytes(ntiles) < (1ll << 31) && (long long)a.H * a.M < (1ll << 31);
        c.cached = c.screened && a.screen;
        c.stagger = c.screened && !sw.no_stagger;
        c.resolve_split = c.screened && !sw.resolve_no_split;
        return c;
    }
    if (pairs_worth_it(DP, ntiles, a.Q, sw)) {
        c.kind = kPair;
        c.waves = 8;
    }
    return c;
}

// Small codebook, plain inference call (one stage, no straight-through / loss / LSE, aligned fp32 rows of D % 16 == 0 dims,
// Dp <= 128) whose image fits the LDS beside the row slabs, and enough rows to give every wave slot of the chip a few 32-row
// blocks: the resident-codebook kernel.  Returns the image's floats, 0: not taken.
inline int resident_image_for(const Call &a, int DP, const Device &dev, const Switches &sw) {
    if (sw.no_resident || DP == 0 || DP > 128 || a.Q != 1 || a.lse || a.sq_err || !a.out || !a.idx || !a.cb || !a.packed) return 0;
    if (a.flags & (VQ_F_STE | VQ_F_FORCE_SIMPLE | VQ_F_FORCE_SPLIT | VQ_F_X_F16 | VQ_F_X_BF16)) return 0;
    if (a.D % 16 || !a.vec_res) return 0;
    const int nsub_k = sub_tiles_of(a.K);
    if (nsub_k < DP / 16) return 0;  // (the sweep's first Dp / 16 sub-tiles carry the next block's slabs)
    if (nsub_k > 8) return 0;        // measured: from K = 512 on the tile-streaming kernels are ahead again
    const int img = resident_image_floats(a.K, DP);
    if (resident_lds_bytes(img, 1) > 160 * 1024) return 0;
    if ((long long)a.H * a.M < (long long)VQ_EXP_RESIDENT_MIN_ROWS_PER_CU * dev.cus) return 0;
    return img;
}
// slab buffers per wave: one per slab of a block when that fits beside the image, else 1
inline int resident_buffers(int img_floats, int DP) { return (DP < 128 && resident_lds_bytes(img_floats, DP / 16) <= 160 * 1024) ? DP / 16 : 1; }

// ---- the cost model of the rounds ------------------------------------------------------------------------------------------
// Time of one 32-code sub-tile of an 8-wave workgroup, microseconds, from the device's own clock instead of a constant
// measured on one box: two waves share a SIMD and each issues Dp / 2 + 1 fp32 MFMAs of 64 cycles per sub-tile (Dp = 256 at
// 2.4 GHz: 6.9 us; the 7.2 us measured in round 2 included the sweep's ~4 % of vector work).  Only the RATIO between a
// sub-tile and the finalize's HBM time enters the plans.
inline double sub_tile_us(int DP, const Device &dev) { return 1.045 * 2.0 * (DP / 2 + 1) * 64.0 / (double)dev.clock_mhz; }

// Quantisation of the grid: with one workgroup per CU the launch runs in rounds of `cus` workgroups, and a row count just
// above a multiple of cus x rows-per-workgroup pays a whole extra round (M = 70 000 at D = 256: 274 workgroups = 2 rounds for
// 1.07 rounds of work).  Splitting K over S workgroups per row block makes the rounds shorter and fuller at the price of one
// more prologue per split and the keys + finalize tail.  Costs in units of one sub-tile of sweep (8 waves): prologue ~1.5,
// fused finalize ~1.2, keys-init + finalize kernels ~ 3 + rows x D x 8 bytes at ~5 TB/s.  Returns the best S (1 = stay fused).
inline int plan_k_split(int DP, int H, long long M, int K, int D, const Device &dev, double *cost = nullptr, double *fused_cost = nullptr) {
    const int cus = dev.cus;
    const int rpw = fused_rows_per_wg(DP);
    const long long nblk = (M + rpw - 1) / rpw * H;
    const int nsub = sub_tiles_of(K);
    if (cost) *cost = *fused_cost = (double)((nblk + cus - 1) / cus) * (1.5 + nsub + 1.2);
    if (nblk * 2 <= cus || nsub < 16) return 1;  // (few workgroups: the older rule of plan_call splits until the chip is full)
    const double sub_us = sub_tile_us(DP, dev);  // one sub-tile of all the workgroup's waves, microseconds
    const double tail = 3.0 + (double)M * H * D * 8.0 / 5e6 / sub_us;  // keys init + finalize kernels
    auto rounds = [&](long long wgs) { return (double)((wgs + cus - 1) / cus); };
    const double fused = rounds(nblk) * (1.5 + nsub + 1.2);
    double best = fused;
    int best_s = 1;
    for (int S = 2; S <= 16 && S * 8 <= nsub; ++S) {
        const int per = (nsub + S - 1) / S;
        const double t = rounds(nblk * S) * (1.5 + per) + tail;
        if (t < best) {
            best = t;
            best_s = S;
        }
    }
    if (best >= 0.88 * fused) return 1;
    if (cost) *cost = best;
    return best_s;
}

// The cut of a grid of `nblk_h` row blocks per head into whole rounds of `cus` workgroups that are also whole row blocks of
// every head (every head gets the same cut), and the workgroups left for a last, partly filled round.
struct RoundsCut {
    long long full, rem;
};
inline RoundsCut whole_rounds(long long nblk_h, int H, int cus) {
    long long full = nblk_h * H / cus;
    while (full > 0 && (full * cus) % H) --full;
    return {full, nblk_h * H - full * cus};
}

// Third remedy for the same quantisation: the row blocks that fill whole rounds run fused, the
// remainder (fewer blocks than CUs) is searched by a second leg, which splits K until the chip is full -- a short round
// instead of a whole one.  Returns the rows of the fused part, 0 when the model does not predict >= 5 % over both alternatives.
inline long long plan_main_tail(int DP, int H, long long M, int K, int D, const Device &dev) {
    const int cus = dev.cus;
    const int rpw = fused_rows_per_wg(DP);
    const RoundsCut cut = whole_rounds((M + rpw - 1) / rpw, H, cus);
    const long long full = cut.full, rem = cut.rem;
    const int nsub = sub_tiles_of(K);
    if (full < 1 || rem == 0 || rem >= cus || nsub < 8) return 0;
    double plan_cost = 0.0, fused_cost = 0.0;
    plan_k_split(DP, H, M, K, D, dev, &plan_cost, &fused_cost);
    int st = (int)((cus + rem - 1) / rem);
    if (st > nsub / 8) st = nsub / 8;
    if (st < 1) st = 1;
    const int per = (nsub + st - 1) / st;
    const double sub_us = sub_tile_us(DP, dev);
    const double tail = (double)((rem * st + cus - 1) / cus) * (1.5 + per) + 3.0 + (double)(rem * rpw) * D * 8.0 / 5e6 / sub_us;
    // (rem counts workgroups of all heads together)
    const double hybrid = (double)full * (1.5 + nsub + 1.2) + tail;
    const double other = plan_cost < fused_cost ? plan_cost : fused_cost;
    return hybrid < 0.95 * other ? full * cus / H * rpw : 0;
}

// ---- residual stacks whose row count leaves the last round of workgroups mostly empty -------------------------------------
// A residual launch cannot split K (every stage needs the whole codebook per row), so M = 70 000 at cfg4's shape pays half a
// round of 128-row workgroups for 7 % of a round of work.  The rows that fill whole rounds run on the fused kernel; the
// remainder runs STAGE BY STAGE, each stage a K-split search over all CUs + a finalize that also writes the next residual
// (r - quant, the fused kernel's arithmetic) into the workspace and accumulates `out`: 2-3 short launches per stage instead of
// half a round of sweep per stage.  The same holds for a stack of FEW rows (less than one round: M = 8192 occupies 32 CUs, or 64
// at one wave per SIMD): then every row runs stage by stage.  Returns the rows (per head) of the fused part -- 0: all rows
// staged -- or -1 = keep the single fused launch.
inline long long plan_residual_tail(const Call &a, int DP, const Device &dev, const Switches &sw) {
    const int cus = dev.cus;
    if (a.Q < 2 || DP == 0 || (a.flags & (VQ_F_FORCE_SIMPLE | VQ_F_FORCE_SPLIT))) return -1;
    if (sw.no_residual_tail) return -1;
    const int rpw = fused_rows_per_wg(DP);  // 256 (128 at Dp = 512)
    const RoundsCut cut = whole_rounds((a.M + rpw - 1) / rpw, a.H, cus);
    const long long full = cut.full, rem = cut.rem;
    if (rem == 0) return -1;
    const long long m1 = full * cus / a.H * rpw, mt = a.M - m1;
    if (mt <= 0 || (long long)a.H * mt * a.D * 4 > residual_tail_room(a.H, a.M, a.Q)) return -1;  // (no room for the residual rows)
    const int nsub = sub_tiles_of(a.K);
    if (nsub < 8) return -1;  // (too short to split)
    const double sweep_us = nsub * sub_tile_us(DP, dev);  // one stage of one round
    // the fused alternative: a whole round, or ~0.55 of one when 128-row workgroups fit one per CU (Dp <= 256: a lone 4-wave
    // workgroup has the matrix pipe to itself, see plan_rows)
    const long long rem4 = ((mt + 127) / 128) * a.H;
    const double fused_rounds = (DP <= 256 && rem4 <= cus) ? 0.55 : 1.0;
    const double fused_us = fused_rounds * a.Q * sweep_us;
    // staged: per stage ~20 us of launches + finalize, the tail's share of a round of sweep (K split: ~1.4 x for the extra prologues)
    const double staged_us = a.Q * (20.0 + 1.4 * sweep_us * (double)rem / cus);
    return staged_us < 0.8 * fused_us ? m1 : -1;
}

// ---- rows wider than 512 dims -------------------------------------------------------------------
// The distance of a (row, code) pair is ONE k-ordered fmaf chain over all dims, so the sweep is cut along d into slices of
// kWideSlice dims: slice j continues the chains slice j - 1 left in the workspace (the accumulators' own fragment layout: every
// lane reads back exactly the 16-byte pieces it wrote, coalesced), and the last slice closes them with the norms and runs
// the argmin into packed keys.  The workspace holds the chains of one (row chunk) x (code chunk) at a time.
#ifndef VQ_EXP_WIDE_SLICE
#define VQ_EXP_WIDE_SLICE 512  // dims per slice of rows wider than 512 dims (256: the round-2 scheme, twice the accumulator traffic)
#endif
constexpr int kWideSlice = VQ_EXP_WIDE_SLICE;                // dims per slice: 512 (4-wave workgroups) or 256 (8-wave)
constexpr int kWideWaves = kWideSlice == 512 ? 4 : 8;
constexpr int kWideRows = 32 * kWideWaves;                   // rows per workgroup
#ifndef VQ_EXP_WIDE_CHUNK_MB
#define VQ_EXP_WIDE_CHUNK_MB 512
#endif
constexpr long long kWideChunkBytes = (long long)VQ_EXP_WIDE_CHUNK_MB << 20;  // accumulator workspace per (row chunk, code chunk)
constexpr int kWideCodes = 4096;                    // codes per chunk

struct WidePlan {
    int nd;            // slices
    int kc;            // codes per chunk (multiple of 32)
    long long mc;      // rows per chunk (multiple of kWideRows)
    long long acc_bytes, xn_bytes;
};

inline WidePlan wide_plan(int H, long long M, int K, int D) {
    WidePlan w;
    w.nd = (D + kWideSlice - 1) / kWideSlice;
    const int Kp = round_up(K, kTileCodes);
    w.kc = Kp < kWideCodes ? Kp : kWideCodes;
    const long long Mp = (M + kWideRows - 1) / kWideRows * kWideRows;
    long long mc = kWideChunkBytes / ((long long)H * w.kc * 4) / kWideRows * kWideRows;
    if (mc < kWideRows) mc = kWideRows;
    if (mc > Mp) mc = Mp;
    w.mc = mc;
    w.acc_bytes = (long long)H * mc * w.kc * 4;
    w.xn_bytes = 2 * (((long long)H * mc * 4 + 255) / 256 * 256);  // two buffers: a slice reads one and writes the other
    return w;
}

inline long long wide_image_floats(int K) { return (long long)round_up(K, kTileCodes) * (kWideSlice + 4) + kPackSlack; }
// the last slice is padded like a narrow row of its own width (32 ... kWideSlice dims) and packed in that layout
inline int wide_last_dims(int D) { return D - (D - 1) / kWideSlice * kWideSlice; }
inline long long wide_last_image_floats(int K, int D) {
    const int DP = padded_dim(wide_last_dims(D));
    return (long long)round_up(K, kTileCodes * sub_tiles(DP)) * (DP + 4) + kPackSlack;
}
// vq_workspace_bytes_wide of a call of wide rows
inline long long wide_workspace_bytes(int H, long long M, const WidePlan &w) { return workspace_bytes(H, M, 1) + w.acc_bytes + w.xn_bytes; }

// ---- keys-mode searches ----------------------------------------------------------------------------------------------------
// Workgroup size of the one-block kernel and the workgroups of its grid: 8 waves (4 at Dp = 512: LDS), or 4 when the 8-wave
// grid leaves CUs empty.
struct WaveGrid {
    int waves;
    long long wgs;
};
inline WaveGrid wave_grid(int DP, int H, long long M, int cus, bool may_halve = true) {
    WaveGrid g = {DP == 512 ? 4 : 8, 0};
    g.wgs = H * one_block_grid_x(M, g.waves);
    if (may_halve && g.waves == 8 && g.wgs < cus) g = {4, H * one_block_grid_x(M, 4)};
    return g;
}

// The fill rule: K is split over workgroups until the chip is full (`fill` workgroups) -- splitting further only repeats the
// prologue and, in the wave-pair kernel, the extra pipeline step.  At most one split per tile.
inline int fill_splits(long long fill, long long wgs, int ntiles) {
    if (wgs >= fill) return 1;
    int splits = (int)((fill + wgs - 1) / wgs);
    if (splits > ntiles) splits = ntiles;
    return splits < 1 ? 1 : splits;
}
// `splits` evened out so that every split owns at least one tile
struct TileSplit {
    int splits, tiles_per_split;
};
inline TileSplit even_splits(int ntiles, int splits) {
    const int per = (ntiles + splits - 1) / splits;
    return {(ntiles + per - 1) / per, per};
}

// How a keys-mode search is launched: workgroup size and the number of K splits (= key planes when the splits store into
// planes of their own instead of combining with atomic MIN), wave pairs or one block.
struct KeysPlan {
    int DP, waves, splits, tiles_per_split;
    bool mfma;       // false: the one-thread-per-row kernel / the sliced sweep of wide rows (one plane, atomic MIN)
    bool wide_rows;  // !mfma: the sliced sweep of rows wider than 512 dims, `wide` its plan
    WidePlan wide;
    SearchChoice choice;  // mfma: wave pairs or one block
};
// `planned_splits` > 0: plan_k_split's (full-size workgroups, S splits)
inline KeysPlan plan_keys(int H, long long M, int K, int D, unsigned flags, int planned_splits, const Device &dev, const Switches &sw) {
    KeysPlan k = {};
    k.DP = padded_dim(D);
    k.mfma = k.DP != 0 && !(flags & VQ_F_FORCE_SIMPLE);
    k.waves = 8;
    k.splits = 1;
    k.tiles_per_split = 1;
    k.choice = {kOneBlock, 8, false, false, false, false, false};
    k.wide_rows = k.DP == 0 && !(flags & VQ_F_FORCE_SIMPLE);
    if (k.wide_rows) k.wide = wide_plan(H, M, K, D);
    if (!k.mfma) return k;
    const int ntiles = tiles_of(K, k.DP);
    const WaveGrid g = wave_grid(k.DP, H, M, dev.cus, /*may_halve=*/planned_splits == 0);
    k.waves = g.waves;
    // full: two 4-wave workgroups fit a CU at Dp <= 256, one (LDS) at Dp = 512
    const int splits = planned_splits > 0 ? (planned_splits < ntiles ? planned_splits : ntiles)
                                          : fill_splits((long long)dev.cus * (k.DP == 512 ? 1 : 2), g.wgs, ntiles);
    const TileSplit ts = even_splits(ntiles, splits);
    k.splits = ts.splits;
    k.tiles_per_split = ts.tiles_per_split;
    if (pairs_worth_it(k.DP, k.tiles_per_split, 1, sw)) k.choice = {kPair, 8, false, false, false, false, false};
    else k.choice.waves = k.waves;
    return k;
}
// the splits of a keys-mode search store into planes of their own when the planes fit the key area of a call of M rows
inline bool key_planes_fit(const KeysPlan &k, int H, long long M) { return k.mfma && (long long)k.splits * H * M * 8 <= ws_keys_bytes(H, M); }

// K splits of one slice launch (`nblk` row blocks per head, `kcodes` codes of the chunk in `ntiles` tiles): the fill rule -- one
// workgroup per CU at Dp = 512 / 8 waves at Dp = 256 -- and, for a full grid that is not the fused last slice, plan_k_split
// for the partly filled last round of workgroups
inline TileSplit wide_slice_splits(int DP, int H, long long nblk, long long mrows, int kcodes, int ntiles, bool fused, const Device &dev) {
    const long long fill = (long long)dev.cus * ((DP == 512 || (kWideWaves == 8 && DP == 256)) ? 1 : 2);
    int splits = 1;
    if (nblk * H < fill) {
        splits = fill_splits(fill, nblk * H, ntiles);
    } else if (!fused) {
        splits = plan_k_split(DP, H, mrows, kcodes, DP, dev);
        if (splits > ntiles) splits = ntiles;
    }
    return fused ? TileSplit{1, ntiles} : even_splits(ntiles, splits);
}

// One (row chunk, code chunk) covers all codes and every launch fills the chip without a K split: the last slice can finish
// the inference call itself (idx, best, out = codebook[idx]) instead of going through keys and the finalize kernel.
inline bool wide_fusable(const Call &a, const Device &dev) {
    if (a.Q != 1 || (a.flags & (VQ_F_STE | VQ_F_FORCE_SPLIT | VQ_F_FORCE_SIMPLE)) || a.sq_err || !a.out || !a.idx || !a.cb) return false;
    if (!a.vec_wide) return false;
    if (round_up(a.K, kTileCodes) > kWideCodes) return false;
    const WidePlan w = wide_plan(a.H, a.M, a.K, a.D);
    const long long last_rows = a.M % w.mc ? a.M % w.mc : w.mc;  // the smallest row chunk
    if (((last_rows + kWideRows - 1) / kWideRows) * a.H < dev.cus) return false;
    // a row count that leaves the last round of workgroups mostly empty is better served by a K split (keys path)
    return plan_k_split(kWideSlice, a.H, w.mc < a.M ? w.mc : a.M, a.K, kWideSlice, dev) == 1;
}

// ---- the plan of a whole call --------------------------------------------------------------------------------------------
enum LegKind {
    kLegFused,      // one launch of `choice`'s kernel: search, gather, straight-through, loss partials
    kLegKeys,       // K-split MFMA search into packed keys (`keys`, `planes`) + the finalize kernel
    kLegStaged,     // the tail of a residual stack stage by stage, each stage a kLegKeys of its own
    kLegWideFused,  // rows wider than 512 dims, the last slice finishes the call
    kLegWideKeys,   // rows wider than 512 dims into one plane of keys + the finalize kernel
    kLegScalar,     // the one-thread-per-row kernel into one plane of keys + the finalize kernel
    kLegNoStack,    // refused: residual stages need the MFMA kernel (D <= 512)
    kLegNoPerHead,  // refused: per-head squared errors need the MFMA kernel
};

struct Leg {
    LegKind kind;
    long long row_begin, rows;
    bool accumulate;  // its squared-error sums are added to the previous leg's (a leg 0 that accumulates: to zero, cleared first)
    int DP;
    SearchChoice choice;              // kLegFused
    int res_img_floats, res_nbuf;     // kLegFused, kResident
    KeysPlan keys;                    // kLegKeys, kLegStaged (every stage alike), kLegWideKeys / kLegScalar (mfma = false)
    bool planes;                      // the splits write key planes (else one plane, initialised, atomic MIN)
    WidePlan wide;                    // kLegWideFused
};

constexpr int kMaxLegs = 2;
struct CallPlan {
    int nlegs;
    Leg leg[kMaxLegs];
};

inline Leg &new_leg(CallPlan &plan, LegKind kind, long long row_begin, long long rows, bool accumulate, int DP) {
    assert(plan.nlegs < kMaxLegs);
    Leg &leg = plan.leg[plan.nlegs++];
    leg = Leg{};
    leg.kind = kind;
    leg.row_begin = row_begin;
    leg.rows = rows;
    leg.accumulate = accumulate;
    leg.DP = DP;
    return leg;
}

// The rows [row_begin, row_begin + a.M) of a call as a call of their own: `a` is the caller's call with M = those rows (the
// workspace sections of a leg are those of ITS row count).  `acc`: the leg adds its squared-error sum to the one before it, and
// is not cut again.  A cut hands both parts back to this function: whole rounds, for which no further cut applies, and a
// remainder that either carries `acc` or is too short for one -- so a plan is at most two legs.
inline void plan_rows(const Call &a, long long row_begin, bool acc, const Device &dev, const Switches &sw, CallPlan &plan) {
    const int cus = dev.cus;
    const int DP = padded_dim(a.D);
    const bool simple = (a.flags & VQ_F_FORCE_SIMPLE) || DP == 0;
    const bool per_head = (a.flags & VQ_F_SQERR_PER_HEAD) && a.sq_err;
    const bool two_byte = (a.flags & (VQ_F_X_F16 | VQ_F_X_BF16)) != 0;
    auto part = [&](long long m0, long long rows, bool part_acc) {
        Call b = a;
        b.M = rows;
        b.lse = false;
        plan_rows(b, row_begin + m0, part_acc, dev, sw, plan);
    };

    const int res_img = (simple || acc) ? 0 : resident_image_for(a, DP, dev, sw);
    if (!res_img && !simple && a.Q == 1 && !a.lse && !acc && !per_head && !(a.flags & VQ_F_FORCE_SPLIT) && !two_byte) {
        const long long m1 = plan_main_tail(DP, a.H, a.M, a.K, a.D, dev);
        if (m1 > 0 && m1 < a.M) {  // whole rounds fused, then the remainder as its own (K-split) leg
            part(0, m1, false);
            part(m1, a.M - m1, a.sq_err);  // one squared-error sum over both parts, fixed order
            return;
        }
    }

    if (!simple && a.Q > 1 && !acc && a.packed && a.workspace_bytes >= workspace_bytes(a.H, a.M, a.Q)) {
        const long long m1 = plan_residual_tail(a, DP, dev, sw);
        if (m1 >= 0 && m1 < a.M) {  // whole rounds on the fused kernel, the remainder stage by stage (K split over all CUs)
            if (m1 > 0) part(0, m1, false);
            Leg &tail = new_leg(plan, kLegStaged, row_begin + m1, a.M - m1, /*accumulate=*/true, DP);  // (the stages ADD their sums)
            tail.keys = plan_keys(a.H, tail.rows, a.K, a.D, a.flags, 0, dev, sw);
            tail.planes = key_planes_fit(tail.keys, a.H, tail.rows);
            return;
        }
    }

    Leg &leg = new_leg(plan, kLegNoStack, row_begin, a.M, acc, DP);

    // ---- fused (one launch, no K split) or split (keys + finalize) ----
    bool fused = !simple;
    int planned_splits = 0;
    int waves = (DP == 512) ? 4 : 8;
    if (fused) {
        const WaveGrid g = wave_grid(DP, a.H, a.M, cus);
        waves = g.waves;
        long long wgs = g.wgs;
        // Residual stacks cannot split K (every stage needs the whole codebook per row), so a row count just above a multiple of
        // cus x 256 used to pay a whole extra round of 8-wave workgroups.  Two 4-wave workgroups share a CU at the pace of one
        // 8-wave workgroup, and a LONE 4-wave workgroup (one wave per SIMD: the matrix pipe to itself) finishes its 128 rows in
        // about half a round -- so with 128-row workgroups the remainder costs half a round instead of a whole one whenever it
        // fits one workgroup per CU (M = 70 000 at cfg4's shape: 2 rounds -> ~1.55).
        if (waves == 8 && DP == 256 && a.Q > 1) {
            const long long nblk4 = (long long)a.H * ((a.M + 127) / 128);
            const long long full = nblk4 / (2ll * cus), rem = nblk4 % (2ll * cus);
            const double t8 = (double)((wgs + cus - 1) / cus);
            const double t4 = (double)full + (rem == 0 ? 0.0 : (rem <= cus ? 0.55 : 1.0));
            if (t4 < 0.97 * t8) {
                waves = 4;
                wgs = nblk4;
            }
        }
#ifdef VQ_EXP_WAVES
        waves = VQ_EXP_WAVES;  // diagnostic builds only
#endif
        const int ntiles = tiles_of(a.K, DP);
        // few workgroups and a long sweep: splitting K over workgroups fills the chip (Q == 1 only)
        if (a.Q == 1 && wgs * 2 <= cus && ntiles * sub_tiles(DP) >= 8 && ntiles >= 2) fused = false;
        if ((a.flags & VQ_F_FORCE_SPLIT) && a.Q == 1) fused = false;
        if (fused && a.Q == 1 && !two_byte) {
            planned_splits = plan_k_split(DP, a.H, a.M, a.K, a.D, dev);  // grid quantisation (see plan_k_split)
            if (planned_splits > 1) fused = false;
        }
        if (res_img) fused = true;  // small codebook resident in LDS: 32-row granularity, no plan needed
        if (a.lse) fused = true;    // the log-sum-exp needs every code of a row in one workgroup
        if (per_head) fused = true;  // per-head partial sums exist on this path only
    }

    if (fused) {
        leg.kind = kLegFused;
        leg.res_img_floats = res_img;
        leg.res_nbuf = res_img ? resident_buffers(res_img, DP) : 0;
        // the one decision which kernel runs this leg: the screen images, the launch and the partials' count all follow it
        leg.choice = choose_search(DP, waves, a, res_img, dev, sw);
        return;
    }
    if (DP == 0 && wide_fusable(a, dev)) {
        leg.kind = kLegWideFused;
        leg.wide = wide_plan(a.H, a.M, a.K, a.D);
        return;
    }
    if (a.Q != 1) return;  // (kLegNoStack)
    if (per_head) {
        leg.kind = kLegNoPerHead;
        return;
    }
    leg.keys = plan_keys(a.H, a.M, a.K, a.D, a.flags, planned_splits, dev, sw);
    leg.planes = key_planes_fit(leg.keys, a.H, a.M);
    leg.kind = leg.keys.mfma ? kLegKeys : leg.keys.wide_rows ? kLegWideKeys : kLegScalar;
}

// the plan of a checked call (no rows: no legs)
inline CallPlan plan_call(const Call &a, const Device &dev, const Switches &sw) {
    CallPlan plan;
    plan.nlegs = 0;
    if (a.M > 0) plan_rows(a, 0, false, dev, sw, plan);
    return plan;
}

}  // namespace vqi
