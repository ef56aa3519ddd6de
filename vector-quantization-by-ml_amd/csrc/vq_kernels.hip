// vq_kernels.hip -- nearest-codebook search for MI355X (gfx950 / CDNA4).  Hand-written HIP, no
// compatibility layers.  See DESIGN.md for the full description; summary of the data path:
//
//   pack      natural codebook [K, D]  ->  packed image  [Kp][Dp + 4]  (even/odd de-interleave inside
//             each group of 8 dims, pre-scaled by -2 for Euclid, |c|^2 in float Dp of every row)
//             (+ a "some code is non-finite" word per image: ATen's argmax rule for NaN / inf inputs is restored out of line,
//             see repair_nonfinite_rows in vq_search.inc)
//   search    one wave owns 32 rows of x for the whole sweep; their fp32 values live in REGISTERS as
//             v_mfma_f32_32x32x2_f32 B-fragments (Dp/2 VGPRs per lane).  The workgroup streams ~33 KB
//             tiles of the packed image HBM/L2 -> LDS with buffer_load ... lds (LDS-DMA, double
//             buffered) and each wave runs Dp/2 MFMAs per 32-code sub-tile (codes on the MFMA i axis,
//             rows on the j axis), then ONE more MFMA that adds |x|^2 * 1 + 1 * |c|^2  (the two
//             augmented GEMM columns of ATen's cdist).  The 32x32 result is reduced in-lane (a lane holds
//             16 codes of ONE row): min3 tree per sub-tile, the record sub-tile's values are parked and
//             the tie-exact rule (correctly rounded sqrt, lowest index) is resolved once per sweep.
//   finalize  gather codebook[idx] (natural layout), straight-through, squared-error sums; fused in
//             the search kernel unless the sweep was split over K (packed 64-bit keys + atomic min).
//
// Arithmetic contract (bit-exact twin: oracle/vq_oracle.c): every distance is the k-ordered fmaf
// chain  fma(1*|c|^2 .. fma(|x|^2*1, fma(x_{D-1}, -2c_{D-1}, ... fma(x_0, -2c_0, 0))))  which is what
// v_mfma_f32_32x32x2_f32 computes; norms are d-ordered fmaf chains; sqrt is correctly rounded.
//
// Source layout (ONE source file: the .inc files are included below inside the anonymous namespace, in this order; the file
// is compiled either whole or once per build part -- see "Build parts"):
//   vq_common.inc        constants, error strings, the kernel-launch helper, metric / padded-dim dispatch, packed (value, index) keys
//   vq_pack.inc          natural codebook -> packed image
//   vq_search.inc        the hot kernel (tile geometry, LDS-DMA staging, MFMA fragment pipeline, tie-exact epilogue, finalize)
//                        and what other sweep kernels share with it: load_x_fragments (a wave's rows -> B fragments + the
//                        |x|^2 chain, for the training-side sweeps), stage_tile, lane_best_start, store_sims_subtile; the
//                        search kernels' back end: row_winner, close_lse, store_key, store_winner, fill_row_from_memory,
//                        wide_acc_init, gather_wide_rows, store_loss_partials
//   vq_search_pair.inc   the same search for 256 < D <= 512 with the dims split over a pair of waves (accumulator hand-off)
//   vq_search_persist.inc  inference search at Dp = 256 with block b's gather hidden inside block b + 1's sweep
//   vq_search_resident.inc small codebooks: the packed image stays in LDS, no barriers, rows streamed past it by LDS-DMA slabs
//   vq_sample.inc        counter-based Gumbel noise (Philox4x32-10) for Gumbel-max code sampling, its test-hook kernel
//   vq_similarity.inc    the same sweep with the similarity / online-softmax / Gumbel-max sampling epilogues, fused
//                        cross-entropy backward
//   vq_gumbel.inc        the resident/streamed sweep with its role table, fourteen roles: Gumbel straight-through and reinmax
//                        backward, codebook diversity loss, orthogonal regularisation loss, the cross-entropy loss's codes
//                        gradient; the row / index packers and the split reductions
//   vq_finalize_ema.inc scalar fallback search, finalize-from-keys, loss reduction, EMA codebook update
//   vq_rotate.inc        the rotation trick: backward of the quantize step with the rotation-and-rescale gradient, one wave per
//                        row with the row in registers (vq_rotate_backward_f32)
//   vq_lfq.inc           lookup-free quantization: sign quantizer, factorised entropy loss forward / backward (stage axis)
//   vq_rlfq.inc          residual LFQ: every stage's quantize step in one pass (residual in registers), its backward
//   vq_fsq.inc           finite scalar quantization (FSQ / residual FSQ): every stage of every group in one pass, its
//                        backward, index -> code decode
//   vq_lq.inc            latent quantization: per-dimension level search against learnable value tables (in LDS), index,
//                        fused squared-error loss and its backward
//   vq_affine.inc        affine re-parameterisation: one-read column mean / squared deviations (Welford lanes, Chan merges),
//                        the moment-matching transform of the codes and of the accumulated EMA sums
//   vq_decode.inc        indices -> code vectors: every stage's gather and their stage-ordered sum in one pass (vq_decode_f32)
//   vq_lfq_decode.inc    the same for the lookup-free family: codes from the index bits, no table (vq_lfq_decode_f32)
//   vq_diversity.inc     codebook diversity loss: the head-ordered sum of the position table (its sweeps are roles of vq_gumbel.inc)
//   (orthogonal regularisation loss: the kOrth role of vq_gumbel.inc, no file of its own)
//   this file           the build parts, the templated launchers, the C ABI (include/vq_mi355x.h) of everything but the search
//   vq_search_plan.h     how a search is launched, as pure arithmetic on values (device, environment switches, call): the geometry
//                        shared with the kernels and the sizers, choose_search, plan_k_split / plan_main_tail / plan_residual_tail /
//                        plan_keys / the wide-row plans, and plan_call -> a CallPlan of at most two legs.  Plain C++17, included
//                        first (namespace vqi); tests/cabi/search_plan.cpp runs it alone on the CPU
//   vq_search_host.inc   the search's host side (included below, build part 0): the readers of the device, the environment and the
//                        call, the executor that walks a plan's legs, the search's C ABI
//   vq_sweep_host.inc    the host side of vq_gumbel.inc's roles (included in the C ABI block below, build part 0): one plan and
//                        workspace description, one codes-resident path, the Gumbel / reinmax / diversity / cross-entropy codes /
//                        orthogonal entries
//
// Reference lines replaced (relative to the reference root): vector_quantization/codebooks.py:386-397,
// utils/general.py:126-136,159-163, vector_quantize_pytorch.py:261-279,361-364, residual_vq.py:212-243; the decode side
// (vq_decode.inc): vector_quantize_pytorch.py:156-180, residual_vq.py:94-132,293-305; (vq_lfq_decode.inc):
// lookup_free_quantization.py:193-220, residual_lfq.py:80-118,240-252.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <type_traits>

#include "../../include/vq_mi355x.h"
#include "vq_search_plan.h"

// Build parts.  `hipcc ... vq_kernels.hip` (VQ_PART undefined) builds everything as ONE translation unit.  build.sh compiles
// the same file once per part (-DVQ_PART=n, in parallel) and links the objects: every part sees the same templates, but only
// its own launchers are defined -- and with them instantiated -- there; the other parts call them through the
// vqi::part_* entry points declared below.
//   0 C ABI, plan executor, small kernels (pack, scalar search, finalize, EMA, expiry, LFQ, FSQ, LQ, affine, decodes) 4 search Dp = 512 + wave-pair kernel
//   1 search Dp = 32 / 64         2 search Dp = 128                             5 similarity / softmax-statistics sweeps
//   3 search Dp = 256 + persistent kernel + full slices of wide rows            6 fused cross-entropy backward (+ live codes)
//   7 Gumbel straight-through backward sweeps               8 Gumbel-max sampling sweeps + Gumbel reinmax backward sweeps
//   9 codebook diversity loss sweeps                       10 orthogonal regularisation loss sweep
//  11 cross-entropy loss: the codes-gradient sweep
#ifndef VQ_PART
#define VQ_PART -1
#endif
#define VQ_OWN(part) (VQ_PART < 0 || VQ_PART == (part))

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
using namespace vqi;  // (vq_search_plan.h: the geometry the kernels share with the plans)

#include "vq_common.inc"
#if VQ_OWN(0)
#include "vq_pack.inc"
#endif
#include "vq_search.inc"
#include "vq_search_pair.inc"
#include "vq_search_persist.inc"
#include "vq_search_resident.inc"
#include "vq_sample.inc"
#include "vq_similarity.inc"
#include "vq_gumbel.inc"
#if VQ_OWN(0)
#include "vq_finalize_ema.inc"
#include "vq_rotate.inc"
#include "vq_expire.inc"
#include "vq_lfq.inc"
#include "vq_rlfq.inc"
#include "vq_fsq.inc"
#include "vq_lq.inc"
#include "vq_affine.inc"
#include "vq_decode.inc"
#include "vq_residual_mask.inc"
#include "vq_lfq_decode.inc"
#include "vq_diversity.inc"
#endif

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// (the launch plans: vq_search_plan.h; the executor that walks them and the search's C ABI: vq_search_host.inc)

template <int DP, int WAVES, int METRIC, int MULTI, bool LSE = false, int XT = 0, int WIDE = 0>
int launch_search_t(const SearchParams &p, int H, int splits, hipStream_t s) {
    using G = Geo<DP, WAVES>;
    const size_t lds = (size_t)(MULTI ? G::MAIN_FLOATS_M : G::MAIN_FLOATS_S) * 4 + (size_t)WAVES * p.Q * 32 * 4 +
                       ((MULTI && p.loss_part) ? (size_t)WAVES * p.Q * 64 * 4 : 0);
    if (lds > 160 * 1024) return fail(VQ_E_UNSUPPORTED, "vq_search: LDS budget exceeded (too many residual stages)");
    return launch<vq_search_mfma<DP, WAVES, METRIC, MULTI, LSE, XT, WIDE>, kBigLds>(
        dim3((unsigned)one_block_grid_x(p.M, WAVES), (unsigned)H, (unsigned)splits), dim3(WAVES * 64), lds, s, "vq_search_mfma launch", p);
}

// LDS bytes of a residual (multi-stage) launch with Q stages; the budget is the CU's 160 KiB
template <int DP, int WAVES>
constexpr size_t multi_lds_bytes(int Q, bool with_loss) {
    return (size_t)Geo<DP, WAVES>::MAIN_FLOATS_M * 4 + (size_t)WAVES * Q * 32 * 4 + (with_loss ? (size_t)WAVES * Q * 64 * 4 : 0);
}

template <int DP, int WAVES>
int max_stages_t(bool with_loss) {
    int q = 1;
    while (q < 4096 && multi_lds_bytes<DP, WAVES>(q + 1, with_loss) <= 160 * 1024) ++q;
    return q;
}

template <int DP, int WAVES>
int launch_search_m(const SearchParams &p, int H, int splits, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        if (p.Q > 1)  // residual stages: eval (1) and straight-through (2) arithmetic are separate instantiations
            return p.ste ? launch_search_t<DP, WAVES, ME, 2>(p, H, splits, s) : launch_search_t<DP, WAVES, ME, 1>(p, H, splits, s);
        if (p.xt == 1) return launch_search_t<DP, WAVES, ME, 0, false, 1>(p, H, splits, s);  // fp16 rows, widened in the prologue (inference)
        if (p.xt == 2) return launch_search_t<DP, WAVES, ME, 0, false, 2>(p, H, splits, s);  // bf16 rows
        if (p.lse) return launch_search_t<DP, WAVES, ME, 0, true>(p, H, splits, s);  // search + log-sum-exp in one sweep (cross-entropy commitment loss)
        return launch_search_t<DP, WAVES, ME, 0>(p, H, splits, s);
    });
}

// 256 < D <= 512: dims split over wave pairs (vq_search_pair.inc)
template <int METRIC, bool LSE = false, int XT = 0, int WIDE = 0, int MULTI = 0>
int launch_pair_t(const SearchParams &p, int H, int splits, hipStream_t s) {
    return launch<vq_search_pair512<METRIC, LSE, XT, WIDE, MULTI>, kBigLds>(dim3((unsigned)pair_grid_x(p.M), (unsigned)H, (unsigned)splits), dim3(512),
                                                                            PairGeo::lds_bytes(MULTI ? p.Q : 1), s, "vq_search_pair512 launch", p);
}

#if VQ_OWN(4)  // (not a template: defining it instantiates the wave-pair kernels)
int launch_pair_any(const SearchParams &p, int H, int splits, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        if (p.Q > 1)  // residual stacks: eval (1) and straight-through (2) arithmetic, as in launch_search_m
            return p.ste ? launch_pair_t<ME, false, 0, 0, 2>(p, H, splits, s) : launch_pair_t<ME, false, 0, 0, 1>(p, H, splits, s);
        if (p.xt == 1) return launch_pair_t<ME, false, 1>(p, H, splits, s);
        if (p.xt == 2) return launch_pair_t<ME, false, 2>(p, H, splits, s);
        if (p.lse) return launch_pair_t<ME, true>(p, H, splits, s);
        return launch_pair_t<ME>(p, H, splits, s);
    });
}
#endif

// the fp16 screen images of H codebooks from their fp32 packed images (the tiles' max |c'_i| first: the pack kernel derives the
// head's scales from them), and a zeroed control block behind them (a template, so that only the build part that launches it
// instantiates the kernels)
template <int DP>
int launch_pack_scr(const float *packed, long long pk_hs, int K, int ntiles, int H, char *img, long long img_hs, unsigned *ctrl, hipStream_t s) {
    if (int rc = launch<vq_scr_absmax_kernel<DP>>(dim3((unsigned)ntiles, (unsigned)H), dim3(256), 0, s, "vq_scr_absmax launch", packed, pk_hs, ntiles,
                                                  img, img_hs))
        return rc;
    return launch<vq_pack_scr_kernel<DP>>(dim3((unsigned)ntiles, (unsigned)H), dim3(256), 0, s, "vq_pack_scr launch", packed, pk_hs, K, ntiles, img,
                                           img_hs, ctrl);
}

template <int METRIC, bool TRAIN = false, bool SCREEN = false>
int launch_persist_t(const SearchParams &p, int H, int cus, hipStream_t s, bool scr_cached = false, bool resolve_split = true) {
    using G = Geo<256, 8>;
    const size_t lds = (size_t)G::MAIN_FLOATS_S * 4 + 2 * 8 * 32 * 4;
    if constexpr (SCREEN) {  // this call's images, unless the caller brought them (then the control block is clean: see the second pass)
        if (!scr_cached)
            if (int rc = launch_pack_scr<256>(p.packed, p.pk_hs, p.K, p.ntiles, H, (char *)p.scr, p.scr_hs, p.scr_count, s)) return rc;
    }
    if (int rc = launch<vq_search_persist<256, 8, METRIC, TRAIN, SCREEN>, kBigLds>(dim3((unsigned)persist_grid_x(p.M, H, cus), (unsigned)H, 1), dim3(512),
                                                                                   lds, s, "vq_search_persist launch", p))
        return rc;
    if constexpr (SCREEN) {
        // second pass: the rows of both lists, in stream order behind the sweep.  One workgroup per CU: the few full searches
        // of a usual call (tens) are split over several workgroups each, the other workgroups share the rescore batches, and
        // every workgroup stays for the exit ticket that leaves the control block clean (vq_resolve_rows_kernel).
        // `resolve_split` false (Switches::resolve_no_split): no split of the full searches
        const int flags = resolve_split ? 0 : kResolveNoSplit;
        return launch<vq_resolve_rows_kernel<256>, kBigLds>(dim3((unsigned)(cus > 0 ? cus : 1)), dim3(kResolveWaves * 64), resolve_lds_bytes<256>(), s,
                                                            "vq_resolve_rows launch", p, H, flags);
    }
    return 0;
}

// small codebooks: the image stays in LDS, one 8-wave workgroup per CU, waves walk 32-row blocks (vq_search_resident.inc)
template <int DP, int METRIC>
int launch_resident_t(const SearchParams &p, int H, int cus, hipStream_t s) {
    const size_t lds = resident_lds_bytes(p.res_img_floats, p.res_nbuf);
    const long long nwb = (p.M + 31) / 32;
    long long gx = cus / H;
    if (gx < 1) gx = 1;
    if (gx > (nwb + 7) / 8) gx = (nwb + 7) / 8;
    auto go = [&](auto multibuf) {
        return launch<vq_search_resident<DP, METRIC, decltype(multibuf)::value>, kBigLds>(dim3((unsigned)gx, (unsigned)H, 1), dim3(512), lds, s,
                                                                                          "vq_search_resident launch", p);
    };
    if constexpr (DP < 128) {
        if (p.res_nbuf > 1) return go(std::true_type{});  // a slab buffer per slab of a block
    }
    return go(std::false_type{});
}

template <int DP>
int launch_resident_m(const SearchParams &p, int H, int cus, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) { return launch_resident_t<DP, decltype(m)::value>(p, H, cus, s); });
}

template <int DP, int WAVES, int METRIC, int MODE>
int launch_aux_t(const AuxParams &p, int H, hipStream_t s) {
    return launch<vq_sweep_aux<DP, WAVES, METRIC, MODE>, kBigLds>(dim3((unsigned)one_block_grid_x(p.M, WAVES), (unsigned)H, 1), dim3(WAVES * 64),
                                                                  (size_t)Geo<DP, WAVES>::MAIN_FLOATS * 4, s, "vq_sweep_aux launch", p);
}

template <int DP, int WAVES>
int launch_aux_m(const AuxParams &p, int H, int metric, int mode, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        return mode == kAuxSims ? launch_aux_t<DP, WAVES, ME, kAuxSims>(p, H, s) : launch_aux_t<DP, WAVES, ME, kAuxStats>(p, H, s);
    });
}

template <int DP, int METRIC>
int launch_ce_bwd_t(const CeBwdParams &p, int H, hipStream_t s) {
    const size_t stage_floats = (size_t)4 * (32 * CeGeo<DP>::GS + 96), main_floats = (size_t)Geo<DP, 4>::MAIN_FLOATS;
    return launch<vq_ce_backward<DP, METRIC>, kBigLds>(dim3((unsigned)((p.M + 127) / 128), (unsigned)H, (unsigned)CeGeo<DP>::NH), dim3(256),
                                                       4 * (main_floats > stage_floats ? main_floats : stage_floats), s, "vq_ce_backward launch", p);
}

// Dp = 256: the two contractions on a pair of waves (two waves per SIMD); VQ_CE_NO_ROLES=1 keeps the one-wave kernel (A/B runs)
template <int METRIC>
int launch_ce_bwd_roles_t(const CeBwdParams &p, int H, hipStream_t s) {
    return launch<vq_ce_backward_roles<METRIC>, kBigLds>(dim3((unsigned)((p.M + 32 * CeRolesGeo::NB - 1) / (32 * CeRolesGeo::NB)), (unsigned)H, 1),
                                                         dim3(512), (size_t)CeRolesGeo::LDS_F * 4, s, "vq_ce_backward_roles launch", p);
}

// Dp = 512: four roles per row block (S cut in two, G in two halves of the positions), 64 rows per workgroup
template <int METRIC>
int launch_ce_bwd_roles512_t(const CeBwdParams &p, int H, hipStream_t s) {
    return launch<vq_ce_backward_roles512<METRIC>, kBigLds>(dim3((unsigned)((p.M + 32 * CeRoles512Geo::NQ - 1) / (32 * CeRoles512Geo::NQ)), (unsigned)H, 1),
                                                            dim3(512), (size_t)CeRoles512Geo::LDS_F * 4, s, "vq_ce_backward_roles512 launch", p);
}

template <int DP>
int launch_ce_bwd_m(const CeBwdParams &p, int H, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        if constexpr (DP == 256 || DP == 512) {
            if (getenv("VQ_CE_NO_ROLES") == nullptr) {  // (read per call: tests switch between the two kernels in one process)
                if constexpr (DP == 512) return launch_ce_bwd_roles512_t<ME>(p, H, s);
                else return launch_ce_bwd_roles_t<ME>(p, H, s);
            }
        }
        return launch_ce_bwd_t<DP, ME>(p, H, s);
    });
}

// live codes (Dp <= 256): the one-wave body with a second tile ring, whatever VQ_CE_NO_ROLES says
template <int DP>
int launch_ce_bwd_live_m(const CeBwdLiveParams &p, int H, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        constexpr int rows = 32 * CeLiveGeo<DP>::WAVES;
        return launch<vq_ce_backward<DP, ME, true, CeLiveGeo<DP>::WAVES>, kBigLds>(dim3((unsigned)((p.M + rows - 1) / rows), (unsigned)H, 1),
                                                                                   dim3(CeLiveGeo<DP>::WAVES * 64), CeLiveGeo<DP>::LDS_B, s,
                                                                                   "vq_ce_backward (live) launch", p);
    });
}

// Gumbel-max sampling: the kAuxSample epilogue, a build part of its own
template <int DP>
int launch_sample_m(const AuxParams &p, int H, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) { return launch_aux_t<DP, 4, decltype(m)::value, kAuxSample>(p, H, s); });
}

// the Gumbel backward sweeps: `gz` = row splits of kGumC
template <int DP, int METRIC, int ROLE>
int launch_gumbel_t(const GumbelParams &p, int H, int gz, hipStream_t s) {
    using G = Geo<DP, 4>;
    using GG = GumGeo<DP>;
    constexpr SweepRole R = sweep_role(ROLE);  // (the table the kernel reads: the LDS below is what ITS switches use)
    // packed x rows and packed g rows; kDivX: the searched codes and, given at run time, the live codes
    const bool two_images = R.second_image || (ROLE == kDivX && p.gimg);
    const size_t tile_floats = (size_t)(two_images ? 2 : 1) * 2 * G::BUF_F4 * 4, rows_floats = (size_t)4 * 32 * G::XS;
    const size_t stage_floats = R.no_contraction ? 0 : (size_t)4 * (32 * GG::GS + 32);  // the finalize staging
    size_t floats = tile_floats > rows_floats ? tile_floats : rows_floats;
    if (stage_floats > floats) floats = stage_floats;
    return launch<vq_gumbel_sweep<DP, METRIC, ROLE>, kBigLds>(dim3((unsigned)((p.NR + 127) / 128), (unsigned)H, (unsigned)gz),
                                                              dim3(256), floats * 4, s, "vq_gumbel_sweep launch", p);
}

template <int DP>
int launch_gumbel_m(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        if (role == kGumStats) return launch_gumbel_t<DP, ME, kGumStats>(p, H, 1, s);
        if (role == kGumX) return launch_gumbel_t<DP, ME, kGumX>(p, H, 1, s);
        return launch_gumbel_t<DP, ME, kGumC>(p, H, gz, s);
    });
}

// the reinmax roles of the same sweep: a build part of their own entry point
template <int DP>
int launch_reinmax_m(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        if (role == kRmStats) return launch_gumbel_t<DP, ME, kRmStats>(p, H, 1, s);
        if (role == kRmCol) return launch_gumbel_t<DP, ME, kRmCol>(p, H, gz, s);
        if (role == kRmX) return launch_gumbel_t<DP, ME, kRmX>(p, H, 1, s);
        return launch_gumbel_t<DP, ME, kRmC>(p, H, gz, s);
    });
}

// the diversity roles of the same sweep: a build part of their own
template <int DP>
int launch_diversity_m(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        if (role == kDivStats) return launch_gumbel_t<DP, ME, kDivStats>(p, H, 1, s);
        if (role == kDivAcc) return launch_gumbel_t<DP, ME, kDivAcc>(p, H, gz, s);
        if (role == kDivDelta) return launch_gumbel_t<DP, ME, kDivDelta>(p, H, 1, s);
        if (role == kDivC) return launch_gumbel_t<DP, ME, kDivC>(p, H, gz, s);
        return launch_gumbel_t<DP, ME, kDivX>(p, H, 1, s);
    });
}

// the cross-entropy role of the same sweep (the gradient with respect to a learnable codebook): a build part of its own
template <int DP>
int launch_ce_codes_m(const GumbelParams &p, int H, int gz, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) { return launch_gumbel_t<DP, decltype(m)::value, kCeC>(p, H, gz, s); });
}

// the orthogonal role of the same sweep (dot metric only): a build part of its own
template <int DP>
int launch_orthogonal_m(const GumbelParams &p, int H, hipStream_t s) {
    return launch_gumbel_t<DP, VQ_METRIC_DOT, kOrth>(p, H, 1, s);
}

// one slice of rows wider than 512 dims: WIDE = 1 a full slice (Dp = the slice width only), 2 / 3 the last slice
template <int DP>
int launch_wide_any(int wide, const SearchParams &p, int H, int splits, int metric, hipStream_t s) {
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        if (wide == 1) {
            if constexpr (DP >= 256) return launch_search_t<DP, kWideWaves, ME, 0, false, 0, 1>(p, H, splits, s);
            else return fail(VQ_E_UNSUPPORTED, "vq_search: a full slice of wide rows is 256 (or 512) dims");
        }
        return wide == 3 ? launch_search_t<DP, kWideWaves, ME, 0, false, 0, 3>(p, H, splits, s)
                         : launch_search_t<DP, kWideWaves, ME, 0, false, 0, 2>(p, H, splits, s);
    });
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// entry points of the build parts: declared everywhere, defined (= their kernels instantiated) in the owning part only
// ------------------------------------------------------------------------------------------------
namespace vqi {
template <int DP> int part_search(int waves, const SearchParams &p, int H, int splits, int metric, hipStream_t s);
template <int DP> int part_wide(int wide, bool pairs, const SearchParams &p, int H, int splits, int metric, hipStream_t s);
template <int DP> int part_resident(const SearchParams &p, int H, int cus, int metric, hipStream_t s);
template <int DP> int part_aux(const AuxParams &p, int H, int metric, int mode, hipStream_t s);
template <int DP> int part_ce_bwd(const CeBwdParams &p, int H, int metric, hipStream_t s);
template <int DP> int part_sample(const AuxParams &p, int H, int metric, hipStream_t s);
template <int DP> int part_gumbel(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s);
template <int DP> int part_reinmax(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s);
template <int DP> int part_diversity(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s);
template <int DP> int part_orthogonal(const GumbelParams &p, int H, hipStream_t s);
template <int DP> int part_ce_codes(const GumbelParams &p, int H, int gz, int metric, hipStream_t s);
#define VQ_DECLARE_GUMBEL_PARTS(DP)                                                                              \
    template <> int part_gumbel<DP>(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s); \
    template <> int part_reinmax<DP>(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s);  \
    template <> int part_diversity<DP>(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s); \
    template <> int part_orthogonal<DP>(const GumbelParams &p, int H, hipStream_t s);                              \
    template <> int part_ce_codes<DP>(const GumbelParams &p, int H, int gz, int metric, hipStream_t s);
template <int DP> int part_ce_bwd_live(const CeBwdLiveParams &p, int H, int metric, hipStream_t s);
template <> int part_ce_bwd_live<32>(const CeBwdLiveParams &p, int H, int metric, hipStream_t s);
template <> int part_ce_bwd_live<64>(const CeBwdLiveParams &p, int H, int metric, hipStream_t s);
template <> int part_ce_bwd_live<128>(const CeBwdLiveParams &p, int H, int metric, hipStream_t s);
template <> int part_ce_bwd_live<256>(const CeBwdLiveParams &p, int H, int metric, hipStream_t s);
VQ_DECLARE_GUMBEL_PARTS(32)
VQ_DECLARE_GUMBEL_PARTS(64)
VQ_DECLARE_GUMBEL_PARTS(128)
VQ_DECLARE_GUMBEL_PARTS(256)
#undef VQ_DECLARE_GUMBEL_PARTS
int part_pair(const SearchParams &p, int H, int splits, int metric, hipStream_t s);
int part_persist(const SearchChoice &c, const SearchParams &p, int H, int cus, int metric, hipStream_t s);
int part_pack_scr(const float *packed, long long pk_hs, int K, int ntiles, int H, char *img, long long img_hs, unsigned *ctrl, hipStream_t s);
#define VQ_DECLARE_PARTS(DP)                                                                                         \
    template <> int part_search<DP>(int waves, const SearchParams &p, int H, int splits, int metric, hipStream_t s); \
    template <> int part_wide<DP>(int wide, bool pairs, const SearchParams &p, int H, int splits, int metric, hipStream_t s); \
    template <> int part_aux<DP>(const AuxParams &p, int H, int metric, int mode, hipStream_t s);                    \
    template <> int part_ce_bwd<DP>(const CeBwdParams &p, int H, int metric, hipStream_t s);                          \
    template <> int part_sample<DP>(const AuxParams &p, int H, int metric, hipStream_t s);
template <> int part_resident<32>(const SearchParams &p, int H, int cus, int metric, hipStream_t s);
template <> int part_resident<64>(const SearchParams &p, int H, int cus, int metric, hipStream_t s);
template <> int part_resident<128>(const SearchParams &p, int H, int cus, int metric, hipStream_t s);
VQ_DECLARE_PARTS(32)
VQ_DECLARE_PARTS(64)
VQ_DECLARE_PARTS(128)
VQ_DECLARE_PARTS(256)
VQ_DECLARE_PARTS(512)
#undef VQ_DECLARE_PARTS

#define VQ_DEFINE_SEARCH_PART(DP, W4)                                                                                 \
    template <> int part_search<DP>(int waves, const SearchParams &p, int H, int splits, int metric, hipStream_t s) { \
        return waves == 8 ? launch_search_m<DP, 8>(p, H, splits, metric, s) : launch_search_m<DP, W4>(p, H, splits, metric, s); \
    }                                                                                                                 \
    template <> int part_wide<DP>(int wide, bool, const SearchParams &p, int H, int splits, int metric, hipStream_t s) { \
        return launch_wide_any<DP>(wide, p, H, splits, metric, s);                                                    \
    }
#define VQ_DEFINE_RESIDENT_PART(DP) \
    template <> int part_resident<DP>(const SearchParams &p, int H, int cus, int metric, hipStream_t s) { return launch_resident_m<DP>(p, H, cus, metric, s); }
#if VQ_OWN(1)
VQ_DEFINE_SEARCH_PART(32, 4)
VQ_DEFINE_SEARCH_PART(64, 4)
VQ_DEFINE_RESIDENT_PART(32)
VQ_DEFINE_RESIDENT_PART(64)
#endif
#if VQ_OWN(2)
VQ_DEFINE_SEARCH_PART(128, 4)
VQ_DEFINE_RESIDENT_PART(128)
#endif
#undef VQ_DEFINE_RESIDENT_PART
#if VQ_OWN(3)
VQ_DEFINE_SEARCH_PART(256, 4)
int part_persist(const SearchChoice &c, const SearchParams &p, int H, int cus, int metric, hipStream_t s) {
    if (c.screened) return launch_persist_t<VQ_METRIC_EUCLID, false, true>(p, H, cus, s, c.cached, c.resolve_split);  // (choose_search: Euclid inference calls)
    return with_metric(metric, [&](auto m) {
        constexpr int ME = decltype(m)::value;
        return c.train ? launch_persist_t<ME, true>(p, H, cus, s) : launch_persist_t<ME>(p, H, cus, s);
    });
}
int part_pack_scr(const float *packed, long long pk_hs, int K, int ntiles, int H, char *img, long long img_hs, unsigned *ctrl, hipStream_t s) {
    return launch_pack_scr<256>(packed, pk_hs, K, ntiles, H, img, img_hs, ctrl, s);
}
#endif
#if VQ_OWN(4)
template <> int part_search<512>(int, const SearchParams &p, int H, int splits, int metric, hipStream_t s) {
    return launch_search_m<512, 4>(p, H, splits, metric, s);
}
template <> int part_wide<512>(int wide, bool pairs, const SearchParams &p, int H, int splits, int metric, hipStream_t s) {
#if VQ_EXP_WIDE_SLICE == 512
    // a 512-dim slice of wider rows: the wave-pair kernel (two waves per SIMD, accumulator hand-off) when the sweep is long
    // enough for its extra pipeline step (`pairs`: pairs_worth_it), else the one-wave kernel
    if (pairs)
        return with_metric(metric, [&](auto m) {
            constexpr int ME = decltype(m)::value;
            if (wide == 1) return launch_pair_t<ME, false, 0, 1>(p, H, splits, s);
            if (wide == 3) return launch_pair_t<ME, false, 0, 3>(p, H, splits, s);
            return launch_pair_t<ME, false, 0, 2>(p, H, splits, s);
        });
    return launch_wide_any<512>(wide, p, H, splits, metric, s);
#else
    (void)wide; (void)pairs; (void)p; (void)H; (void)splits; (void)metric; (void)s;
    return fail(VQ_E_UNSUPPORTED, "vq_search: unsupported padded dim");
#endif
}
int part_pair(const SearchParams &p, int H, int splits, int metric, hipStream_t s) { return launch_pair_any(p, H, splits, metric, s); }
#endif
#undef VQ_DEFINE_SEARCH_PART
#if VQ_OWN(5)
#define VQ_DEFINE_AUX_PART(DP) \
    template <> int part_aux<DP>(const AuxParams &p, int H, int metric, int mode, hipStream_t s) { return launch_aux_m<DP, 4>(p, H, metric, mode, s); }
VQ_DEFINE_AUX_PART(32)
VQ_DEFINE_AUX_PART(64)
VQ_DEFINE_AUX_PART(128)
VQ_DEFINE_AUX_PART(256)
VQ_DEFINE_AUX_PART(512)
#undef VQ_DEFINE_AUX_PART
#endif
#if VQ_OWN(6)
#define VQ_DEFINE_CE_PART(DP) \
    template <> int part_ce_bwd<DP>(const CeBwdParams &p, int H, int metric, hipStream_t s) { return launch_ce_bwd_m<DP>(p, H, metric, s); }
VQ_DEFINE_CE_PART(32)
VQ_DEFINE_CE_PART(64)
VQ_DEFINE_CE_PART(128)
VQ_DEFINE_CE_PART(256)
VQ_DEFINE_CE_PART(512)
#undef VQ_DEFINE_CE_PART
#define VQ_DEFINE_CE_LIVE_PART(DP) \
    template <> int part_ce_bwd_live<DP>(const CeBwdLiveParams &p, int H, int metric, hipStream_t s) { return launch_ce_bwd_live_m<DP>(p, H, metric, s); }
VQ_DEFINE_CE_LIVE_PART(32)
VQ_DEFINE_CE_LIVE_PART(64)
VQ_DEFINE_CE_LIVE_PART(128)
VQ_DEFINE_CE_LIVE_PART(256)
#undef VQ_DEFINE_CE_LIVE_PART
#endif
#if VQ_OWN(7)
#define VQ_DEFINE_GUMBEL_PART(DP) \
    template <> int part_gumbel<DP>(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s) { return launch_gumbel_m<DP>(role, p, H, gz, metric, s); }
VQ_DEFINE_GUMBEL_PART(32)
VQ_DEFINE_GUMBEL_PART(64)
VQ_DEFINE_GUMBEL_PART(128)
VQ_DEFINE_GUMBEL_PART(256)
#undef VQ_DEFINE_GUMBEL_PART
#endif
#if VQ_OWN(8)
#define VQ_DEFINE_SAMPLE_PART(DP) \
    template <> int part_sample<DP>(const AuxParams &p, int H, int metric, hipStream_t s) { return launch_sample_m<DP>(p, H, metric, s); }
VQ_DEFINE_SAMPLE_PART(32)
VQ_DEFINE_SAMPLE_PART(64)
VQ_DEFINE_SAMPLE_PART(128)
VQ_DEFINE_SAMPLE_PART(256)
VQ_DEFINE_SAMPLE_PART(512)
#undef VQ_DEFINE_SAMPLE_PART
#define VQ_DEFINE_REINMAX_PART(DP) \
    template <> int part_reinmax<DP>(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s) { return launch_reinmax_m<DP>(role, p, H, gz, metric, s); }
VQ_DEFINE_REINMAX_PART(32)
VQ_DEFINE_REINMAX_PART(64)
VQ_DEFINE_REINMAX_PART(128)
VQ_DEFINE_REINMAX_PART(256)
#undef VQ_DEFINE_REINMAX_PART
#endif
#if VQ_OWN(9)
#define VQ_DEFINE_DIVERSITY_PART(DP) \
    template <> int part_diversity<DP>(int role, const GumbelParams &p, int H, int gz, int metric, hipStream_t s) { return launch_diversity_m<DP>(role, p, H, gz, metric, s); }
VQ_DEFINE_DIVERSITY_PART(32)
VQ_DEFINE_DIVERSITY_PART(64)
VQ_DEFINE_DIVERSITY_PART(128)
VQ_DEFINE_DIVERSITY_PART(256)
#undef VQ_DEFINE_DIVERSITY_PART
#endif
#if VQ_OWN(10)
#define VQ_DEFINE_ORTHOGONAL_PART(DP) \
    template <> int part_orthogonal<DP>(const GumbelParams &p, int H, hipStream_t s) { return launch_orthogonal_m<DP>(p, H, s); }
VQ_DEFINE_ORTHOGONAL_PART(32)
VQ_DEFINE_ORTHOGONAL_PART(64)
VQ_DEFINE_ORTHOGONAL_PART(128)
VQ_DEFINE_ORTHOGONAL_PART(256)
#undef VQ_DEFINE_ORTHOGONAL_PART
#endif
#if VQ_OWN(11)
#define VQ_DEFINE_CE_CODES_PART(DP) \
    template <> int part_ce_codes<DP>(const GumbelParams &p, int H, int gz, int metric, hipStream_t s) { return launch_ce_codes_m<DP>(p, H, gz, metric, s); }
VQ_DEFINE_CE_CODES_PART(32)
VQ_DEFINE_CE_CODES_PART(64)
VQ_DEFINE_CE_CODES_PART(128)
VQ_DEFINE_CE_CODES_PART(256)
#undef VQ_DEFINE_CE_CODES_PART
#endif
}  // namespace vqi

#if VQ_OWN(0)
namespace vqi {
thread_local char g_err[512] = "";
}
namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// 16-byte (float4) accesses: the pointer aligned to `align` bytes (16; 8 for 2-byte rows) and every stride -- or extent that
// acts as one -- a multiple of 4 elements
bool vec4_ok(const void *p, std::initializer_list<long long> strides, unsigned align = 16) {
    for (const long long st : strides)
        if (st % 4) return false;
    return ((uintptr_t)p & (align - 1)) == 0;
}

int launch_aux(int DP, const AuxParams &p, int H, int metric, int mode, hipStream_t s) {
    return with_padded_dim(DP, [&](auto dp) { return vqi::part_aux<decltype(dp)::value>(p, H, metric, mode, s); },
                           [] { return fail(VQ_E_UNSUPPORTED, "vq_sweep_aux: unsupported padded dim"); });
}

int check_common(const vq_args *a) {
    if (!a) return fail(VQ_E_BADARG, "vq: null args");
    if (a->H <= 0 || a->Q <= 0 || a->M < 0 || a->K <= 0 || a->D <= 0) return fail(VQ_E_BADARG, "vq: non-positive size");
    if (a->metric != VQ_METRIC_EUCLID && a->metric != VQ_METRIC_DOT) return fail(VQ_E_BADARG, "vq: unknown metric");
    if (!a->x && a->M > 0) return fail(VQ_E_BADARG, "vq: x is null");
    return 0;
}

}  // namespace

#include "vq_search_host.inc"

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char *vq_last_error(void) { return g_err; }

#ifdef VQ_EXP_STAMPS
int vq_debug_read_stamps(unsigned long long *host, size_t n) {  // diagnostic build only
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), n * sizeof(unsigned long long));
}
#endif

#ifdef VQ_EXP_SCREEN_COUNT
int vq_debug_screen_rows(unsigned long long *host2, int reset) {  // diagnostic build only (single translation unit): {rows listed for the full search of the second pass, rows, rows rescored}
    hipError_t e = hipMemcpyFromSymbol(host2, HIP_SYMBOL(g_scr_rows), 3 * sizeof(unsigned long long));
    if (e == hipSuccess && reset) {
        const unsigned long long z[3] = {0, 0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_scr_rows), z, sizeof(z));
    }
    return (int)e;
}
#endif

int vq_device_info(char *buf, size_t n) {
    const DevInfo &di = dev_info();
    if (!di.ok) return fail(VQ_E_NODEVICE, "vq: no HIP device");
    snprintf(buf, n, "%s %d CUs", di.name, di.cus);
    return 0;
}

int64_t vq_packed_floats(int K, int D) {
    if (K <= 0 || D <= 0) return 0;
    const int DP = padded_dim(D);
    if (DP == 0)  // one image per slice, the last one in the layout of its own (padded) width
        return (int64_t)((D - 1) / kWideSlice) * wide_image_floats(K) + wide_last_image_floats(K, D);
    return (int64_t)round_up(K, kTileCodes * sub_tiles(DP)) * (DP + 4) + kPackSlack;
}

int64_t vq_workspace_bytes_wide(int H, int64_t M, int K, int D) {
    if (H <= 0 || M < 0 || K <= 0 || D <= 0) return 0;
    if (padded_dim(D) != 0 || M == 0) return workspace_bytes(H, M, 1);
    return wide_workspace_bytes(H, M, wide_plan(H, M, K, D));
}

int64_t vq_workspace_bytes(int H, int64_t M, int Q) {
    if (H <= 0 || M < 0 || Q <= 0) return 0;
    // (+ residual stacks of many rows: room for the residual rows of a tail run stage by stage, see plan_residual_tail)
    return workspace_bytes(H, M, Q);
}

int64_t vq_screen_image_bytes(int H, int K, int D, int metric) {
    if (H <= 0 || K <= 0 || D <= 0 || metric != VQ_METRIC_EUCLID || padded_dim(D) != 256) return 0;
    const int ntiles = tiles_of(K, 256), nsub = ntiles * sub_tiles(256);
    if (nsub < kPersistMinSub || nsub > kPersistMaxSub) return 0;
    return screen_image_bytes(H, ntiles);
}

int vq_pack_screen_image_f32(const float *packed, int H, int64_t pk_hs, int K, int D, int metric, void *screen, int64_t screen_bytes,
                             void *stream) {
    const int64_t need = vq_screen_image_bytes(H, K, D, metric);
    if (need == 0) return fail(VQ_E_UNSUPPORTED, "vq_pack_screen_image: no screened sweep for this shape (see vq_screen_image_bytes)");
    if (!packed || !screen || screen_bytes != need || !aligned16(packed) || !aligned16(screen) || pk_hs < vq_packed_floats(K, D))
        return fail(VQ_E_BADARG, "vq_pack_screen_image: bad argument");
    const int ntiles = tiles_of(K, 256);
    const long long img = scr_image_bytes(ntiles);
    return vqi::part_pack_scr(packed, pk_hs, K, ntiles, H, (char *)screen, img, (unsigned *)((char *)screen + (long long)H * img),
                              (hipStream_t)stream);
}

int vq_pack_codebooks_f32(const float *cb, int n_codebooks, int64_t cb_stride, int K, int D, int metric, float *packed,
                          void *stream) {
    if (!cb || !packed || n_codebooks <= 0 || K <= 0 || D <= 0) return fail(VQ_E_BADARG, "vq_pack: bad argument");
    if (metric != VQ_METRIC_EUCLID && metric != VQ_METRIC_DOT) return fail(VQ_E_BADARG, "vq_pack: unknown metric");
    const int DP = padded_dim(D);
    if (!aligned16(packed)) return fail(VQ_E_BADARG, "vq_pack: packed buffer must be 16-byte aligned");
    const long long pk_stride = vq_packed_floats(K, D);
    hipStream_t s = (hipStream_t)stream;
    if (DP == 0) {  // rows wider than 512 dims: one image per slice
        const int nd = (D + kWideSlice - 1) / kWideSlice;
        for (int j = 0; j < nd; ++j) {
            const int dp = (j + 1 == nd) ? padded_dim(wide_last_dims(D)) : kWideSlice;
            const int Kp = round_up(K, kTileCodes * sub_tiles(dp));
            if (int rc = launch<vq_pack_kernel>(dim3(Kp / 64 + 1, n_codebooks), dim3(64), 0, s, "vq_pack launch", cb, (long long)cb_stride, K, Kp, D,
                                                j * kWideSlice, dp, metric, packed + (long long)j * wide_image_floats(K), pk_stride))
                return rc;
        }
        return launch<vq_pack_flag_kernel>(dim3(n_codebooks), dim3(256), 0, s, "vq_pack launch", packed, pk_stride, K, kWideSlice + 4, kWideSlice, nd,
                                           wide_image_floats(K), wide_last_image_floats(K, D));
    }
    const int Kp = round_up(K, kTileCodes * sub_tiles(DP));
    // grid covers Kp rows plus at least one extra block whose threads zero the over-copy slack
    if (int rc = launch<vq_pack_kernel>(dim3(Kp / 64 + 1, n_codebooks), dim3(64), 0, s, "vq_pack launch", cb, (long long)cb_stride, K, Kp, D, 0, DP,
                                        metric, packed, pk_stride))
        return rc;
    return launch<vq_pack_flag_kernel>(dim3(n_codebooks), dim3(256), 0, s, "vq_pack launch", packed, pk_stride, K, DP + 4, DP, 1, pk_stride,
                                       (long long)vq_packed_floats(K, D));
}

int vq_quantize_backward_f32(const vq_args *a, const float *grad_out, int64_t go_rs, int64_t go_hs, const double *grad_sq_err,
                             float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    if (!a->cb || !a->idx || !grad_x) return fail(VQ_E_BADARG, "vq_quantize_backward: cb / idx / grad_x is null");
    QuantBwdParams p;
    memset(&p, 0, sizeof(p));
    p.x = a->x; p.x_rs = a->x_rs; p.x_hs = a->x_hs;
    p.cb = a->cb; p.cb_hs = a->cb_hs; p.cb_qs = a->cb_qs;
    p.idx = (const long long *)a->idx; p.idx_rs = a->idx_rs; p.idx_hs = a->idx_hs; p.idx_qs = a->idx_qs;
    p.go = grad_out; p.go_rs = go_rs; p.go_hs = go_hs;
    p.g_err = grad_sq_err;
    p.g_err_hs = (a->flags & VQ_F_SQERR_PER_HEAD) ? a->Q : 0;
    p.gx = grad_x; p.gx_rs = gx_rs; p.gx_hs = gx_hs;
    p.M = a->M; p.D = a->D; p.Q = a->Q; p.ste = (a->flags & VQ_F_STE) ? 1 : 0;
    p.vec = (vec4_ok(a->x, {a->D, a->x_rs, a->x_hs}) && vec4_ok(grad_x, {gx_rs, gx_hs}) && vec4_ok(a->cb, {a->cb_hs, a->cb_qs}) &&
             (!grad_out || vec4_ok(grad_out, {go_rs, go_hs}))) ? 1 : 0;
    long long blocks = (a->M + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    return launch<vq_quantize_backward_kernel>(dim3((unsigned)blocks, (unsigned)a->H), dim3(256), 0, (hipStream_t)stream, "vq_quantize_backward launch", p);
}

int vq_rotate_backward_f32(const vq_args *a, const float *grad_out, int64_t go_rs, int64_t go_hs, const double *grad_sq_err,
                           float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    if (!a->cb || !a->idx || !grad_x) return fail(VQ_E_BADARG, "vq_rotate_backward: cb / idx / grad_x is null");
    if (a->D > kRotateMaxDim) return fail(VQ_E_UNSUPPORTED, "vq_rotate_backward: rows of more than 1024 dims (the row is held in registers)");
    QuantBwdParams p;
    memset(&p, 0, sizeof(p));
    p.x = a->x; p.x_rs = a->x_rs; p.x_hs = a->x_hs;
    p.cb = a->cb; p.cb_hs = a->cb_hs; p.cb_qs = a->cb_qs;
    p.idx = (const long long *)a->idx; p.idx_rs = a->idx_rs; p.idx_hs = a->idx_hs; p.idx_qs = a->idx_qs;
    p.go = grad_out; p.go_rs = go_rs; p.go_hs = go_hs;
    p.g_err = grad_sq_err;
    p.g_err_hs = (a->flags & VQ_F_SQERR_PER_HEAD) ? a->Q : 0;
    p.gx = grad_x; p.gx_rs = gx_rs; p.gx_hs = gx_hs;
    p.M = a->M; p.D = a->D; p.Q = a->Q; p.ste = (a->flags & VQ_F_STE) ? 1 : 0;
    p.vec = (vec4_ok(a->x, {a->D, a->x_rs, a->x_hs}) && vec4_ok(grad_x, {gx_rs, gx_hs}) && vec4_ok(a->cb, {a->cb_hs, a->cb_qs}) &&
             (!grad_out || vec4_ok(grad_out, {go_rs, go_hs}))) ? 1 : 0;
    long long blocks = (a->M + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    const dim3 grid((unsigned)blocks, (unsigned)a->H);
    hipStream_t s = (hipStream_t)stream;
    const char *what = "vq_rotate_backward launch";
    // the row in registers: N slots of V per lane, the smallest variant that holds D
    const int slots = p.vec ? (a->D + 255) / 256 : (a->D + 63) / 64;
    if (p.vec) {
        if (slots <= 1) return launch<vq_rotate_backward_kernel<f32x4, 1>>(grid, dim3(256), 0, s, what, p);
        if (slots <= 2) return launch<vq_rotate_backward_kernel<f32x4, 2>>(grid, dim3(256), 0, s, what, p);
        return launch<vq_rotate_backward_kernel<f32x4, 4>>(grid, dim3(256), 0, s, what, p);
    }
    if (slots <= 1) return launch<vq_rotate_backward_kernel<float, 1>>(grid, dim3(256), 0, s, what, p);
    if (slots <= 2) return launch<vq_rotate_backward_kernel<float, 2>>(grid, dim3(256), 0, s, what, p);
    if (slots <= 4) return launch<vq_rotate_backward_kernel<float, 4>>(grid, dim3(256), 0, s, what, p);
    if (slots <= 8) return launch<vq_rotate_backward_kernel<float, 8>>(grid, dim3(256), 0, s, what, p);
    return launch<vq_rotate_backward_kernel<float, 16>>(grid, dim3(256), 0, s, what, p);
}

// Owner-computes launch plan: a wave owns cw codes (8 KiB of partial sums) and one of row_blocks contiguous row ranges
struct EmaOwnerPlan {
    int cw;
    long long owners, row_blocks, rows_per_block;
    size_t lds;
};

static bool ema_owner_plan(int H, long long M, int K, int D, EmaOwnerPlan &pl) {
    if (D > 2048) return false;
    const int D4 = (D + 3) & ~3;
    int cw = 2048 / D4;
    if (cw > 64) cw = 64;
    if (cw > K) cw = K;
    pl.cw = cw;
    pl.owners = (K + cw - 1) / cw;
    long long row_blocks = (16ll * device_cus()) / (pl.owners * H);  // ~16 waves per CU in total
    if (row_blocks < 1) row_blocks = 1;
    long long rows_per_block = (M + row_blocks - 1) / row_blocks;
    if (rows_per_block < 2048) rows_per_block = 2048;
    rows_per_block = (rows_per_block + 63) / 64 * 64;
    pl.rows_per_block = rows_per_block;
    pl.row_blocks = (M + rows_per_block - 1) / rows_per_block;
    const size_t per_wave = (size_t)cw * D4 + ((cw + 3) & ~3) + 64 * 2 + 64;
    pl.lds = per_wave * 4 * 4;
    return true;
}

static int launch_ema_owner(const EmaOwnerPlan &pl, const float *x, int64_t x_rs, int64_t x_hs, const int64_t *idx, int64_t idx_rs,
                            int64_t idx_hs, const uint8_t *mask, int H, int64_t M, int K, int D, float *counts, float *sums,
                            float *part_sums, float *part_counts, hipStream_t s) {
    return launch<vq_ema_accumulate_owner_kernel, kBigLds>(dim3((unsigned)((pl.owners + 3) / 4), (unsigned)pl.row_blocks, (unsigned)H), dim3(256), pl.lds, s,
                                                           "vq_ema_accumulate_owner launch", x, (long long)x_rs, (long long)x_hs, (const long long *)idx,
                                                           (long long)idx_rs, (long long)idx_hs, mask, (long long)M, pl.rows_per_block, K, pl.cw, D, counts,
                                                           sums, part_sums, part_counts);
}

int vq_ema_accumulate_f32(const float *x, int64_t x_rs, int64_t x_hs, const int64_t *idx, int64_t idx_rs, int64_t idx_hs,
                          const uint8_t *mask, int H, int64_t M, int K, int D, float *counts, float *sums, void *stream) {
    if (H <= 0 || M < 0 || K <= 0 || D <= 0 || !counts || !sums) return fail(VQ_E_BADARG, "vq_ema_accumulate: bad argument");
    if (M == 0) return 0;
    if (!x || !idx) return fail(VQ_E_BADARG, "vq_ema_accumulate: null input");
    hipStream_t s = (hipStream_t)stream;
    // Owner-computes path: worth it when each owner sees many rows
    EmaOwnerPlan pl;
    if (ema_owner_plan(H, M, K, D, pl) && M / pl.owners >= 1024)
        return launch_ema_owner(pl, x, x_rs, x_hs, idx, idx_rs, idx_hs, mask, H, M, K, D, counts, sums, nullptr, nullptr, s);
    long long blocks = (M + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    return launch<vq_ema_accumulate_kernel>(dim3((unsigned)blocks, (unsigned)H), dim3(256), 0, s, "vq_ema_accumulate launch", x, (long long)x_rs,
                                            (long long)x_hs, (const long long *)idx, (long long)idx_rs, (long long)idx_hs, mask, (long long)M, K, D, counts,
                                            sums);
}

int64_t vq_ema_det_workspace_bytes(int H, int64_t M, int K, int D) {
    EmaOwnerPlan pl;
    if (H <= 0 || M <= 0 || K <= 0 || D <= 0 || !ema_owner_plan(H, M, K, D, pl)) return 0;
    return pl.row_blocks * H * (int64_t)K * (D + 1) * 4 + 256;
}

int vq_ema_accumulate_det_f32(const float *x, int64_t x_rs, int64_t x_hs, const int64_t *idx, int64_t idx_rs, int64_t idx_hs,
                              const uint8_t *mask, int H, int64_t M, int K, int D, float *counts, float *sums, void *workspace,
                              int64_t workspace_bytes, void *stream) {
    if (H <= 0 || M < 0 || K <= 0 || D <= 0 || !counts || !sums) return fail(VQ_E_BADARG, "vq_ema_accumulate_det: bad argument");
    if (M == 0) return 0;
    if (!x || !idx) return fail(VQ_E_BADARG, "vq_ema_accumulate_det: null input");
    EmaOwnerPlan pl;
    if (!ema_owner_plan(H, M, K, D, pl)) return fail(VQ_E_UNSUPPORTED, "vq_ema_accumulate_det: D > 2048");
    if (!workspace || workspace_bytes < vq_ema_det_workspace_bytes(H, M, K, D) || ((uintptr_t)workspace & 15))
        return fail(VQ_E_BADARG, "vq_ema_accumulate_det: workspace too small or misaligned (see vq_ema_det_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    float *part_sums = (float *)workspace;
    float *part_counts = part_sums + pl.row_blocks * H * (long long)K * D;
    if (int rc = launch_ema_owner(pl, x, x_rs, x_hs, idx, idx_rs, idx_hs, mask, H, M, K, D, counts, sums, part_sums, part_counts, s))
        return rc;
    const long long n_s = (long long)H * K * D, n_c = (long long)H * K;
    if (int rc = launch<vq_ema_reduce_parts_kernel>(dim3((unsigned)((n_s + 255) / 256)), dim3(256), 0, s, "vq_ema_reduce_parts launch", part_sums,
                                                    (int)pl.row_blocks, n_s, sums))
        return rc;
    return launch<vq_ema_reduce_parts_kernel>(dim3((unsigned)((n_c + 255) / 256)), dim3(256), 0, s, "vq_ema_reduce_parts launch", part_counts,
                                              (int)pl.row_blocks, n_c, counts);
}

int vq_ema_accumulate_residual_f32(const vq_args *a, float *counts, float *sums, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    if (!a->cb || !a->idx || !counts || !sums) return fail(VQ_E_BADARG, "vq_ema_accumulate_residual: cb / idx / counts / sums is null");
    long long blocks = (a->M + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    return launch<vq_ema_accumulate_residual_kernel>(dim3((unsigned)blocks, (unsigned)a->H), dim3(256), 0, (hipStream_t)stream,
                                                     "vq_ema_accumulate_residual launch", a->x, (long long)a->x_rs, (long long)a->x_hs, a->cb,
                                                     (long long)a->cb_hs, (long long)a->cb_qs, (const long long *)a->idx, (long long)a->idx_rs,
                                                     (long long)a->idx_hs, (long long)a->idx_qs, (long long)a->M, a->K, a->D, a->Q,
                                                     (a->flags & VQ_F_STE) ? 1 : 0, counts, sums);
}

int vq_ema_update_f32(float *cluster_size, float *embed_avg, float *embeddings, const float *counts, const float *sums,
                      float *total_scratch, int H, int K, int D, double decay, float eps, int l2norm, void *stream) {
    if (!cluster_size || !embed_avg || !embeddings || !counts || !sums || !total_scratch || H <= 0 || K <= 0 || D <= 0)
        return fail(VQ_E_BADARG, "vq_ema_update: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const float weight = (float)(1.0 - decay);  // lerp_(.., 1 - decay): the reference subtracts in double and rounds the weight once
    if (int rc = launch<vq_ema_sizes_kernel>(dim3(H), dim3(256), 0, s, "vq_ema_update launch", cluster_size, counts, K, weight, total_scratch)) return rc;
    const long long rows = (long long)H * K;
    return launch<vq_ema_codes_kernel>(dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, "vq_ema_update launch", cluster_size, total_scratch, embed_avg,
                                       sums, embeddings, H, K, D, weight, eps, l2norm);
}

static int64_t expire_round16(int64_t n) { return (n + 15) / 16 * 16; }

int64_t vq_expire_workspace_bytes(int H, int K) {
    if (H < 0 || K < 0) return 0;
    return expire_round16((int64_t)H * 4) + expire_round16((int64_t)H * K * 4) + 16;  // [n_dead: H][list: H * K], int32
}

int vq_expire_codes_f32(float *cluster_size, float *embed_avg, float *embeddings, const float *pool, int64_t pool_rs, int64_t pool_hs,
                        int64_t N, const vq_args *chain, int stage, int H, int K, int D, float threshold, float reset_cluster_size,
                        int l2norm, const int64_t *seed, int64_t *picked, int32_t *n_expired, void *workspace, void *stream) {
    if (H < 0 || K < 0 || D < 1 || H > 65535) return fail(VQ_E_BADARG, "vq_expire_codes: bad size (H in [0, 65535], K >= 0, D >= 1)");
    ExpireChain ch = {};
    if (chain) {
        if (H > 1 || chain->H != 1 || chain->K != K || chain->D != D || stage < 0 || stage >= chain->Q || chain->M < 0)
            return fail(VQ_E_BADARG, "vq_expire_codes: the chain needs H == 1, the codebook's K and D, and 0 <= stage < Q");
        N = chain->M;
    }
    if (N < 0) return fail(VQ_E_BADARG, "vq_expire_codes: negative N");
    if (N == 0 || H == 0 || K == 0) return 0;
    if (!cluster_size || !embed_avg || !embeddings || !seed || !workspace)
        return fail(VQ_E_BADARG, "vq_expire_codes: cluster_size / embed_avg / embeddings / seed / workspace is null");
    if ((uintptr_t)workspace & 15) return fail(VQ_E_BADARG, "vq_expire_codes: workspace is not 16-byte aligned");
    if (chain) {
        if (!chain->x || (stage > 0 && (!chain->cb || !chain->idx))) return fail(VQ_E_BADARG, "vq_expire_codes: chain x / cb / idx is null");
        ch.x = chain->x, ch.x_rs = chain->x_rs, ch.cb = chain->cb, ch.cb_qs = chain->cb_qs;
        ch.idx = (const long long *)chain->idx, ch.idx_rs = chain->idx_rs, ch.idx_qs = chain->idx_qs, ch.stage = stage;
    } else if (!pool) {
        return fail(VQ_E_BADARG, "vq_expire_codes: pool is null and no chain is given");
    }
    hipStream_t s = (hipStream_t)stream;
    int *n_dead_ws = (int *)workspace;
    int *list_ws = (int *)((char *)workspace + expire_round16((int64_t)H * 4));
    if (int rc = launch<vq_expire_scan_kernel>(dim3((unsigned)H), dim3(256), 0, s, "vq_expire_scan launch", (const float *)cluster_size, K, threshold,
                                               n_dead_ws, list_ws, (long long *)picked, (int *)n_expired))
        return rc;
    int blocks = (K + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    return launch<vq_expire_copy_kernel>(dim3((unsigned)blocks, (unsigned)H), dim3(256), 0, s, "vq_expire_copy launch", cluster_size, embed_avg,
                                         embeddings, pool, (long long)pool_rs, (long long)pool_hs, (long long)N, ch, chain ? 1 : 0, K, D,
                                         reset_cluster_size, l2norm ? 1 : 0, (const long long *)seed, (long long *)picked,
                                         (const int *)n_dead_ws, (const int *)list_ws);
}

int64_t vq_affine_stats_workspace_bytes(int H, int64_t M, int D) {
    if (H <= 0 || M < 0 || D <= 0) return 0;
    // (the geometry depends on the alignment of the call: the larger of the two)
    const AffineGeo a = affine_geo(H, M, D, true), b = affine_geo(H, M, D, false);
    const int nblk = a.nblk > b.nblk ? a.nblk : b.nblk;
    return affine_ws_counts(H, nblk) * 4 + 2ll * H * nblk * D * 8 + 256;
}

int vq_affine_stats_f32(const float *x, int64_t x_rs, int64_t x_hs, const uint8_t *mask, int64_t mask_rs, int64_t mask_hs, int H,
                        int64_t M, int D, int64_t *count, float *mean, float *m2, void *workspace, int64_t workspace_bytes,
                        void *stream) {
    if (H <= 0 || M < 0 || D <= 0 || H > 65535) return fail(VQ_E_BADARG, "vq_affine_stats: bad size");
    if (!count || !mean || !m2) return fail(VQ_E_BADARG, "vq_affine_stats: count / mean / m2 is null");
    if (!x && M > 0) return fail(VQ_E_BADARG, "vq_affine_stats: x is null");
    if (M > 1 && x_rs < D) return fail(VQ_E_BADARG, "vq_affine_stats: row stride smaller than D");
    if (!workspace || workspace_bytes < vq_affine_stats_workspace_bytes(H, M, D) || ((uintptr_t)workspace & 15))
        return fail(VQ_E_BADARG, "vq_affine_stats: workspace too small or misaligned (see vq_affine_stats_workspace_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = D % 4 == 0 && vec4_ok(x, {x_rs, x_hs});
    const AffineGeo g = affine_geo(H, M, D, vec);
    if (M / g.nblk >= (1ll << 24)) return fail(VQ_E_UNSUPPORTED, "vq_affine_stats: more than 2^24 rows per partial");
    unsigned *part_n = (unsigned *)workspace;
    double *part_mean = (double *)((unsigned *)workspace + affine_ws_counts(H, g.nblk));  // (a multiple of 256 bytes in)
    double *part_m2 = part_mean + (long long)H * g.nblk * D;
    const int nblk = M > 0 ? g.nblk : 0;
    if (nblk > 0) {
        const dim3 grid((unsigned)g.nblk, (unsigned)g.cg, (unsigned)H);
        const int rc = vec ? launch<vq_affine_stats_kernel<4>>(grid, dim3(256), 0, s, "vq_affine_stats launch", x, (long long)x_rs, (long long)x_hs, mask,
                                                               (long long)mask_rs, (long long)mask_hs, (long long)M, D, g.tc, g.nblk, part_n, part_mean, part_m2)
                           : launch<vq_affine_stats_kernel<1>>(grid, dim3(256), 0, s, "vq_affine_stats launch", x, (long long)x_rs, (long long)x_hs, mask,
                                                               (long long)mask_rs, (long long)mask_hs, (long long)M, D, g.tc, g.nblk, part_n, part_mean, part_m2);
        if (rc) return rc;
    }
    return launch<vq_affine_merge_kernel>(dim3((unsigned)((D + 3) / 4), (unsigned)H), dim3(256), 0, s, "vq_affine_merge launch", (const unsigned *)part_n,
                                          (const double *)part_mean, (const double *)part_m2, H, D, nblk, (long long *)count, mean, m2);
}

int vq_affine_apply_f32(const float *in, float *out, const float *hits, const float *codebook_mean, const float *codebook_variance,
                        const float *batch_mean, const float *batch_variance, int H, int K, int D, int mode, void *stream) {
    if (H <= 0 || K <= 0 || D <= 0) return fail(VQ_E_BADARG, "vq_affine_apply: non-positive size");
    if (mode != 0 && mode != 1) return fail(VQ_E_BADARG, "vq_affine_apply: mode must be 0 (codes) or 1 (accumulated sums)");
    if (!in || !out || !codebook_mean || !codebook_variance || !batch_mean || !batch_variance)
        return fail(VQ_E_BADARG, "vq_affine_apply: null argument");
    if (mode == 1 && !hits) return fail(VQ_E_BADARG, "vq_affine_apply: mode 1 needs hits");
    const long long total = (long long)H * K * D;
    if ((total + 255) / 256 >= (1ll << 31)) return fail(VQ_E_UNSUPPORTED, "vq_affine_apply: too many elements for one launch");
    return launch<vq_affine_apply_kernel>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, "vq_affine_apply launch", in, out,
                                          hits, codebook_mean, codebook_variance, batch_mean, batch_variance, K, D, total, mode);
}

static int fill_aux_params(AuxParams &p, const vq_args *a) {
    memset(&p, 0, sizeof(p));
    if (!a->packed) return fail(VQ_E_BADARG, "vq: packed codebook is null");
    if (vq_packed_floats(a->K, a->D) * 4 >= (1ll << 31))
        return fail(VQ_E_UNSUPPORTED, "vq: packed codebook image >= 2 GiB (shard the codebook)");
    p.x = a->x; p.x_rs = a->x_rs; p.x_hs = a->x_hs;
    p.packed = a->packed; p.pk_hs = a->pk_hs;
    p.pk_bytes = (unsigned)(vq_packed_floats(a->K, a->D) * 4);
    p.M = a->M; p.K = a->K; p.D = a->D;
    p.ntiles = tiles_of(a->K, padded_dim(a->D));
    p.vec_x = vec4_ok(a->x, {a->D, a->x_rs, a->x_hs}) ? 1 : 0;
    return 0;
}

int vq_similarities_f32(const vq_args *a, float *sims, int64_t sims_rs, int64_t sims_hs, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    if (!sims) return fail(VQ_E_BADARG, "vq_similarities: sims is null");
    hipStream_t s = (hipStream_t)stream;
    const int DP = padded_dim(a->D);
    // rows wider than 512 dims: the sliced MFMA sweep when the caller provides its workspace (vq_workspace_bytes_wide),
    // else the one-thread-per-entry kernel
    if (DP == 0 && !(a->flags & VQ_F_FORCE_SIMPLE) && a->packed) {
        const WidePlan w = wide_plan(a->H, a->M, a->K, a->D);
        if (a->workspace && a->workspace_bytes >= wide_workspace_bytes(a->H, a->M, w))
            return run_wide(a, w, 0, nullptr, sims, sims_rs, sims_hs, plan_device(), read_switches(), s);
    }
    if ((a->flags & VQ_F_FORCE_SIMPLE) || DP == 0) {
        if (!a->cb) return fail(VQ_E_BADARG, "vq_similarities: natural codebook required for the scalar kernel");
        const long long n = a->M * (long long)a->K;
        if ((n + 255) / 256 > 0x7FFFFFFFll) return fail(VQ_E_UNSUPPORTED, "vq_similarities: chunk too large for the scalar kernel");
        return with_metric(a->metric, [&](auto m) {
            return launch<vq_sims_simple<decltype(m)::value>>(dim3((unsigned)((n + 255) / 256), (unsigned)a->H), dim3(256), 0, s, "vq_sims_simple launch", a->x,
                                                              a->x_rs, a->x_hs, a->cb, a->cb_hs, a->M, a->K, a->D, sims, (long long)sims_rs, (long long)sims_hs);
        });
    }
    AuxParams p;
    rc = fill_aux_params(p, a);
    if (rc) return rc;
    p.sims = sims; p.sims_rs = sims_rs; p.sims_hs = sims_hs;
    p.vec_s = vec4_ok(sims, {a->K, sims_rs, sims_hs}) ? 1 : 0;
    return launch_aux(DP, p, a->H, a->metric, kAuxSims, s);
}

int vq_softmax_stats_f32(const vq_args *a, float scale, const int64_t *target, int64_t tgt_rs, int64_t tgt_hs, float *lse,
                         float *target_logit, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    if (!lse) return fail(VQ_E_BADARG, "vq_softmax_stats: lse is null");
    if (target && !target_logit) return fail(VQ_E_BADARG, "vq_softmax_stats: target_logit is null");
    const int DP = padded_dim(a->D);
    if (DP == 0) return fail(VQ_E_UNSUPPORTED, "vq_softmax_stats: D > 512 is not supported (use vq_similarities_f32 chunks)");
    AuxParams p;
    rc = fill_aux_params(p, a);
    if (rc) return rc;
    p.scale = scale;
    p.target = (const long long *)target; p.tgt_rs = tgt_rs; p.tgt_hs = tgt_hs;
    p.lse = lse; p.tgt_logit = target_logit;
    return launch_aux(DP, p, a->H, a->metric, kAuxStats, (hipStream_t)stream);
}

// the arguments both cross-entropy backward entries share; `cb`: the natural codes the finalize takes the target's row from
static int fill_ce_bwd_params(CeBwdParams &p, const vq_args *a, const float *cb, int64_t cb_hs, const float *lse, const float *target_logit,
                              const int64_t *target, int64_t tgt_rs, int64_t tgt_hs, const float *coef, float *grad_x, int64_t gx_rs,
                              int64_t gx_hs) {
    AuxParams ap;
    const int rc = fill_aux_params(ap, a);
    if (rc) return rc;
    memset(&p, 0, sizeof(p));
    p.x = ap.x; p.x_rs = ap.x_rs; p.x_hs = ap.x_hs;
    p.packed = ap.packed; p.pk_hs = ap.pk_hs; p.pk_bytes = ap.pk_bytes;
    p.M = ap.M; p.K = ap.K; p.D = ap.D; p.ntiles = ap.ntiles; p.vec_x = ap.vec_x;
    p.lse = lse;
    p.target = (const long long *)target; p.tgt_rs = tgt_rs; p.tgt_hs = tgt_hs;
    p.coef = coef;
    p.cb = cb; p.cb_hs = cb_hs;
    p.tgt_logit = target_logit;
    p.gx = grad_x; p.gx_rs = gx_rs; p.gx_hs = gx_hs;
    return 0;
}

int vq_ce_backward_f32(const vq_args *a, const float *lse, const float *target_logit, const int64_t *target, int64_t tgt_rs,
                       int64_t tgt_hs, const float *coef, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    if (!lse || !target_logit || !target || !coef || !grad_x || !a->cb)
        return fail(VQ_E_BADARG, "vq_ce_backward: null argument (lse / target_logit / target / coef / grad_x / cb)");
    const int DP = padded_dim(a->D);
    if (DP == 0) return fail(VQ_E_UNSUPPORTED, "vq_ce_backward: D > 512 (use vq_similarities_f32 row chunks)");
    CeBwdParams p;
    rc = fill_ce_bwd_params(p, a, a->cb, a->cb_hs, lse, target_logit, target, tgt_rs, tgt_hs, coef, grad_x, gx_rs, gx_hs);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return with_padded_dim(DP, [&](auto dp) { return vqi::part_ce_bwd<decltype(dp)::value>(p, a->H, a->metric, s); },
                           [] { return fail(VQ_E_UNSUPPORTED, "vq_ce_backward: unsupported padded dim"); });
}

int vq_ce_backward_live_f32(const vq_args *a, const float *live_cb, int64_t live_cb_hs, const float *live_packed, int64_t live_pk_hs,
                            const float *lse, const float *target_logit, const int64_t *target, int64_t tgt_rs, int64_t tgt_hs,
                            const float *coef, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (!live_cb || !live_packed) return fail(VQ_E_BADARG, "vq_ce_backward_live: null argument (live_cb / live_packed)");
    if (!lse || !target_logit || !target || !coef || !grad_x)
        return fail(VQ_E_BADARG, "vq_ce_backward_live: null argument (lse / target_logit / target / coef / grad_x)");
    if (!a->packed) return fail(VQ_E_BADARG, "vq_ce_backward_live: packed codebook is null (the codes the forward searched)");
    if (a->D > 256) return fail(VQ_E_UNSUPPORTED, "vq_ce_backward_live: D > 256 (four tile buffers of wider rows do not fit in LDS; use vq_similarities_f32 row chunks)");
    if (a->M == 0) return 0;
    const int DP = padded_dim(a->D);
    CeBwdLiveParams p;
    // (the finalize adds the target's term from p.cb: the live codes; a->cb is not read)
    rc = fill_ce_bwd_params(p, a, live_cb, live_cb_hs, lse, target_logit, target, tgt_rs, tgt_hs, coef, grad_x, gx_rs, gx_hs);
    if (rc) return rc;
    p.live_packed = live_packed; p.live_pk_hs = live_pk_hs;
    hipStream_t s = (hipStream_t)stream;
    return with_padded_dim(DP,
                           [&](auto dp) {
                               constexpr int DPC = decltype(dp)::value;
                               if constexpr (DPC > 256) return fail(VQ_E_UNSUPPORTED, "vq_ce_backward_live: unsupported padded dim");
                               else return vqi::part_ce_bwd_live<DPC>(p, a->H, a->metric, s);
                           },
                           [] { return fail(VQ_E_UNSUPPORTED, "vq_ce_backward_live: unsupported padded dim"); });
}

// ---- Gumbel-max code sampling (vq_sample.inc, kAuxSample in vq_similarity.inc) -----------------------------------------
int vq_gumbel_sample_f32(const vq_args *a, float tau, const int64_t *seed, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (!(__builtin_fabsf(tau) < __builtin_inff())) return fail(VQ_E_BADARG, "vq_gumbel_sample: tau is not finite");
    if (!seed) return fail(VQ_E_BADARG, "vq_gumbel_sample: seed is null");
    if (a->M == 0) return 0;
    if (!a->idx) return fail(VQ_E_BADARG, "vq_gumbel_sample: idx is null");
    const int DP = padded_dim(a->D);
    if (DP == 0) return fail(VQ_E_UNSUPPORTED, "vq_gumbel_sample: D > 512 is not supported (use vq_similarities_f32 chunks)");
    AuxParams p;
    rc = fill_aux_params(p, a);
    if (rc) return rc;
    p.tau = tau;
    p.seed = (const long long *)seed;
    p.idx = (long long *)a->idx; p.idx_rs = a->idx_rs; p.idx_hs = a->idx_hs;
    hipStream_t s = (hipStream_t)stream;
    return with_padded_dim(DP, [&](auto dp) { return vqi::part_sample<decltype(dp)::value>(p, a->H, a->metric, s); },
                           [] { return fail(VQ_E_UNSUPPORTED, "vq_gumbel_sample: unsupported padded dim"); });
}

int vq_gumbel_noise_f32(const int64_t *seed, int H, int64_t M, int K, float *noise, uint32_t *bits, void *stream) {
    if (!seed || !noise) return fail(VQ_E_BADARG, "vq_gumbel_noise: null argument (seed / noise)");
    if (H <= 0 || M < 0 || K <= 0) return fail(VQ_E_BADARG, "vq_gumbel_noise: non-positive size");
    if (M == 0) return 0;
    const long long n = (long long)H * M * K;
    long long blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;  // (the kernel strides over the rest)
    return launch<vq_gumbel_noise_kernel>(dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, "vq_gumbel_noise launch",
                                          (const long long *)seed, H, (long long)M, K, noise, (unsigned *)bits);
}

// ---- the resident/streamed sweep family (Gumbel, reinmax, diversity, cross-entropy codes, orthogonal): its plans, helpers and entries
#include "vq_sweep_host.inc"

int vq_max_fused_stages(int D, int want_sq_err) {
    // largest Q one residual launch can hold (winner indices and loss partials of every stage live in LDS); 0: no fused residual launch (D > 512)
    return with_padded_dim(padded_dim(D), [&](auto dp) { return max_stages_t<decltype(dp)::value, decltype(dp)::value == 512 ? 4 : 8>(want_sq_err != 0); },
                           [] { return 0; });
}

int vq_nearest_f32(const vq_args *a, void *stream) {
    if (a && a->Q != 1) return fail(VQ_E_BADARG, "vq_nearest_f32: Q must be 1");
    return vq_quantize_f32(a, stream);
}

int vq_residual_f32(const vq_args *a, void *stream) { return vq_quantize_f32(a, stream); }

int64_t vq_lfq_workspace_bytes(int64_t N, int64_t R, int C, int d) {
    if (lfq_check_shape(N, C, d) || R < 0 || R > N) return 0;
    return lfq_ws_layout(N, R, C, d).total;
}

int vq_lfq_quantize_f32(const float *v, int64_t v_rs, const float *xa, int64_t xa_rs, int64_t N, int C, int d, float qmag,
                        const uint8_t *mask, float *q, float *out, int64_t *idx, double *commit_sum, void *workspace,
                        int64_t workspace_bytes, void *stream) {
    int rc = lfq_check_shape(N, C, d);
    if (rc) return rc;
    if (!v || !q || !idx || (out && !xa)) return fail(VQ_E_BADARG, "vq_lfq_quantize: null pointer");
    if (v_rs < (int64_t)C * d || (out && xa_rs < (int64_t)C * d)) return fail(VQ_E_BADARG, "vq_lfq_quantize: row stride < C * d");
    const LfqWs ws = lfq_ws_layout(N, 0, C, d);
    if (commit_sum && (!workspace || workspace_bytes < ws.ent)) return fail(VQ_E_BADARG, "vq_lfq_quantize: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = lfq_quant_blocks(N, C);
    double *part = commit_sum ? (double *)((char *)workspace + ws.commit) : nullptr;
    if (blocks > 0)
        rc = launch<lfq_quantize_kernel>(dim3((unsigned)blocks), dim3(kLfqQuantThreads), 0, s, "vq_lfq_quantize launch", v, v_rs, xa, xa_rs, N, C, d, qmag,
                                         mask, q, out, idx, part);
    if (rc || !commit_sum) return rc;
    return launch<lfq_sum_kernel<double>>(dim3(1), dim3(kLfqSumThreads), 0, s, "vq_lfq_quantize launch", part, blocks, commit_sum, (int64_t)0);
}

int vq_lfq_entropy_fwd_f32(const float *v, int64_t v_rs, const int64_t *rows, int64_t R, int C, int d, float code_scale,
                           float inv_temperature, float *avg_prob, double *per_sample_sum, void *workspace,
                           int64_t workspace_bytes, void *stream) {
    return lfq_entropy_fwd_run(v, v_rs, 0, rows, 0, R, 1, C, d, &code_scale, nullptr, 1, inv_temperature, avg_prob, per_sample_sum,
                               workspace, workspace_bytes, stream, "vq_lfq_entropy_fwd");
}

int vq_lfq_entropy_bwd_f32(const float *v, int64_t v_rs, const int64_t *rows, int64_t R, int C, int d, float code_scale,
                           float inv_temperature, const float *w_ps, const float *w_cb, float *grad_v, int64_t gv_rs,
                           void *stream) {
    return lfq_entropy_bwd_run(v, v_rs, 0, rows, 0, R, 1, C, d, &code_scale, nullptr, 1, inv_temperature, w_ps, w_cb, grad_v, gv_rs, 0,
                               stream, "vq_lfq_entropy_bwd");
}

int64_t vq_lfq_staged_workspace_bytes(int64_t R, int T, int d) {
    if (T < 1 || lfq_check_shape(R, 1, d)) return 0;
    return lfq_ws_layout(R, R, 1, d, T).total;
}

int vq_lfq_entropy_staged_fwd_f32(const float *v, int64_t v_rs, int64_t v_ss, const int64_t *rows, int64_t rows_ss, int64_t R,
                                  int T, int d, const float *code_scale, int period, float inv_temperature, float *avg_prob,
                                  double *per_sample_sum, void *workspace, int64_t workspace_bytes, void *stream) {
    return lfq_entropy_fwd_run(v, v_rs, v_ss, rows, rows_ss, R, T, 1, d, nullptr, code_scale, period, inv_temperature, avg_prob,
                               per_sample_sum, workspace, workspace_bytes, stream, "vq_lfq_entropy_staged_fwd");
}

int vq_lfq_entropy_staged_bwd_f32(const float *v, int64_t v_rs, int64_t v_ss, const int64_t *rows, int64_t rows_ss, int64_t R,
                                  int T, int d, const float *code_scale, int period, float inv_temperature, const float *w_ps,
                                  const float *w_cb, float *grad_v, int64_t gv_rs, int64_t gv_ss, void *stream) {
    return lfq_entropy_bwd_run(v, v_rs, v_ss, rows, rows_ss, R, T, 1, d, nullptr, code_scale, period, inv_temperature, w_ps, w_cb, grad_v,
                               gv_rs, gv_ss, stream, "vq_lfq_entropy_staged_bwd");
}

int64_t vq_rlfq_workspace_bytes(int64_t G, int64_t N, int S) {
    if (G < 1 || N < 0 || S < 1 || S > VQ_RLFQ_MAX_STAGES) return 0;
    return rlfq_ws_bytes(G, N, S);
}

int vq_rlfq_quantize_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, int S, const float *stage_consts,
                         int spherical, int ste, const uint8_t *mask, float *out, int64_t out_gs, int64_t out_rs, int64_t *idx,
                         float *v_all, double *commit_sum, void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = rlfq_check(G, N, d, S, stage_consts, "vq_rlfq_quantize");
    if (rc) return rc;
    if (!x || !out || !idx) return fail(VQ_E_BADARG, "vq_rlfq_quantize: null pointer");
    if (commit_sum && (!workspace || workspace_bytes < rlfq_ws_bytes(G, N, S)))
        return fail(VQ_E_BADARG, "vq_rlfq_quantize: workspace too small");
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = rlfq_blocks(N);
    double *part = commit_sum ? (double *)workspace : nullptr;
    rc = rlfq_launch_quantize(d, dim3((unsigned)blocks, (unsigned)G), s, "vq_rlfq_quantize launch", x, x_gs, x_rs, N, S, stage_consts, spherical != 0,
                              ste != 0, mask, out, out_gs, out_rs, idx, v_all, part);
    if (rc || !commit_sum) return rc;
    return launch<lfq_sum_kernel<double>>(dim3((unsigned)(G * S)), dim3(kLfqSumThreads), 0, s, "vq_rlfq_quantize launch", part, blocks, commit_sum, blocks);
}

int vq_rlfq_backward_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, int S, const float *stage_consts,
                         int spherical, const uint8_t *mask, const float *g_out, int64_t g_gs, int64_t g_rs,
                         const float *w_commit, const float *g_ent, float *grad_x, int64_t gx_gs, int64_t gx_rs, void *stream) {
    int rc = rlfq_check(G, N, d, S, stage_consts, "vq_rlfq_backward");
    if (rc) return rc;
    if (!x || !grad_x) return fail(VQ_E_BADARG, "vq_rlfq_backward: null pointer");
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    return rlfq_launch_backward(d, dim3((unsigned)rlfq_blocks(N), (unsigned)G), s, "vq_rlfq_backward launch", x, x_gs, x_rs, N, S, stage_consts,
                                spherical != 0, mask, g_out, g_gs, g_rs, w_commit, g_ent, grad_x, gx_gs, gx_rs);
}

int vq_fsq_quantize_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, const int32_t *levels, int S,
                        const float *consts, int prebound, float *out, int64_t out_gs, int64_t out_rs, int32_t *idx,
                        void *stream) {
    FsqLevels lv;
    int rc = fsq_check(G, N, d, S, levels, consts, lv, "vq_fsq_quantize");
    if (rc) return rc;
    if (!x || !out) return fail(VQ_E_BADARG, "vq_fsq_quantize: null pointer");
    hipStream_t s = (hipStream_t)stream;
    return fsq_launch_quantize(d, dim3((unsigned)fsq_blocks(N), (unsigned)G), s, "vq_fsq_quantize launch", x, x_gs, x_rs, N, S, lv, consts, prebound != 0,
                               out, out_gs, out_rs, idx);
}

int vq_fsq_backward_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, const int32_t *levels, int S,
                        const float *consts, int prebound, const float *g_out, int64_t g_gs, int64_t g_rs, float *grad_x,
                        int64_t gx_gs, int64_t gx_rs, void *stream) {
    FsqLevels lv;
    int rc = fsq_check(G, N, d, S, levels, consts, lv, "vq_fsq_backward");
    if (rc) return rc;
    if (!x || !g_out || !grad_x) return fail(VQ_E_BADARG, "vq_fsq_backward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    return fsq_launch_backward(d, dim3((unsigned)fsq_blocks(N), (unsigned)G), s, "vq_fsq_backward launch", x, x_gs, x_rs, N, S, lv, consts, prebound != 0,
                               g_out, g_gs, g_rs, grad_x, gx_gs, gx_rs);
}

int vq_fsq_decode_f32(const void *idx, int idx_64, int64_t N, int Q, int d, const int32_t *levels, const float *scales,
                      int drop_null, float *codes_sum, float *all_codes, void *stream) {
    FsqLevels lv;
    int rc = fsq_check(1, N, d, Q, levels, scales, lv, "vq_fsq_decode");
    if (rc) return rc;
    if (!idx || (!codes_sum && !all_codes)) return fail(VQ_E_BADARG, "vq_fsq_decode: null pointer");
    hipStream_t s = (hipStream_t)stream;
    return fsq_launch_decode(d, dim3((unsigned)fsq_blocks(N)), s, "vq_fsq_decode launch", idx, idx_64 != 0, N, Q, lv, scales, drop_null != 0, codes_sum,
                             all_codes);
}

int vq_decode_f32(const float *cb, int64_t cb_gs, int64_t cb_qs, int G, int Q, int K, int D, const void *idx, int idx_64,
                  int64_t idx_gs, int64_t idx_rs, int64_t idx_qs, int64_t N, int Q_given, int drop_null, float *codes_sum,
                  int64_t sum_gs, int64_t sum_rs, int64_t sum_ds, float *all_codes, int64_t all_qs, int64_t all_gs,
                  int64_t all_rs, void *stream) {
    if (!cb || !idx) return fail(VQ_E_BADARG, "vq_decode: cb or idx is null");
    if (!codes_sum && !all_codes) return fail(VQ_E_BADARG, "vq_decode: both outputs are null");
    if (G <= 0 || Q <= 0 || K <= 0 || D <= 0 || N < 0) return fail(VQ_E_BADARG, "vq_decode: non-positive size");
    if (Q_given < 1 || Q_given > Q) return fail(VQ_E_BADARG, "vq_decode: Q_given must be in [1, Q]");
    if (N > INT64_MAX / D || N * D > INT64_MAX / G) return fail(VQ_E_BADARG, "vq_decode: too many elements");
    if (N == 0) return 0;
    DecodeParams p;
    memset(&p, 0, sizeof(p));
    p.cb = cb; p.cb_gs = cb_gs; p.cb_qs = cb_qs;
    p.G = G; p.Q = Q; p.K = K; p.D = D;
    p.idx = idx; p.idx64 = idx_64 != 0; p.idx_gs = idx_gs; p.idx_rs = idx_rs; p.idx_qs = idx_qs;
    p.N = N; p.Qg = Q_given; p.drop_null = drop_null != 0;
    p.sum = codes_sum; p.sum_gs = sum_gs; p.sum_rs = sum_rs; p.sum_ds = sum_ds;
    p.all = all_codes; p.all_qs = all_qs; p.all_gs = all_gs; p.all_rs = all_rs;
    return decode_launch(p, device_cus(), (hipStream_t)stream);
}

static int rm_check(const char *who, const float *x, const float *cb, const void *idx, const uint8_t *mask, int G, int64_t M, int Q,
                    int K, int D) {
    if (G <= 0 || G > 65535 || Q <= 0 || K <= 0 || M < 0) return fail(VQ_E_BADARG, who, "G must be in [1, 65535], Q and K positive, M non-negative");
    if (D < 1 || D > 512) return fail(VQ_E_BADARG, who, "D must be in [1, 512]");
    if (M > INT64_MAX / D || M * D > INT64_MAX / G || M > INT64_MAX / Q / G) return fail(VQ_E_BADARG, who, "too many elements");
    if (M == 0) return 0;
    if (!x || !cb || !idx || !mask) return fail(VQ_E_BADARG, who, "x, cb, idx or mask is null");
    return 0;
}

int vq_residual_mask_f32(const float *x, int64_t x_gs, int64_t x_rs, const float *cb, int64_t cb_gs, int64_t cb_qs, int64_t *idx,
                         int64_t idx_gs, int64_t idx_rs, int64_t idx_qs, const uint8_t *mask, int64_t mask_gs,
                         const int64_t *zero_idx, int G, int64_t M, int Q, int K, int D, int train, float *out, int64_t out_gs,
                         int64_t out_rs, double *sq_err, int sq_err_per_group, void *workspace, int64_t workspace_bytes,
                         void *stream) {
    const char *who = "vq_residual_mask";
    int rc = rm_check(who, x, cb, idx, mask, G, M, Q, K, D);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {  // no launch: the sums of no rows
        if (sq_err) return clear_sq_err(sq_err, (size_t)Q * (sq_err_per_group ? G : 1), s, "vq_residual_mask memset");
        return 0;
    }
    if (!out || !zero_idx) return fail(VQ_E_BADARG, who, "out or zero_idx is null");
    ResMaskParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.x_gs = x_gs; p.x_rs = x_rs;
    p.cb = cb; p.cb_gs = cb_gs; p.cb_qs = cb_qs;
    p.idx = (long long *)idx; p.idx_gs = idx_gs; p.idx_rs = idx_rs; p.idx_qs = idx_qs;
    p.mask = mask; p.mask_gs = mask_gs;
    p.zero_idx = (const long long *)zero_idx;
    p.M = M; p.Q = Q; p.K = K; p.D = D; p.train = train != 0;
    p.out = out; p.out_gs = out_gs; p.out_rs = out_rs;
    rm_plan(p);
    if (sq_err) {
        if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < (int64_t)sizeof(float) * G * p.units * Q)
            return fail(VQ_E_BADARG, who, "workspace is null, misaligned or smaller than 4 * G * Q * ceil(M / 2) bytes");
        p.part = (float *)workspace;
    }
    const bool vec = D % 4 == 0 && rm_aligned(x, {x_gs, x_rs}) && rm_aligned(cb, {cb_gs, cb_qs}) && rm_aligned(out, {out_gs, out_rs});
    rc = rm_dispatch<RmForward>(p, vec, G, device_cus(), s, "vq_residual_mask launch");
    if (rc || !sq_err) return rc;
    // part is [G][units][Q]: one sum per group, or the groups' partials as one list
    if (sq_err_per_group)
        return launch<vq_loss_reduce_kernel>(dim3((unsigned)Q, (unsigned)G), dim3(256), 0, s, "vq_residual_mask reduce launch", (const float *)p.part,
                                             p.units, Q, sq_err, 0, -1);
    return launch<vq_loss_reduce_kernel>(dim3((unsigned)Q), dim3(256), 0, s, "vq_residual_mask reduce launch", (const float *)p.part,
                                         p.units * G, Q, sq_err, 0, -1);
}

int vq_residual_mask_backward_f32(const float *x, int64_t x_gs, int64_t x_rs, const float *cb, int64_t cb_gs, int64_t cb_qs,
                                  const int64_t *idx, int64_t idx_gs, int64_t idx_rs, int64_t idx_qs, const uint8_t *mask,
                                  int64_t mask_gs, int G, int64_t M, int Q, int K, int D, int train, const float *grad_out,
                                  int64_t go_gs, int64_t go_rs, const double *grad_sq_err, int sq_err_per_group, float *grad_x,
                                  int64_t gx_gs, int64_t gx_rs, void *stream) {
    const char *who = "vq_residual_mask_backward";
    int rc = rm_check(who, x, cb, idx, mask, G, M, Q, K, D);
    if (rc || M == 0) return rc;
    if (!grad_x) return fail(VQ_E_BADARG, who, "grad_x is null");
    ResMaskParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.x_gs = x_gs; p.x_rs = x_rs;
    p.cb = cb; p.cb_gs = cb_gs; p.cb_qs = cb_qs;
    p.idx = (long long *)idx; p.idx_gs = idx_gs; p.idx_rs = idx_rs; p.idx_qs = idx_qs;
    p.mask = mask; p.mask_gs = mask_gs;
    p.M = M; p.Q = Q; p.K = K; p.D = D; p.train = train != 0;
    p.out = grad_x; p.out_gs = gx_gs; p.out_rs = gx_rs;
    p.go = grad_out; p.go_gs = go_gs; p.go_rs = go_rs;
    p.g_err = grad_sq_err; p.g_err_gs = sq_err_per_group ? Q : 0;
    rm_plan(p);
    const bool vec = D % 4 == 0 && rm_aligned(x, {x_gs, x_rs}) && rm_aligned(cb, {cb_gs, cb_qs}) && rm_aligned(grad_x, {gx_gs, gx_rs}) &&
                     (!grad_out || rm_aligned(grad_out, {go_gs, go_rs}));
    return rm_dispatch<RmBackward>(p, vec, G, device_cus(), (hipStream_t)stream, "vq_residual_mask_backward launch");
}

int vq_lfq_decode_f32(const void *idx, int idx_64, int64_t idx_gs, int64_t idx_rs, int64_t idx_qs, int G, int64_t N, int Q_given,
                      int Q, int d, const float *mag, int drop_null, float *codes_sum, int64_t sum_gs, int64_t sum_rs,
                      int64_t sum_ds, float *all_codes, int64_t all_qs, int64_t all_gs, int64_t all_rs, void *stream) {
    const char *who = "vq_lfq_decode";
    if (!idx || !mag) return fail(VQ_E_BADARG, who, "idx or mag is null");
    if (!codes_sum && !all_codes) return fail(VQ_E_BADARG, who, "both outputs are null");
    if (d < 1 || d > kLfqMaxDim) return fail(VQ_E_BADARG, who, "d must be in [1, 20]");
    if (Q < 1 || Q > VQ_RLFQ_MAX_STAGES) return fail(VQ_E_BADARG, who, "Q must be in [1, 32]");
    if (Q_given < 1 || Q_given > Q) return fail(VQ_E_BADARG, who, "Q_given must be in [1, Q]");
    if (G < 1 || G > 65535 || N < 0) return fail(VQ_E_BADARG, who, "G must be in [1, 65535] and N non-negative");
    if (N > (int64_t)0x7fffffff * kLfqDecodeThreads / d - kLfqDecodeThreads) return fail(VQ_E_BADARG, who, "too many rows");
    if (N == 0) return 0;
    LfqDecodeParams p;
    memset(&p, 0, sizeof(p));
    p.idx = idx; p.idx64 = idx_64 != 0; p.idx_gs = idx_gs; p.idx_rs = idx_rs; p.idx_qs = idx_qs;
    p.N = N; p.Q = Q; p.Qg = Q_given; p.d = d; p.drop_null = drop_null != 0;
    p.sum = codes_sum; p.sum_gs = sum_gs; p.sum_rs = sum_rs; p.sum_ds = sum_ds;
    p.all = all_codes; p.all_qs = all_qs; p.all_gs = all_gs; p.all_rs = all_rs;
    for (int q = 0; q < Q; ++q) p.mag[q] = mag[q];
    return lfq_decode_launch(p, G, (hipStream_t)stream);
}

int64_t vq_lq_workspace_bytes(int64_t B, int64_t P, int C) {
    if (B < 1 || P < 1 || C < 1 || B > INT64_MAX / P || B * P > INT64_MAX / C) return 0;
    return lq_blocks(B * P * C) * (int64_t)sizeof(float);
}

int vq_lq_quantize_f32(const float *z, int64_t z_bs, int64_t z_ps, int64_t z_cs, int64_t B, int64_t P, int C, int d,
                       const int32_t *levels, const float *tables, float *codes, int64_t c_bs, int64_t c_ps, int64_t c_cs,
                       int32_t *idx, float *loss, float w_c, float w_q, void *workspace, int64_t workspace_bytes,
                       void *stream) {
    FsqLevels lv;
    int rc = fsq_check(1, 1, d, 1, levels, tables, lv, "vq_lq_quantize");
    if (rc) return rc;
    int n_table = 0;
    rc = lq_check(B, P, C, d, levels, n_table, "vq_lq_quantize");
    if (rc) return rc;
    if (!z || !codes) return fail(VQ_E_BADARG, "vq_lq_quantize: null pointer");
    const int64_t N = B * P * C;
    const int64_t blocks = lq_blocks(N);
    if (loss && (!workspace || workspace_bytes < blocks * (int64_t)sizeof(float)))
        return fail(VQ_E_BADARG, "vq_lq_quantize: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *part = loss ? (float *)workspace : nullptr;
    rc = lq_launch_quantize(d, dim3((unsigned)blocks), s, "vq_lq_quantize launch", z, LqStrides{z_bs, z_ps, z_cs}, P, C, N, lv, tables, n_table, codes,
                            LqStrides{c_bs, c_ps, c_cs}, idx, part);
    if (rc || !loss) return rc;
    return launch<lq_loss_kernel>(dim3(1), dim3(kLqLossThreads), 0, s, "vq_lq_quantize launch", part, blocks, (double)N * (double)d, w_c, w_q, loss);
}

int vq_lq_backward_f32(const float *x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float *out, int64_t o_bs, int64_t o_ps,
                       int64_t o_cs, const float *g_out, int64_t g_bs, int64_t g_ps, int64_t g_cs, const float *g_loss,
                       float coef, int64_t B, int64_t P, int W, float *grad_x, int64_t gx_bs, int64_t gx_ps, int64_t gx_cs,
                       void *stream) {
    if (B < 1 || P < 1 || W < 1) return fail(VQ_E_BADARG, "vq_lq_backward: sizes must be positive");
    if (!x || !out || !g_out || !g_loss || !grad_x) return fail(VQ_E_BADARG, "vq_lq_backward: null pointer");
    if (B > INT64_MAX / P || B * P > INT64_MAX / W || lq_blocks(B * P * W) > 0x7fffffff)
        return fail(VQ_E_BADARG, "vq_lq_backward: too many elements");
    const int64_t N = B * P * W;
    hipStream_t s = (hipStream_t)stream;
    return launch<lq_backward_kernel>(dim3((unsigned)lq_blocks(N)), dim3(kLqThreads), 0, s, "vq_lq_backward launch", x, LqStrides{x_bs, x_ps, x_cs}, out,
                                      LqStrides{o_bs, o_ps, o_cs}, g_out, LqStrides{g_bs, g_ps, g_cs}, g_loss, coef, P, W, N, grad_x,
                                      LqStrides{gx_bs, gx_ps, gx_cs});
}

}  // extern "C"
#endif  // VQ_OWN(0)
