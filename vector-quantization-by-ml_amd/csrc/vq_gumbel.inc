// vq_gumbel.inc -- one resident/streamed sweep, fourteen roles (the role table `sweep_role` below; host side: vq_sweep_host.inc).
// First the backward of the straight-through and of the reinmax Gumbel softmax over the similarities
// (utils/general.py:131-149, codebooks.py:386-395), nothing of [M, K] in memory.  Included by vq_kernels.hip (after vq_similarity.inc: shares its row
// prologue, the tile geometry and the fragment pipeline of the search).
// ------------------------------------------------------------------------------------------------
//   s = similarities [M, K]   g = dL/dquantize [M, D]   a = g c^T [M, K]   tau = 1 / temperature
//   p = softmax_k(tau s)      delta_m = sum_k p_mk a_mk      w = tau p (a - delta) = dL/ds
//   dot     gx = w c                    gc = w^T x
//   Euclid  r = w / s (0 at s == 0)     gx = x rowsum(r) - r c      gc = c colsum(r) - r^T x
// One kernel, three roles to begin with.  "Resident" rows become MFMA B fragments of a wave (32 rows per wave), "streamed" rows pass
// through LDS as packed images (vq_pack.inc layout) and are the A operands:
//   kGumStats  resident x and g rows, streamed codes: two products per tile (s and a), online softmax in the log2 domain
//              -> lse2[m] = log2 sum_k exp2(tau s log2 e) and delta[m]
//   kGumX      the same two products, w (or r) in place in the accumulator of s, then the contraction with the SAME
//              codebook tile (vq_ce_backward's G sweep: the accumulator registers are valid B operands as they stand)
//   kGumC      the roles swapped: a wave owns 32 codes (one fragment set serves both products), tiles of the packed x rows
//              and of the packed g rows are streamed, lse2 / delta are read per streamed row (= per accumulator register),
//              the contraction runs onto the streamed x tile.  The rows are split over blockIdx.z; every split STORES its
//              partial [K, D] (rank-one term included: it is linear in the split) and vq_gumbel_reduce_parts adds the
//              splits in a fixed order: no atomics, bit-identical from run to run.
// Registers at Dp = 256: kGumX holds x fragments + g fragments + gradient accumulators (3 x 128) and compiles to 472 of the
// 512 entries without scratch, so the dims are NOT split over workgroups (a split would repeat the two products per part);
// kGumC holds 128 + 128.  One wave per SIMD from Dp = 128 on.
//
// Reinmax (utils/general.py:131-146) through the same sweep, four more roles.  With p0 = softmax_k(s),
// p1 = max((onehot(ind) + softmax_k(tau s)) / 2, 1e-5), col_k = sum_m p1_mk, e_k = (sum_m p1_mk a_mk) / col_k and
// delta0_m = sum_k p0_mk a_mk:   w = 2 (p1 / col)(a - e) - 0.5 p0 (a - delta0)
//   kRmStats   as kGumStats with two online softmaxes over one running maximum (log2 e s; tau > 0 keeps the order of the
//              logits) -> lse (at tau), lse1 (at 1) and delta = delta0
//   kRmCol     the orientation of kGumC, the two products only: p1 from lse and the int32 copy of ind of the streamed row,
//              per-lane sums of p1 and p1 a over the rows of the split -> partial col / e per blockIdx.z, added in split
//              order by vq_gumbel_reduce_cols
//   kRmX       as kGumX: the statistics and ind of the lane's row, col / e of the streamed codes read four at a time
//   kRmC       as kGumC: the statistics and ind of the streamed rows read four at a time, col / e of the lane's code
// ind is only ever compared with a code index.  Streamed padding is masked AFTER the clamp (p1 = 1e-5 there, not 0).
//
// Codebook diversity loss (vector_quantize_pytorch.py:324-334) through the same sweep, five more roles with ONE product per
// sub-tile (there is no g: what a = g c^T is above is a lookup in the table U [N, K] here).  tau = -T, so p = softmax_k(-T s):
//   kDivStats  as kGumStats without the second product -> lse2
//   kDivAcc    the orientation of kRmCol: the streamed image holds the x rows in position-major order, every position padded
//              to whole 32-row sub-tiles (vq_gumbel_pack_rows with a RowMap), the log-sum-exps in the same order; the per-lane
//              sums of p are flushed at the last sub-tile of a position -> one partial [N, K] per head.  blockIdx.z splits
//              the POSITIONS, so no position is summed across workgroups; padding rows are masked (select, no clamp)
//   kDivDelta  as kGumStats: delta_m = sum_k p_mk U[n(m)][k] / sum_k p_mk, U read four codes at a time in the row of the lane's
//              position
//   kDivX      as kGumX with a = U[n(m)][k]; when a second image is given (the live codes) the contraction reads ITS tile,
//              staged beside the first the way the codes-resident roles stage the g rows
//   kDivC      the orientation of kGumC with the image of kDivAcc (lse2 AND delta copied along in image order): a wave owns 32
//              codes, a = U[n][own code] is one scalar per position, w (or r) of the 16 streamed rows in place in the
//              accumulator of s, the contraction onto the same staged x tile, the column sum of r for the rank-one term.  The
//              staged tiles are split over blockIdx.z as for kGumC (gc sums over ALL rows: a position may straddle workgroups),
//              one partial [K, D] per split.  A position's padding rows hold |x|^2 = +inf under Euclid: with tau < 0 their
//              logit is +inf, p = inf and r = inf * rsqrt(inf) = NaN, which the contraction would multiply with the zero x
//              row -- w / r of a padding row is therefore SELECTED to 0 before the contraction and the column sum
// n(m) = (m / pos_div) % N.
//
// Orthogonal regularisation loss (utils/losses.py:23-28) through the same sweep, one more role (dot metric only): the codes on
// BOTH sides, cos = x x^T of the rows x [n, D] as given (the caller normalises), nothing of [n, n] in memory:
//   kOrth      as kDivX with w = s and no table: resident rows x, streamed the dot image of the same rows.  Each 32x32 block of
//              cos is squared into the lane's running sum -> rowsq_i = sum_j cos_ij^2 (p.lse), then contracted with the
//              same staged tile -> G_i = sum_j cos_ij x_j (p.out; null: the contraction and the finalize are skipped).
//              cos of a streamed row past n and of a resident row past n is SELECTED to 0 by index before either use; a
//              NaN / inf of a real row goes through untouched.  One lane set per row, tile order, no atomics.
//
// Cross-entropy loss over the similarities (vector_quantize_pytorch.py:287-297), the gradient with respect to a learnable
// codebook, one more role with one product per sub-tile.  lse = the natural-log log-sum-exp vq_softmax_stats_f32 wrote (scale 1),
// t the target of the row, coef one float on the device:   w_mk = coef (exp(s_mk - lse_m) - [k == t_m])
//   kCeC       the orientation of kGumC over the natural-order x image: lse and the int32 copy of the target of the 16 streamed
//              rows read four at a time (as kRmC reads its statistics and ind32); the one-hot term is the comparison of the
//              row's target with the lane's code, no side pass.  The int32 copy holds -1 for an ignored row (target < 0 or
//              >= K, compared as the 64-bit value) and past M, and the image holds such a row as padding (zeros, |x|^2 = +inf):
//              its w / r is SELECTED to 0 before the contraction and the column sum, whatever NaN / inf its x or lse holds.
//              The norms enter the product in vq_sweep_aux's order, so s is the value lse was summed from bit for bit (one
//              code: exp(s - lse) = 1 and the gradient is exactly 0).  Row splits and partials as kGumC.
// ------------------------------------------------------------------------------------------------
constexpr int kGumStats = 0;
constexpr int kGumX = 1;
constexpr int kGumC = 2;
constexpr int kRmStats = 3;
constexpr int kRmCol = 4;
constexpr int kRmX = 5;
constexpr int kRmC = 6;
constexpr int kDivStats = 7;
constexpr int kDivAcc = 8;
constexpr int kDivDelta = 9;
constexpr int kDivX = 10;
constexpr int kDivC = 11;
constexpr int kOrth = 12;
constexpr int kCeC = 13;

// The role table: ONE row per role, read by the kernel (its compile-time switches), by launch_gumbel_t (the dynamic LDS those
// switches use) and by the host's launch_gumbel (the build part that owns the role's kernels).  A new role is a new row.
enum SweepPart { kPartGumbel = 7, kPartReinmax = 8, kPartDiversity = 9, kPartOrthogonal = 10, kPartCeCodes = 11 };  // = VQ_PART
struct SweepRole {
    int part;
    bool codes_resident;  // a wave owns 32 codes and the packed rows are streamed (else: rows resident, packed codes streamed)
    bool one_product;     // one product per sub-tile: no g rows, nothing of a = g c^T
    bool reinmax;
    bool no_contraction;  // statistics only: no gradient accumulators, no finalize
    bool second_image;    // a second streamed image at compile time: the packed g rows
    bool xnorm_first;     // |x|^2 of the streamed row enters the product before |c|^2
    bool z_splits_tiles;  // blockIdx.z owns tiles_per_split staged tiles
};
constexpr SweepRole sweep_role(int role) {
    switch (role) {
        //                      part             codes  one    reinmx no_con img2   xnorm  z_tiles
        case kGumStats: return {kPartGumbel,     false, false, false, true,  false, false, false};
        case kGumX:     return {kPartGumbel,     false, false, false, false, false, false, false};
        case kGumC:     return {kPartGumbel,     true,  false, false, false, true,  false, true};
        case kRmStats:  return {kPartReinmax,    false, false, true,  true,  false, false, false};
        case kRmCol:    return {kPartReinmax,    true,  false, true,  true,  true,  false, true};
        case kRmX:      return {kPartReinmax,    false, false, true,  false, false, false, false};
        case kRmC:      return {kPartReinmax,    true,  false, true,  false, true,  false, true};
        case kDivStats: return {kPartDiversity,  false, true,  false, true,  false, false, false};
        case kDivAcc:   return {kPartDiversity,  true,  true,  false, true,  false, true,  false};
        case kDivDelta: return {kPartDiversity,  false, true,  false, true,  false, false, false};
        case kDivX:     return {kPartDiversity,  false, true,  false, false, false, false, false};
        case kDivC:     return {kPartDiversity,  true,  true,  false, false, false, true,  true};
        case kOrth:     return {kPartOrthogonal, false, true,  false, false, false, false, false};
        case kCeC:      return {kPartCeCodes,    true,  true,  false, false, false, true,  true};
        default:        return {-1,              false, false, false, false, false, false, false};
    }
}
typedef int i32x4 __attribute__((ext_vector_type(4)));

}  // namespace
namespace vqi {
struct GumbelParams {
    const float *res;  // resident rows: x (kGumStats, kGumX) / the natural codebook (kGumC)
    long long res_rs, res_hs;
    const float *g;  // upstream gradient rows (kGumStats, kGumX)
    long long g_rs, g_hs;
    const float *img;  // streamed image of the two sweeps over s: packed codes / packed x rows (kGumC)
    long long img_hs;
    unsigned img_bytes;
    const float *gimg;  // kGumC: packed g rows (plain values)
    long long NR, NS;   // resident / streamed rows per head
    int D, ntiles, vec_res, vec_g;
    float tau;
    float *lse, *delta;  // [H][st_hs]: log2-domain log-sum-exp and delta per row m (written by kGumStats)
    long long st_hs;
    float *out;  // gx (kGumX) / the partials of gc (kGumC)
    long long out_rs, out_hs, out_zs;
    int tiles_per_split;  // kGumC / kDivC: streamed tiles per blockIdx.z
    // reinmax roles (lse / delta above: the log-sum-exp at tau and delta0)
    float *lse1;                   // [H][st_hs]: log2-domain log-sum-exp at temperature 1
    const long long *ind;          // kRmX: the caller's selection, (h, m) at ind[h*ind_hs + m*ind_rs]
    long long ind_rs, ind_hs;
    const int *ind32;              // kRmCol / kRmC: [H][st_hs] int32 copy, -1 past M
    float *col, *e;                // [H][ck_hs] per code (read by kRmX / kRmC)
    long long ck_hs;
    float *colp, *ep;              // kRmCol: partials [splits][H][ck_hs]
    long long cp_zs;
    // orthogonal role (kOrth): lse = rowsq [H][st_hs], out = G or null
    // cross-entropy role (kCeC): lse = the natural-log log-sum-exp [H][st_hs], ind32 = the targets (-1: ignored), out the partials of gc
    const float *coef;             // kCeC: one float, upstream gradient / number of non-ignored rows
    // diversity roles (tau = -T; lse: per row, kDivAcc / kDivC in image order; delta (kDivC: in image order); out: gx, kDivAcc
    // the per-head partials of A, kDivC the partials of gc)
    const float *U;                // kDivDelta / kDivX / kDivC: [N][U_rs], finite past K
    long long U_rs, gimg_hs;       // gimg (kDivX): the packed live codes or null, head stride gimg_hs
    int div_N, div_posdiv;         // position of row m: (m / div_posdiv) % div_N
    int div_spp, div_ch, div_pps;  // kDivAcc / kDivC: sub-tiles per position, rows per position and head; kDivAcc: positions per blockIdx.z
};
}  // namespace vqi
namespace {
using vqi::GumbelParams;

template <int DP>
struct GumGeo {
    static constexpr int V = DP >= 128 ? 4 : DP / 32;  // floats per A-fragment read of the contraction (positions V i + e)
    static constexpr int NJ = DP / (32 * V);           // 128-wide (V = 4) position blocks
    static constexpr int NACC = DP / 32;               // 32x32 accumulators of the gradient
    static constexpr int GS = DP + 4;                  // staging row stride (floats)
};

// both products over one staged tile: every fragment read feeds the s and the a accumulator
template <int DP>
__device__ __forceinline__ void mfma_range2(f32x16 &acc, f32x16 &acc2, f32x4 (&a)[DP / 8], const f32x4 *ta,
                                            const float (&xf)[DP / 2], const float (&gf)[DP / 2]) {
    constexpr int NG = FragPipe<DP>::NG, PF = FragPipe<DP>::PF;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + PF < NG) a[g + PF] = ta[2 * (g + PF)];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].x, xf[4 * g + 0], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].x, gf[4 * g + 0], acc2, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].y, xf[4 * g + 1], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].y, gf[4 * g + 1], acc2, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].z, xf[4 * g + 2], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].z, gf[4 * g + 2], acc2, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].w, xf[4 * g + 3], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].w, gf[4 * g + 3], acc2, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the weight through the similarity (kDivC, kCeC, kDivX): dot w as it stands; Euclid r = w / s with s = -dist = -sqrt(tc), and at
// s == 0 ATen's subgradient 0 (a NaN stays a NaN)
template <bool EUCLID>
__device__ __forceinline__ float euclid_ratio(float v, float tc) {
    if (EUCLID) {
        v = -v * __builtin_amdgcn_rsqf(tc);
        if (tc == 0.0f) v = 0.0f;
    }
    return v;
}

template <int DP, int METRIC, int ROLE>
__global__ void __launch_bounds__(256, (DP <= 64 ? 2 : 1)) vq_gumbel_sweep(const GumbelParams p) {
    constexpr int WAVES = 4;
    using G = Geo<DP, WAVES>;
    using GG = GumGeo<DP>;
    constexpr int RS = G::RS, RS4 = G::RS4, SUB = G::SUB, NG = DP / 8, V = GG::V, NJ = GG::NJ, NACC = GG::NACC;
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    constexpr SweepRole R = sweep_role(ROLE);  // (the fields are described at the table)
    constexpr bool DIV = R.one_product;  // (the diversity roles, kOrth and kCeC)
    constexpr bool CODES = R.codes_resident;
    constexpr bool RM = R.reinmax;
    constexpr bool COLS = (ROLE == kRmCol);
    constexpr bool STATS = R.no_contraction;
    constexpr bool GIMG = R.second_image;
    constexpr bool XNORM_FIRST = R.xnorm_first;
    constexpr int IMG_F4 = 2 * G::BUF_F4;  // the two tile buffers of one image
    constexpr float LOG2E = 1.4426950408889634f;
    const float INF = __builtin_inff();

    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4 *tile4 = (f32x4 *)smem;
    lds_f32x4 *tile4_lds = (lds_f32x4 *)smem;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const long long row0 = ((long long)blockIdx.x * WAVES + wave) * 32;
    const float *rh = p.res + (long long)head * p.res_hs;

    float rf[DP / 2];
    float rn0 = 0.0f;
    load_x_fragments<G::CH, G::XS, DP / G::CH, EUCLID>(rh, p.res_rs, p.NR, p.D, p.vec_res, row0, true, smem, wave, lane, rf, rn0);
    __syncthreads();  // (the staging regions are reused: by the second pass, then as tile buffers)
    float gf[(CODES || DIV) ? 1 : DP / 2];
    if constexpr (!CODES && !DIV) {
        float unused = 0.0f;
        load_x_fragments<G::CH, G::XS, DP / G::CH, false>(p.g + (long long)head * p.g_hs, p.g_rs, p.NR, p.D, p.vec_g, row0, true, smem,
                                                          wave, lane, gf, unused);
        __syncthreads();
    }

    const long long row = row0 + c;
    const bool row_ok = row < p.NR;
    const float *img = p.img + (long long)head * p.img_hs;
    const bool live = (ROLE == kDivX) && p.gimg != nullptr;  // (workgroup-uniform) contract with the tile of a second image
    const bool contract = ROLE != kOrth || p.out != nullptr;  // (workgroup-uniform) kOrth without G: rowsq only
    const float *gimg = GIMG ? p.gimg + (long long)head * p.img_hs : (live ? p.gimg + (long long)head * p.gimg_hs : nullptr);
    // (kDivAcc / kDivC: the streamed row's norm first, as in the rows-resident roles -- its similarities are theirs bit for bit;
    // kCeC: as in vq_sweep_aux, whose log-sum-exp it reads)
    const float b_aug = XNORM_FIRST ? (h ? rn0 : 1.0f) : (h ? 1.0f : rn0);
    const float tau2 = p.tau * LOG2E;
    const long long st0 = (long long)head * p.st_hs;

    // per resident row (kGumX): the statistics of this lane's row
    float lse_row = 0.0f, delta_row = 0.0f;
    if ((ROLE == kGumX || ROLE == kRmX || ROLE == kDivX) && row_ok) {
        lse_row = p.lse[st0 + row];
        delta_row = p.delta[st0 + row];
    }
    // diversity: the row of U of this lane's sequence position
    const float *u_row = nullptr;
    if constexpr (ROLE == kDivDelta || ROLE == kDivX) {
        if (ROLE == kDivDelta && row_ok) lse_row = p.lse[st0 + row];
        u_row = p.U + (row_ok ? (row / p.div_posdiv) % p.div_N : 0) * p.U_rs;
    }
    // reinmax: kRmX the rest of the row's statistics and its selected code; kRmC the lane's own code's 1 / col and e
    float lse1_row = 0.0f, rcol_own = 0.0f, e_own = 0.0f;
    float coef = 0.0f;
    if constexpr (ROLE == kCeC) coef = *p.coef;
    long long ind_row = -1;
    if (ROLE == kRmX && row_ok) {
        lse1_row = p.lse1[st0 + row];
        ind_row = p.ind[(long long)head * p.ind_hs + row * p.ind_rs];
    }
    if (ROLE == kRmC && row_ok) {
        rcol_own = __builtin_amdgcn_rcpf(p.col[(long long)head * p.ck_hs + row]);
        e_own = p.e[(long long)head * p.ck_hs + row];
    }
    // kGumStats: running max / sum of exp2 / sum of exp2 * a over the codes this lane has seen
    // (kRmStats: run_m in units of log2 e s, run_s at tau, run_s1 and run_d at temperature 1; kRmCol: run_s = sum p1, run_d = sum p1 a)
    float run_m = -INF, run_s = 0.0f, run_d = 0.0f, run_s1 = 0.0f;

    f32x16 gacc[STATS ? 1 : NACC];
#pragma unroll
    for (int j = 0; j < (STATS ? 1 : NACC); ++j) gacc[j] = (f32x16){0};
    float sum_ratio = 0.0f;

    auto stage = [&](int tile, int buf) {
#pragma unroll
        for (int i = 0; i < (G::TILE_CHUNKS + WAVES - 1) / WAVES; ++i) {
            const int ck = i * WAVES + wave;
            if (ck < G::TILE_CHUNKS) {
                lds_dma16(img, p.img_bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16, tile4_lds + buf * G::BUF_F4 + ck * 64);
                if constexpr (GIMG)
                    lds_dma16(gimg, p.img_bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16,
                              tile4_lds + IMG_F4 + buf * G::BUF_F4 + ck * 64);
                if constexpr (ROLE == kDivX) {
                    if (live)
                        lds_dma16(gimg, p.img_bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16,
                                  tile4_lds + IMG_F4 + buf * G::BUF_F4 + ck * 64);
                }
            }
        }
    };

    int t_begin = 0, t_end = p.ntiles;
    if constexpr (R.z_splits_tiles) {
        t_begin = (int)blockIdx.z * p.tiles_per_split;
        t_end = t_begin + p.tiles_per_split < p.ntiles ? t_begin + p.tiles_per_split : p.ntiles;
    }
    // kDivAcc: the sub-tiles [u_lo, u_hi) of this split's positions, and the staged tiles that hold them
    int u_lo = 0, u_hi = 0;
    if constexpr (ROLE == kDivAcc) {
        const int n0 = (int)blockIdx.z * p.div_pps;
        const int n1 = n0 + p.div_pps < p.div_N ? n0 + p.div_pps : p.div_N;
        u_lo = n0 * p.div_spp;
        u_hi = n1 * p.div_spp;
        t_begin = u_lo / SUB;
        t_end = (u_hi + SUB - 1) / SUB;
    }
    // kDivC: U[n][own code] of the position the sweep is in
    int u_pos = -1;
    float u_own = 0.0f;
    stage(t_begin, 0);
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
        const int cur = (t - t_begin) & 1;
        if (t + 1 < t_end) stage(t + 1, cur ^ 1);
#pragma unroll 1
        for (int st = 0; st < SUB; ++st) {
            const int u = t * SUB + st;
            if ((long long)u * kTileCodes >= p.NS) break;  // workgroup-uniform: nothing but padding from here on
            if constexpr (ROLE == kDivAcc) {
                if (u < u_lo) continue;  // (a neighbour split's position in the same staged tile)
                if (u >= u_hi) break;
            }
            const f32x4 *tb = tile4 + cur * G::BUF_F4 + st * (kTileCodes * RS4);
            const long long sbase = (long long)u * kTileCodes + 4 * h;  // streamed row of this lane's register 0
            // kGumC: the statistics of the 16 streamed rows this lane's registers stand for (rows 8 g + 4 h + 0..3 of the sub-tile)
            f32x4 l4[4], d4[4];
            if constexpr (CODES && !RM && ROLE != kCeC) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    l4[g] = *(const f32x4 *)(p.lse + st0 + sbase + 8 * g);
                    if constexpr (!DIV || ROLE == kDivC) d4[g] = *(const f32x4 *)(p.delta + st0 + sbase + 8 * g);
                }
            }
            // ---- the two products: acc = t (squared distance / dot product), acca = the image's multiple of a
            f32x16 acc = {0}, acca = {0};
            {
                const f32x4 *ta = tb + c * RS4 + h;
                f32x4 a[NG];
                const float cnv = EUCLID ? ((const float *)tb)[c * RS + DP] : 0.0f;
                mfma_prefetch<DP>(a, ta);
                if constexpr (CODES || DIV) mfma_range<DP, 0, NG>(acc, a, ta, rf);
                else mfma_range2<DP>(acc, acca, a, ta, rf, gf);
                if (EUCLID) {
                    const float a_aug = XNORM_FIRST ? (h ? 1.0f : cnv) : (h ? cnv : 1.0f);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
                }
            }
            if constexpr (GIMG) {
                const f32x4 *ta = tb + IMG_F4 + c * RS4 + h;
                f32x4 a[NG];
                mfma_prefetch<DP>(a, ta);
                mfma_range<DP, 0, NG>(acca, a, ta, rf);
            }
            // (the codebook image of the Euclid metric holds -2 c; the image of the g rows holds g)
            const float a_scale = (EUCLID && !CODES) ? -0.5f : 1.0f;
            if constexpr (ROLE == kDivAcc) {
                // ---- p of the 16 streamed rows of this lane's registers; row j of the position is real while j < div_ch
                const int jb = (u % p.div_spp) * kTileCodes + 4 * h;
                float sum_p = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float tv = acc[r];
                    const float lse2 = l4[r >> 2][r & 3];
                    // (the logit exactly as kDivStats rounded it, then minus the row's lse2: the p of a row sum to 1 within rounding)
                    const float lg = EUCLID ? -tau2 * __builtin_amdgcn_sqrtf(tv < 0.0f ? 0.0f : tv) : tau2 * tv;
                    const float pr = __builtin_amdgcn_exp2f(lg - lse2);
                    sum_p += (jb + (r & 3) + 8 * (r >> 2) < p.div_ch) ? pr : 0.0f;
                }
                run_s += sum_p;
                if ((u + 1) % p.div_spp == 0) {  // the position's last sub-tile: its sum over the rows of this head is complete
                    const float tot = run_s + __shfl_xor(run_s, 32);
                    if (h == 0 && row_ok) p.out[(long long)head * p.out_hs + (long long)(u / p.div_spp) * p.out_rs + row] = tot;
                    run_s = 0.0f;
                }
            } else if constexpr (ROLE == kDivC) {
                // ---- acc[r] <- w (dot) / r = w / s (Euclid) of (streamed row r of the position, this lane's code), w = tau p (U - delta)
                const int n = u / p.div_spp;
                if (n != u_pos) {  // (workgroup-uniform)
                    u_pos = n;
                    u_own = row_ok ? p.U[(long long)n * p.U_rs + row] : 0.0f;
                }
                const int jb = (u % p.div_spp) * kTileCodes + 4 * h;
                float sum_u = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float tv = acc[r];
                    const float tc = tv < 0.0f ? 0.0f : tv;  // (keeps a NaN, unlike fmaxf)
                    const float lg = EUCLID ? -tau2 * __builtin_amdgcn_sqrtf(tc) : tau2 * tv;  // as kDivStats rounded it
                    const float pr = __builtin_amdgcn_exp2f(lg - l4[r >> 2][r & 3]);
                    float v = (p.tau * pr) * (u_own - d4[r >> 2][r & 3]);
                    v = euclid_ratio<EUCLID>(v, tc);
                    // row j of the position is real while j < div_ch; a padding row gives inf / NaN under Euclid: select, never multiply
                    v = (jb + (r & 3) + 8 * (r >> 2) < p.div_ch) ? v : 0.0f;
                    acc[r] = v;
                    sum_u += v;
                }
                sum_ratio += sum_u;
            } else if constexpr (ROLE == kCeC) {
                // ---- acc[r] <- w (dot) / r = w / s (Euclid) of (streamed row sbase + 8 g + q, this lane's code), w = coef (p - onehot)
                float sum_u = 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 ls4 = *(const f32x4 *)(p.lse + st0 + sbase + 8 * g);
                    const i32x4 t4 = *(const i32x4 *)(p.ind32 + st0 + sbase + 8 * g);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int r = 4 * g + q;
                        const float tv = acc[r];
                        const float tc = tv < 0.0f ? 0.0f : tv;  // (keeps a NaN, unlike fmaxf)
                        const float sv = EUCLID ? -__builtin_amdgcn_sqrtf(tc) : tv;  // the logit vq_sweep_aux summed
                        const float pr = __builtin_amdgcn_exp2f((sv - ls4[q]) * LOG2E);
                        float v = coef * (pr - (((long long)t4[q] == row) ? 1.0f : 0.0f));
                        v = euclid_ratio<EUCLID>(v, tc);
                        // an ignored row and a row past M: its x, its lse and with them v may be NaN / inf -- select, never multiply
                        v = t4[q] >= 0 ? v : 0.0f;
                        acc[r] = v;
                        sum_u += v;
                    }
                }
                sum_ratio += sum_u;
            } else if constexpr (ROLE == kOrth) {
                // ---- acc[r] <- cos of (streamed row sbase + (r&3) + 8(r>>2), this lane's resident row), 0 by index in the padding
                float sq = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool pad = !row_ok || sbase + (r & 3) + 8 * (r >> 2) >= p.NS;
                    const float v = pad ? 0.0f : acc[r];
                    acc[r] = v;
                    sq = fmaf(v, v, sq);
                }
                run_s += sq;
            } else if constexpr (ROLE == kDivDelta || ROLE == kDivX) {
                // ---- kDivDelta: run_d += p U;  kDivX: acc[r] <- w (dot) / r = w / s (Euclid) in place, w = tau p (U - delta)
                float sum_u = 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 u4 = *(const f32x4 *)(u_row + sbase + 8 * g);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int r = 4 * g + q;
                        const bool pad = sbase + 8 * g + q >= p.NS;  // padding codes of the streamed image
                        const float tv = acc[r];
                        const float tc = tv < 0.0f ? 0.0f : tv;  // (keeps a NaN, unlike fmaxf)
                        const float lg = EUCLID ? -tau2 * __builtin_amdgcn_sqrtf(tc) : tau2 * tv;  // as kDivStats rounded it
                        const float pr = __builtin_amdgcn_exp2f(lg - lse_row);
                        if constexpr (ROLE == kDivDelta) {
                            run_s += pad ? 0.0f : pr;
                            run_d += pad ? 0.0f : pr * u4[q];
                        } else {
                            float v = (p.tau * pr) * (u4[q] - delta_row);
                            v = euclid_ratio<EUCLID>(v, tc);
                            if (pad) v = 0.0f;
                            acc[r] = v;
                            sum_u += v;
                        }
                    }
                }
                sum_ratio += sum_u;
            } else if constexpr (ROLE == kRmStats) {
                float b[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float tv = acc[r];
                    b[r] = EUCLID ? -LOG2E * __builtin_amdgcn_sqrtf(fmaxf(tv, 0.0f)) : LOG2E * tv;
                    if (sbase + (r & 3) + 8 * (r >> 2) >= p.NS) b[r] = -INF;
                }
                float tm = b[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) tm = fmaxf(tm, b[r]);
                if (tm > run_m) {
                    const float df = run_m - tm;  // -inf on the first visit: both factors 0
                    const float sc1 = __builtin_amdgcn_exp2f(df);
                    run_s *= __builtin_amdgcn_exp2f(p.tau * df);
                    run_s1 *= sc1;
                    run_d *= sc1;
                    run_m = tm;
                }
                if (run_m > -INF) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float df = b[r] - run_m;
                        const float e1 = __builtin_amdgcn_exp2f(df);
                        run_s += __builtin_amdgcn_exp2f(p.tau * df);
                        run_s1 += e1;
                        run_d = fmaf(e1, a_scale * acca[r], run_d);
                    }
                }
            } else if constexpr (RM) {
                // ---- reinmax: p1, then the column sums (kRmCol) or acc[r] <- w / r in place (kRmX, kRmC); the per-streamed
                // arrays are read four registers' worth at a time (rows / codes sbase + 8 g + 0..3)
                float sum_u = 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 lt4 = {0}, l14 = {0}, dl4 = {0}, c4 = {0}, e4 = {0};
                    i32x4 i4 = {0};
                    if constexpr (CODES) {
                        lt4 = *(const f32x4 *)(p.lse + st0 + sbase + 8 * g);
                        i4 = *(const i32x4 *)(p.ind32 + st0 + sbase + 8 * g);
                        if constexpr (!COLS) {
                            l14 = *(const f32x4 *)(p.lse1 + st0 + sbase + 8 * g);
                            dl4 = *(const f32x4 *)(p.delta + st0 + sbase + 8 * g);
                        }
                    } else {
                        c4 = *(const f32x4 *)(p.col + (long long)head * p.ck_hs + sbase + 8 * g);
                        e4 = *(const f32x4 *)(p.e + (long long)head * p.ck_hs + sbase + 8 * g);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int r = 4 * g + q;
                        const long long sidx = sbase + 8 * g + q;
                        const bool pad = sidx >= p.NS;  // padding rows / codes of the streamed image
                        const float tv = acc[r];
                        const float av = a_scale * acca[r];
                        const float tc = fmaxf(tv, 0.0f);
                        const float dist = __builtin_amdgcn_sqrtf(tc);
                        const float lse2 = CODES ? lt4[q] : lse_row;
                        const float pt = __builtin_amdgcn_exp2f(EUCLID ? fmaf(dist, -tau2, -lse2) : fmaf(tv, tau2, -lse2));
                        const bool hot = CODES ? ((long long)i4[q] == row) : (ind_row == sidx);
                        const float p1 = fmaxf(0.5f * ((hot ? 1.0f : 0.0f) + pt), 1e-5f);
                        if constexpr (COLS) {
                            const float pm = pad ? 0.0f : p1;  // (the clamp made 1e-5 of a padding row)
                            run_s += pm;
                            run_d = fmaf(pm, pad ? 0.0f : av, run_d);
                        } else {
                            const float lse1 = CODES ? l14[q] : lse1_row;
                            const float dl = CODES ? dl4[q] : delta_row;
                            const float rc = CODES ? rcol_own : __builtin_amdgcn_rcpf(c4[q]);
                            const float ek = CODES ? e_own : e4[q];
                            const float p0 = __builtin_amdgcn_exp2f(EUCLID ? fmaf(dist, -LOG2E, -lse1) : fmaf(tv, LOG2E, -lse1));
                            float v = (2.0f * p1 * rc) * (av - ek) - (0.5f * p0) * (av - dl);
                            if (EUCLID) v = -v * __builtin_amdgcn_rsqf(tc);  // w / s with s = -dist; inf / nan at dist == 0
                            if (!(__builtin_fabsf(v) < INF)) v = 0.0f;       // 1 / 0: ATen's subgradient 0
                            if (pad) v = 0.0f;
                            acc[r] = v;
                            sum_u += v;
                        }
                    }
                }
                sum_ratio += sum_u;
            } else if constexpr (STATS) {
                float l[16];
                bool nan_seen = false;  // kDivStats: a NaN similarity makes the row's lse2 NaN (fmaxf below would drop it)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float tv = acc[r];
                    if constexpr (DIV) l[r] = EUCLID ? -tau2 * __builtin_amdgcn_sqrtf(tv < 0.0f ? 0.0f : tv) : tau2 * tv;
                    else l[r] = EUCLID ? -tau2 * __builtin_amdgcn_sqrtf(fmaxf(tv, 0.0f)) : tau2 * tv;
                    if (sbase + (r & 3) + 8 * (r >> 2) >= p.NS) l[r] = -INF;
                    if constexpr (DIV) nan_seen |= l[r] != l[r];
                }
                float tm = l[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) tm = fmaxf(tm, l[r]);
                if (tm > run_m) {
                    const float sc = __builtin_amdgcn_exp2f(run_m - tm);  // exp2(-inf) = 0 on the first visit
                    run_s *= sc;
                    run_d *= sc;
                    run_m = tm;
                }
                if (run_m > -INF) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float e = __builtin_amdgcn_exp2f(l[r] - run_m);
                        run_s += e;
                        if constexpr (!DIV) run_d = fmaf(e, a_scale * acca[r], run_d);
                    }
                }
                if constexpr (DIV) {
                    if (nan_seen) run_s = __builtin_nanf("");
                }
            } else {
                // ---- acc[r] <- w (dot) / r = w / s (Euclid) of (streamed row sbase + (r&3) + 8(r>>2), this lane's resident row)
                float sum_u = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float lse2 = CODES ? l4[r >> 2][r & 3] : lse_row;
                    const float dl = CODES ? d4[r >> 2][r & 3] : delta_row;
                    const float tv = acc[r];
                    const float av = a_scale * acca[r];
                    float v;
                    if (EUCLID) {
                        const float tc = fmaxf(tv, 0.0f);
                        const float dist = __builtin_amdgcn_sqrtf(tc), rs = __builtin_amdgcn_rsqf(tc);
                        const float pr = __builtin_amdgcn_exp2f(fmaf(dist, -tau2, -lse2));
                        v = -((p.tau * pr) * (av - dl)) * rs;  // w / s with s = -dist; inf / nan at dist == 0 (fixed below)
                    } else {
                        const float pr = __builtin_amdgcn_exp2f(fmaf(tv, tau2, -lse2));
                        v = (p.tau * pr) * (av - dl);
                    }
                    if (!(__builtin_fabsf(v) < INF)) v = 0.0f;                  // 1 / 0: ATen's subgradient 0
                    if (sbase + (r & 3) + 8 * (r >> 2) >= p.NS) v = 0.0f;       // padding rows of the streamed image
                    acc[r] = v;
                    sum_u += v;
                }
                sum_ratio += sum_u;
            }
            if constexpr (!STATS) if (contract) {
                // ---- contraction: gacc[J*V + e][position i, resident row] += img[streamed row (r, half)][128 J + V i + e] * acc[r]
                const float *trow = (const float *)(live ? tb + IMG_F4 : tb) + (4 * h) * RS + V * c;
                if constexpr (V == 4) {
                    constexpr int NSEQ = NJ * 16, PF = 4;
                    auto frag = [&](int n) -> f32x4 {
                        const int J = n >> 4, r = n & 15;
                        return *(const f32x4 *)(trow + ((r & 3) + 8 * (r >> 2)) * RS + 128 * J);
                    };
                    f32x4 af[NSEQ];
#pragma unroll
                    for (int n = 0; n < PF; ++n) af[n] = frag(n);
#pragma unroll
                    for (int n = 0; n < NSEQ; ++n) {
                        if (n + PF < NSEQ) af[n + PF] = frag(n + PF);
                        const int J = n >> 4, r = n & 15;
                        gacc[J * 4 + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].x, acc[r], gacc[J * 4 + 0], 0, 0, 0);
                        gacc[J * 4 + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].y, acc[r], gacc[J * 4 + 1], 0, 0, 0);
                        gacc[J * 4 + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].z, acc[r], gacc[J * 4 + 2], 0, 0, 0);
                        gacc[J * 4 + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].w, acc[r], gacc[J * 4 + 3], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float *ap = trow + ((r & 3) + 8 * (r >> 2)) * RS;
                        if (V == 2) {
                            const float a0 = ap[0], a1 = ap[1];
                            gacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, acc[r], gacc[0], 0, 0, 0);
                            gacc[NACC > 1 ? 1 : 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, acc[r], gacc[NACC > 1 ? 1 : 0], 0, 0, 0);
                        } else {
                            gacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[0], acc[r], gacc[0], 0, 0, 0);
                        }
                        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound the fragment reads in flight
                    }
                }
            }
        }
        __syncthreads();  // next tile landed, everybody is done reading this one
    }

    if constexpr (ROLE == kDivAcc) {
        // (every position was flushed inside the sweep)
    } else if constexpr (ROLE == kDivDelta) {
        // (divided by the p that were summed, 1 within rounding: sum_k w_k = 0 then holds for the p kDivX recomputes)
        run_s += __shfl_xor(run_s, 32);
        run_d += __shfl_xor(run_d, 32);
        if (h == 0 && row_ok) p.delta[st0 + row] = run_d / run_s;
    } else if constexpr (COLS) {
        // the two lane halves hold the two halves of every sub-tile's rows; one partial per (split, code)
        run_s += __shfl_xor(run_s, 32);
        run_d += __shfl_xor(run_d, 32);
        if (h == 0 && row_ok) {
            const long long o = (long long)blockIdx.z * p.cp_zs + (long long)head * p.ck_hs + row;
            p.colp[o] = run_s;
            p.ep[o] = run_d;
        }
    } else if constexpr (ROLE == kRmStats) {
        const float om = __shfl_xor(run_m, 32), os = __shfl_xor(run_s, 32), os1 = __shfl_xor(run_s1, 32), od = __shfl_xor(run_d, 32);
        const float mm = fmaxf(run_m, om);  // lane half 0 always saw streamed row 0, so mm is finite
        const bool mine = run_m > -INF, other = om > -INF;
        const float w0 = mine ? __builtin_amdgcn_exp2f(run_m - mm) : 0.0f, w1 = other ? __builtin_amdgcn_exp2f(om - mm) : 0.0f;
        const float t0 = mine ? __builtin_amdgcn_exp2f(p.tau * (run_m - mm)) : 0.0f;
        const float t1 = other ? __builtin_amdgcn_exp2f(p.tau * (om - mm)) : 0.0f;
        const float st = run_s * t0 + os * t1;
        const float s1 = run_s1 * w0 + os1 * w1;
        const float d = run_d * w0 + od * w1;
        if (h == 0 && row_ok) {
            p.lse[st0 + row] = fmaf(p.tau, mm, __builtin_amdgcn_logf(st));
            p.lse1[st0 + row] = mm + __builtin_amdgcn_logf(s1);
            p.delta[st0 + row] = d / s1;
        }
    } else if constexpr (STATS) {
        const float om = __shfl_xor(run_m, 32), os = __shfl_xor(run_s, 32), od = __shfl_xor(run_d, 32);
        const float mm = fmaxf(run_m, om);  // lane half 0 always saw streamed row 0, so mm is finite
        const float w0 = run_m > -INF ? __builtin_amdgcn_exp2f(run_m - mm) : 0.0f;
        const float w1 = om > -INF ? __builtin_amdgcn_exp2f(om - mm) : 0.0f;
        const float s = run_s * w0 + os * w1;
        const float d = run_d * w0 + od * w1;
        if (h == 0 && row_ok) {
            p.lse[st0 + row] = mm + __builtin_amdgcn_logf(s);
            if constexpr (!DIV) p.delta[st0 + row] = d / s;
        }
    } else {
        if constexpr (ROLE == kOrth) {
            // the two lane halves hold the two halves of every sub-tile's codes
            run_s += __shfl_xor(run_s, 32);
            if (h == 0 && row_ok) p.lse[st0 + row] = run_s;
            if (p.out == nullptr) return;  // (workgroup-uniform, behind the last barrier)
        }
        // ---------------- finalize: fragment layout -> natural rows through LDS ----------------
        // (the loop's last barrier guarantees nobody reads the tile buffers any more; the region is wave-private)
        constexpr int GS = GG::GS;
        float *stg = smem + wave * (32 * GS + 32);
        float *srs = stg + 32 * GS;
        sum_ratio += __shfl_xor(sum_ratio, 32);
        if (h == 0) srs[c] = sum_ratio;
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const int J = a / V, e = a % V;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 8 * (r >> 2) + 4 * h + (r & 3);  // MFMA i index held by this lane's register r
                const int pos = 32 * V * J + V * i + e;        // position in the packed row
                const int p8 = pos & 7;
                const int dim = (pos & ~7) + (p8 < 4 ? 2 * p8 : 2 * (p8 - 4) + 1);
                stg[c * GS + dim] = gacc[a][r];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private region: in-order LDS, no barrier needed
        const long long left = p.NR - row0;
        const int nrows = left >= 32 ? 32 : (left > 0 ? (int)left : 0);
        float *oh = p.out + (CODES ? (long long)blockIdx.z * p.out_zs : 0) + (long long)head * p.out_hs;
        for (int rr = 0; rr < nrows; ++rr) {
            const float sr = srs[rr];
            const float *xr = rh + (row0 + rr) * p.res_rs;
            float *orow = oh + (row0 + rr) * p.out_rs;
            for (int d = lane; d < p.D; d += 64) {
                const float gv = stg[rr * GS + d];
                // Euclid: x rowsum(r) - r c  with the image holding -2 c (kGumC: c colsum(r) - r^T x, image -2 x)
                orow[d] = EUCLID ? fmaf(xr[d], sr, 0.5f * gv) : gv;
            }
        }
    }
}

// packed images of the x rows (metric-scaled, |x|^2 behind every row: vq_pack.inc layout) and of the g rows (plain) for
// kGumC; rows may be strided.  One thread per packed row; rows past M are zero (|x|^2 = +inf under Euclid, as for padding codes).
// With a RowMap (Cp > 0; the diversity loss, g == nullptr: no g image) the image is position-major: image row n Cp + j holds
// row j of sequence position n for j < C -- source row ((j / pos_div) N + n) pos_div + j % pos_div, the j-th row m in
// ascending order with (m / pos_div) % N == n -- and padding for C <= j < Cp and past N Cp; `stat` (a per-row array,
// [head][stat_hs]) is copied along in image order, 0 in the padding, and so is `stat2` when it is given (same strides).
// With `keep` (the cross-entropy loss: the int32 targets vq_gumbel_pack_ind wrote) a row whose entry is negative is packed as
// padding and its x is not read: a NaN / inf there must not meet the zero weight of the row in the contraction.
}  // namespace
namespace vqi {
struct RowMap {
    long long C, Cp;  // rows per position and head; the same padded to whole sub-tiles (0: image row m = source row m)
    int N, pos_div;
    const float *stat;
    float *stat_img;
    long long stat_hs, stat_img_hs;
    const float *stat2;  // optional second per-row array (kDivC: delta beside lse2)
    float *stat2_img;
    const int *keep;  // optional (kCeC, Cp == 0): [head][keep_hs], image row m is real only where keep >= 0
    long long keep_hs;
};
}  // namespace vqi
namespace {
using vqi::RowMap;
__global__ void __launch_bounds__(64) vq_gumbel_pack_rows(const float *__restrict__ x, long long x_rs, long long x_hs,
                                                          const float *__restrict__ g, long long g_rs, long long g_hs, long long M,
                                                          long long Mp, int D, int DP, int metric, float *__restrict__ ximg,
                                                          float *__restrict__ gimg, long long img_hs, const RowMap map) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= Mp) return;
    const int RS = DP + 4;
    bool real = m < M;
    if (map.keep && real) real = map.keep[(long long)blockIdx.y * map.keep_hs + m] >= 0;
    long long src = m;
    if (map.Cp > 0) {
        const long long n = m / map.Cp, j = m % map.Cp;
        real = n < map.N && j < map.C;
        src = ((j / map.pos_div) * map.N + n) * map.pos_div + j % map.pos_div;
        map.stat_img[(long long)blockIdx.y * map.stat_img_hs + m] = real ? map.stat[(long long)blockIdx.y * map.stat_hs + src] : 0.0f;
        if (map.stat2)
            map.stat2_img[(long long)blockIdx.y * map.stat_img_hs + m] = real ? map.stat2[(long long)blockIdx.y * map.stat_hs + src] : 0.0f;
    }
    const float *xs = x + (long long)blockIdx.y * x_hs + (real ? src : 0) * x_rs;
    const float *gs = g ? g + (long long)blockIdx.y * g_hs + (real ? src : 0) * g_rs : xs;
    float *xd = ximg + (long long)blockIdx.y * img_hs + m * RS;
    float *gd = gimg + (long long)blockIdx.y * img_hs + m * RS;
    const float scale = (metric == VQ_METRIC_EUCLID) ? -2.0f : 1.0f;
    float cn = 0.0f;
    for (int g8 = 0; g8 < DP / 8; ++g8) {
        float v[8], w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = 8 * g8 + e;
            const bool in = real && d < D;
            v[e] = in ? xs[d] : 0.0f;
            w[e] = in ? gs[d] : 0.0f;
            cn = fmaf(v[e], v[e], cn);  // d-ordered chain; padded zeros leave it unchanged
        }
        *(f32x4 *)(xd + 8 * g8) = (f32x4){scale * v[0], scale * v[2], scale * v[4], scale * v[6]};
        *(f32x4 *)(xd + 8 * g8 + 4) = (f32x4){scale * v[1], scale * v[3], scale * v[5], scale * v[7]};
        if (g) {
            *(f32x4 *)(gd + 8 * g8) = (f32x4){w[0], w[2], w[4], w[6]};
            *(f32x4 *)(gd + 8 * g8 + 4) = (f32x4){w[1], w[3], w[5], w[7]};
        }
    }
    const float chain = real ? cn : 0.0f;
    if (!real) cn = __builtin_inff();
    *(f32x4 *)(xd + DP) = (f32x4){(metric == VQ_METRIC_EUCLID) ? cn : 0.0f, 1.0f, chain, 0.0f};
    if (g) *(f32x4 *)(gd + DP) = (f32x4){0.0f, 1.0f, 0.0f, 0.0f};
}

// gc[i] = parts[0][i] + parts[1][i] + ... in this order, i over [H, K, D]
__global__ void __launch_bounds__(256) vq_gumbel_reduce_parts(const float *__restrict__ parts, long long n, int splits,
                                                              float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = parts[i];
    for (int z = 1; z < splits; ++z) s += parts[(long long)z * n + i];
    out[i] = s;
}

// the int32 copy of ind the codes-resident reinmax roles read 16 bytes at a time: [H][stride], -1 past M and for values no
// code index can equal (the copy is only ever compared).  K > 0 (kCeC: ind is the target of the cross entropy): a value >= K
// is -1 too -- the 64-bit value is compared, before the narrowing -- and `stat` [H][stat_hs] (the log-sum-exp, rows of M
// floats) is copied along to stat_out [H][stride], 0 past M.
__global__ void __launch_bounds__(256) vq_gumbel_pack_ind(const long long *__restrict__ ind, long long ind_rs, long long ind_hs, long long M,
                                                          long long stride, int *__restrict__ out, int K, const float *__restrict__ stat,
                                                          long long stat_hs, float *__restrict__ stat_out) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= stride) return;
    int v = -1;
    if (m < M) {
        const long long i = ind[(long long)blockIdx.y * ind_hs + m * ind_rs];
        if (i >= 0 && i <= 0x7FFFFFFFll && (K <= 0 || i < K)) v = (int)i;
    }
    out[(long long)blockIdx.y * stride + m] = v;
    if (stat) stat_out[(long long)blockIdx.y * stride + m] = m < M ? stat[(long long)blockIdx.y * stat_hs + m] : 0.0f;
}

// col[h][k] = colp[0] + colp[1] + ... and e[h][k] = (ep[0] + ep[1] + ...) / col in this order; 1 / 0 in the padding past K
__global__ void __launch_bounds__(256) vq_gumbel_reduce_cols(const float *__restrict__ colp, const float *__restrict__ ep, long long n,
                                                             long long stride, int K, int splits, float *__restrict__ col,
                                                             float *__restrict__ e) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i % stride >= K) {
        col[i] = 1.0f;
        e[i] = 0.0f;
        return;
    }
    float cs = colp[i], es = ep[i];
    for (int z = 1; z < splits; ++z) {
        cs += colp[(long long)z * n + i];
        es += ep[(long long)z * n + i];
    }
    col[i] = cs;
    e[i] = es / cs;
}
