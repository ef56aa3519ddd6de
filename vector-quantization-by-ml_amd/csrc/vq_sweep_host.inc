// vq_sweep_host.inc -- host side of the resident/streamed sweep (the fourteen roles of vq_gumbel.inc): the Gumbel
// straight-through and reinmax backward, the codebook diversity loss, the cross-entropy loss's codes gradient and the orthogonal
// regularisation loss.  Included by vq_kernels.hip in build part 0, inside its extern "C" block: the vq_* functions below are
// the C ABI (include/vq_mi355x.h), everything else is static.
// ------------------------------------------------------------------------------------------------
// Rows-resident entries (stats, delta, backward_x, orthogonal_gram): fill_gumbel_rows, launch_gumbel.
// Codes-resident entries (backward_codes, reinmax_columns, diversity_accumulate): a wave owns 32 codes and the packed rows are
// streamed from an image in the workspace, split over blockIdx.z.  ONE path: plan_sweep (image geometry, split, workspace
// regions), fill_gumbel_codes (checks + every codes-resident field), pack_gumbel_rows, launch_gumbel, and for a [K, D] gradient
// sweep_grad_codes.
int64_t vq_gumbel_row_stride(int64_t M) { return M <= 0 ? 0 : (M + 255) / 256 * 256; }

// The split of `units` (staged tiles; positions for kDivAcc) over blockIdx.z: every CU a workgroup (a workgroup owns 128 codes
// of one head), at most 64 splits, at least one unit each, regrouped into equal runs.
struct UnitSplit {
    int per_split, splits;
};
static UnitSplit split_units(int H, int K, long long units) {
    const long long blocks = (long long)((K + 127) / 128) * H;
    long long want = (device_cus() + blocks - 1) / blocks;
    if (want > 64) want = 64;
    if (want > units) want = units;
    if (want < 1) want = 1;
    UnitSplit u;
    u.per_split = (int)((units + want - 1) / want);
    u.splits = (int)((units + u.per_split - 1) / u.per_split);
    return u;
}

// The workspace of a codes-resident entry: the regions below in THIS order, each entry with its own count of every region
// (documented per entry in vq_mi355x.h).  Units in 4-byte words, img = the packed image of a head, rsM / rsK =
// vq_gumbel_row_stride(M / K); a position-major image (the diversity loss: every position's M / N rows of a head padded to whole
// 32-row sub-tiles) has N > 0 and its per-row arrays in image order, Mp per head:
//   kWsX      x image                H x img
//   kWsG      g image                H x img
//   kWsInt    int32 per row          H x rsM                   (reinmax: ind; cross entropy: the targets)
//   kWsStat   per-row statistics     H x rsM, or H x Mp in image order   (lse; lse2, delta)
//   kWsCols   column partials        splits x H x rsK          (reinmax: col, e)
//   kWsA      partials of A          H x N x rsK
//   kWsParts  grad_codes partials    splits x H x K x D, only when splits > 1
enum SweepRegion { kWsX, kWsG, kWsInt, kWsStat, kWsCols, kWsA, kWsParts, kWsRegions };
struct SweepEntry {
    unsigned char count[kWsRegions];
    bool position_major;   // the image of the diversity loss
    bool split_positions;  // blockIdx.z splits the positions (kDivAcc: no position is summed across workgroups), not the staged tiles
    const char *sizer;     // named by the "workspace too small" failure
};
//                                             x  g  int stat cols A  parts
constexpr SweepEntry kWsStraightThrough = {{1, 1, 0, 0, 0, 0, 1}, false, false, "vq_gumbel_workspace_bytes"};
constexpr SweepEntry kWsReinmax = {{1, 1, 1, 0, 2, 0, 1}, false, false, "vq_gumbel_reinmax_workspace_bytes"};
constexpr SweepEntry kWsCeCodes = {{1, 0, 1, 1, 0, 0, 1}, false, false, "vq_ce_codes_workspace_bytes"};
constexpr SweepEntry kWsDiversity = {{1, 0, 0, 1, 0, 1, 0}, true, true, "vq_diversity_workspace_bytes"};
constexpr SweepEntry kWsDiversityCodes = {{1, 0, 0, 2, 0, 0, 1}, true, false, "vq_diversity_codes_workspace_bytes"};

struct SweepPlan {
    long long Ch, Cp;            // position-major: rows per position and head, the same padded to whole sub-tiles (else 0)
    long long Mp, img_floats;    // rows of the image (whole staged tiles), floats of one head's image (vq_packed_floats layout)
    int spp, ntiles;             // sub-tiles per position, staged tiles
    int per_split, splits;       // units per blockIdx.z, number of splits
    long long unit[kWsRegions];  // floats of ONE array of the region
    long long off[kWsRegions];   // where the region starts (its second array: off + unit)
    long long floats;
};
static SweepPlan plan_sweep(const SweepEntry &e, int H, long long M, int K, int D, int N) {
    SweepPlan pl{};
    const int DP = padded_dim(D);
    const int tile = kTileCodes * sub_tiles(DP);
    long long rows = M;
    if (e.position_major) {
        pl.Ch = M / N;
        pl.spp = (int)((pl.Ch + kTileCodes - 1) / kTileCodes);
        pl.Cp = (long long)pl.spp * kTileCodes;
        rows = (long long)N * pl.Cp;
    }
    pl.Mp = (rows + tile - 1) / tile * tile;
    pl.img_floats = pl.Mp * (DP + 4) + kPackSlack;
    pl.ntiles = (int)(pl.Mp / tile);
    const UnitSplit u = split_units(H, K, e.split_positions ? N : pl.ntiles);
    pl.per_split = u.per_split;
    pl.splits = u.splits;
    const long long rsM = vq_gumbel_row_stride(M), rsK = vq_gumbel_row_stride(K);
    pl.unit[kWsX] = pl.unit[kWsG] = (long long)H * pl.img_floats;
    pl.unit[kWsInt] = (long long)H * rsM;
    pl.unit[kWsStat] = (long long)H * (e.position_major ? pl.Mp : rsM);
    pl.unit[kWsCols] = (long long)pl.splits * H * rsK;
    pl.unit[kWsA] = (long long)H * N * rsK;
    pl.unit[kWsParts] = pl.splits > 1 ? (long long)pl.splits * H * K * D : 0;
    for (int r = 0; r < kWsRegions; ++r) {
        pl.off[r] = pl.floats;
        pl.floats += e.count[r] * pl.unit[r];
    }
    return pl;
}

// the sizes every diversity entry checks the same way: M must be whole groups of N * pos_div rows
static bool diversity_shape_ok(int H, int64_t M, int K, int D, int N, int pos_div) {
    return H > 0 && M >= 0 && K > 0 && D > 0 && N > 0 && pos_div > 0 && M % ((int64_t)N * pos_div) == 0;
}
// padded rows of the position-major image < 2^31 and the image < 2 GiB (one buffer descriptor)
static bool diversity_image_ok(int64_t M, int D, int N) {
    if (M > 0x7FFFFFFFll) return false;
    const long long rows = ((M / N + 31) / 32 * 32) * N + 256;
    return rows <= 0x7FFFFFFFll && (rows * (padded_dim(D) + 4) + kPackSlack) * 4 < (1ll << 31);
}

// the five sizers: 0 for a shape the entry refuses
static int64_t sweep_workspace_bytes(const SweepEntry &e, int H, int64_t M, int K, int D, int N) {
    const bool ok = e.position_major ? diversity_shape_ok(H, M, K, D, N, 1) && M != 0 && D <= 256 && diversity_image_ok(M, D, N)
                                     : H > 0 && M > 0 && K > 0 && D > 0 && D <= 256 && M <= 0x7FFFFFFFll;
    return ok ? 4 * plan_sweep(e, H, M, K, D, N).floats : 0;
}
int64_t vq_gumbel_workspace_bytes(int H, int64_t M, int K, int D) { return sweep_workspace_bytes(kWsStraightThrough, H, M, K, D, 0); }
int64_t vq_gumbel_reinmax_workspace_bytes(int H, int64_t M, int K, int D) { return sweep_workspace_bytes(kWsReinmax, H, M, K, D, 0); }
int64_t vq_ce_codes_workspace_bytes(int H, int64_t M, int K, int D) { return sweep_workspace_bytes(kWsCeCodes, H, M, K, D, 0); }
int64_t vq_diversity_workspace_bytes(int H, int64_t M, int K, int D, int N) { return sweep_workspace_bytes(kWsDiversity, H, M, K, D, N); }
int64_t vq_diversity_codes_workspace_bytes(int H, int64_t M, int K, int D, int N) {
    return sweep_workspace_bytes(kWsDiversityCodes, H, M, K, D, N);
}

// the fields every role reads the same way
static void init_sweep_params(GumbelParams &p, const vq_args *a, float tau) {
    memset(&p, 0, sizeof(p));
    p.D = a->D;
    p.tau = tau;
    p.st_hs = vq_gumbel_row_stride(a->M);
}

// The argument rules on which the two Gumbel families differ (callers may rely on either; tests/test_gumbel_abi_host.py pins
// both):
//   tau_finite: tau = +inf is rejected
//   null_first: a null statistics array is reported with a null g, before tau and D; otherwise with the alignment, after them
struct GumbelFamily {
    bool tau_finite, null_first;
    const char *null_msg, *tau_msg;
};
constexpr GumbelFamily kStraightThrough = {false, true, "null argument (g / lse2 / delta)", "tau must be positive"};
constexpr GumbelFamily kReinmax = {true, false, "g is null", "tau must be positive and finite"};

// what every Gumbel entry checks and fills; `arrays`: the per-row and per-code arrays the entry uses (non-null, 16-byte aligned)
static int fill_gumbel_params(GumbelParams &p, const char *who, const GumbelFamily &f, const vq_args *a, const float *g, int64_t g_rs,
                              int64_t g_hs, float tau, std::initializer_list<const void *> arrays) {
    bool null_array = false, misaligned = false;
    if (a->M > 0) {  // (M == 0: no launch, the per-row arrays are empty)
        for (const void *q : arrays) {
            null_array |= !q;
            misaligned |= !aligned16(q);
        }
    }
    if (!g || (f.null_first && null_array)) return fail(VQ_E_BADARG, who, f.null_msg);
    if (!(tau > 0.0f) || (f.tau_finite && !(tau < __builtin_inff()))) return fail(VQ_E_BADARG, who, f.tau_msg);
    if (a->D > 256) return fail(VQ_E_UNSUPPORTED, who, "D > 256 (use row chunks of vq_similarities_f32)");
    if (null_array || misaligned) return fail(VQ_E_BADARG, who, "a statistics array is null or not 16-byte aligned");
    init_sweep_params(p, a, tau);
    p.ck_hs = vq_gumbel_row_stride(a->K);  // (read by the kRm* roles only)
    p.g = g; p.g_rs = g_rs; p.g_hs = g_hs;
    p.vec_g = vec4_ok(g, {a->D, g_rs, g_hs}) ? 1 : 0;
    return 0;
}

// what every diversity entry checks before any launch and fills: tau = -T
static int fill_diversity_params(GumbelParams &p, const char *who, const vq_args *a, float T, int N, int pos_div,
                                 std::initializer_list<const void *> arrays) {
    if (!(__builtin_fabsf(T) < __builtin_inff())) return fail(VQ_E_BADARG, who, "T is not finite");
    if (!diversity_shape_ok(a->H, a->M, a->K, a->D, N, pos_div))
        return fail(VQ_E_BADARG, who, "N and pos_div must be positive and M a multiple of N * pos_div");
    for (const void *q : arrays)
        if (!q || !aligned16(q)) return fail(VQ_E_BADARG, who, "an array argument is null or not 16-byte aligned");
    if (a->D > 256) return fail(VQ_E_UNSUPPORTED, who, "D > 256 (use row chunks of vq_similarities_f32)");
    init_sweep_params(p, a, -T);
    p.U_rs = vq_gumbel_row_stride(a->K);
    p.div_N = N;
    p.div_posdiv = pos_div;
    return 0;
}

// rows-resident roles: the rows are resident, the packed codebook is streamed
static int fill_gumbel_rows(GumbelParams &p, const vq_args *a) {
    AuxParams ap;
    if (int rc = fill_aux_params(ap, a)) return rc;
    p.res = a->x; p.res_rs = a->x_rs; p.res_hs = a->x_hs;
    p.vec_res = ap.vec_x;
    p.img = ap.packed; p.img_hs = ap.pk_hs; p.img_bytes = ap.pk_bytes;
    p.NR = a->M; p.NS = a->K;
    p.ntiles = ap.ntiles;
    return 0;
}

// codes-resident roles: the codes are resident, the packed rows are streamed -- the checks, the plan, and every field that
// follows from the plan and the workspace (N: the positions of a position-major image)
static int fill_gumbel_codes(GumbelParams &p, const char *who, const SweepEntry &e, const vq_args *a, int N, void *workspace,
                             int64_t workspace_bytes, SweepPlan &pl) {
    if (!a->cb) return fail(VQ_E_BADARG, who, "cb is null");
    if (e.position_major) {
        if (!diversity_image_ok(a->M, a->D, N)) return fail(VQ_E_UNSUPPORTED, who, "packed row image >= 2 GiB or too many rows (use row chunks)");
    } else if (a->M > 0x7FFFFFFFll) {
        return fail(VQ_E_UNSUPPORTED, who, "too many rows (use row chunks)");
    }
    pl = plan_sweep(e, a->H, a->M, a->K, a->D, N);
    if (pl.img_floats * 4 >= (1ll << 31)) return fail(VQ_E_UNSUPPORTED, who, "packed row image >= 2 GiB (use row chunks)");
    if (!workspace || !aligned16(workspace) || workspace_bytes < 4 * pl.floats) {
        char msg[96];
        snprintf(msg, sizeof(msg), "workspace too small or misaligned (see %s)", e.sizer);
        return fail(VQ_E_BADARG, who, msg);
    }
    float *ws = (float *)workspace;
    p.res = a->cb; p.res_rs = a->D; p.res_hs = a->cb_hs;
    p.vec_res = vec4_ok(a->cb, {a->D, a->cb_hs}) ? 1 : 0;
    p.img = ws + pl.off[kWsX];
    if (e.count[kWsG]) p.gimg = ws + pl.off[kWsG];
    p.img_hs = pl.img_floats; p.img_bytes = (unsigned)(pl.img_floats * 4);
    if (e.count[kWsInt]) p.ind32 = (const int *)(ws + pl.off[kWsInt]);
    p.NR = a->K; p.NS = e.position_major ? (long long)N * pl.Cp : a->M;
    p.ntiles = pl.ntiles;
    (e.split_positions ? p.div_pps : p.tiles_per_split) = pl.per_split;
    if (e.count[kWsStat] > 0) p.lse = ws + pl.off[kWsStat];
    if (e.count[kWsStat] > 1) p.delta = ws + pl.off[kWsStat] + pl.unit[kWsStat];
    if (e.position_major) {  // (the per-row arrays are read in image order)
        p.st_hs = pl.Mp;
        p.div_spp = pl.spp; p.div_ch = (int)pl.Ch;
    }
    return 0;
}

// the only vq_gumbel_pack_rows launch: the x rows (and the g rows, g null: the x image alone) into the images at the head of
// the workspace; `map`: a position-major image and the statistics copied along, or the rows to keep (vq_gumbel.inc)
static int pack_gumbel_rows(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, const SweepPlan &pl, float *ws, hipStream_t s,
                            const vqi::RowMap &map = vqi::RowMap{}) {
    return launch<vq_gumbel_pack_rows>(dim3((unsigned)((pl.Mp + 63) / 64), (unsigned)a->H), dim3(64), 0, s, "vq_gumbel_pack_rows launch", a->x,
                                       (long long)a->x_rs, (long long)a->x_hs, g, (long long)g_rs, (long long)g_hs, (long long)a->M, pl.Mp,
                                       a->D, padded_dim(a->D), a->metric, ws + pl.off[kWsX], g ? ws + pl.off[kWsG] : (float *)nullptr,
                                       pl.img_floats, map);
}

// the position-major image of the diversity loss: lse2 (and delta, or null) of the caller's row order copied along in image order
static vqi::RowMap position_row_map(const SweepPlan &pl, const vq_args *a, int N, int pos_div, const float *lse2, const float *delta,
                                    float *ws) {
    vqi::RowMap map{};
    map.C = pl.Ch; map.Cp = pl.Cp; map.N = N; map.pos_div = pos_div;
    map.stat = lse2; map.stat_hs = vq_gumbel_row_stride(a->M);
    map.stat_img = ws + pl.off[kWsStat]; map.stat_img_hs = pl.Mp;
    if (delta) {
        map.stat2 = delta; map.stat2_img = ws + pl.off[kWsStat] + pl.unit[kWsStat];
    }
    return map;
}

// the only padded-dim dispatch of the fourteen roles, to the build part the role table names (vq_gumbel.inc)
static int launch_gumbel(int role, const GumbelParams &p, const vq_args *a, int gz, hipStream_t s) {
    const int DP = padded_dim(a->D);
    return with_padded_dim(DP == 512 ? 0 : DP,
                           [&](auto dp) {
                               constexpr int DPC = decltype(dp)::value;
                               if constexpr (DPC > 256) return fail(VQ_E_UNSUPPORTED, "vq_gumbel: unsupported padded dim");
                               else switch (sweep_role(role).part) {
                                   case kPartGumbel: return vqi::part_gumbel<DPC>(role, p, a->H, gz, a->metric, s);
                                   case kPartReinmax: return vqi::part_reinmax<DPC>(role, p, a->H, gz, a->metric, s);
                                   case kPartDiversity: return vqi::part_diversity<DPC>(role, p, a->H, gz, a->metric, s);
                                   case kPartOrthogonal: return vqi::part_orthogonal<DPC>(p, a->H, s);
                                   case kPartCeCodes: return vqi::part_ce_codes<DPC>(p, a->H, gz, a->metric, s);
                                   default: return fail(VQ_E_UNSUPPORTED, "vq_gumbel: unknown sweep role");
                               }
                           },
                           [] { return fail(VQ_E_UNSUPPORTED, "vq_gumbel: unsupported padded dim"); });
}

// grad_codes [H][K][D] of the *_backward_codes entries: all zeros for an empty call ...
static int clear_grad_codes(const vq_args *a, float *grad_codes, hipStream_t s, const char *what) {
    const hipError_t e = hipMemsetAsync(grad_codes, 0, (size_t)a->H * a->K * a->D * 4, s);
    return e == hipSuccess ? 0 : hip_fail(e, what);
}

// ... else the sweep (kGumC / kRmC / kDivC / kCeC), straight into grad_codes or into one partial per split that
// vq_gumbel_reduce_parts sums in split order
static int sweep_grad_codes(int role, GumbelParams &p, const vq_args *a, const SweepPlan &pl, float *ws, float *grad_codes, hipStream_t s) {
    const long long n = (long long)a->H * a->K * a->D;
    float *parts = ws + pl.off[kWsParts];
    p.out = pl.splits > 1 ? parts : grad_codes;
    p.out_rs = a->D; p.out_hs = (long long)a->K * a->D; p.out_zs = n;
    if (int rc = launch_gumbel(role, p, a, pl.splits, s)) return rc;
    if (pl.splits == 1) return 0;
    return launch<vq_gumbel_reduce_parts>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, "vq_gumbel_reduce_parts launch", (const float *)parts, n,
                                          pl.splits, grad_codes);
}

// the int32 copy of ind / of the targets the codes-resident roles read 16 bytes at a time (K, stat: see vq_gumbel_pack_ind)
static int pack_gumbel_ind(const GumbelParams &p, const vq_args *a, const int64_t *ind, int64_t ind_rs, int64_t ind_hs, int K,
                           const float *stat, float *stat_out, hipStream_t s) {
    return launch<vq_gumbel_pack_ind>(dim3((unsigned)((p.st_hs + 255) / 256), (unsigned)a->H), dim3(256), 0, s, "vq_gumbel_pack_ind launch",
                                      (const long long *)ind, (long long)ind_rs, (long long)ind_hs, (long long)a->M, p.st_hs, (int *)p.ind32, K,
                                      stat, (long long)a->M, stat_out);
}

// ---- Gumbel backward through the similarities: the straight-through (kGum*) and reinmax (kRm*) roles ------------------------
int vq_gumbel_stats_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, float *lse2, float *delta,
                        void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    GumbelParams p;
    if ((rc = fill_gumbel_params(p, "vq_gumbel_stats", kStraightThrough, a, g, g_rs, g_hs, tau, {lse2, delta}))) return rc;
    if ((rc = fill_gumbel_rows(p, a))) return rc;
    p.lse = lse2; p.delta = delta;
    return launch_gumbel(kGumStats, p, a, 1, (hipStream_t)stream);
}

int vq_gumbel_backward_x_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2,
                             const float *delta, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (a->M == 0) return 0;
    if (!grad_x) return fail(VQ_E_BADARG, "vq_gumbel_backward_x: grad_x is null");
    GumbelParams p;
    if ((rc = fill_gumbel_params(p, "vq_gumbel_backward_x", kStraightThrough, a, g, g_rs, g_hs, tau, {lse2, delta}))) return rc;
    if ((rc = fill_gumbel_rows(p, a))) return rc;
    p.lse = (float *)lse2; p.delta = (float *)delta;
    p.out = grad_x; p.out_rs = gx_rs; p.out_hs = gx_hs;
    return launch_gumbel(kGumX, p, a, 1, (hipStream_t)stream);
}

int vq_gumbel_backward_codes_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2,
                                 const float *delta, float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream) {
    static const char who[] = "vq_gumbel_backward_codes";
    int rc = check_common(a);
    if (rc) return rc;
    if (!grad_codes || !a->cb) return fail(VQ_E_BADARG, who, "null argument (grad_codes / cb)");
    hipStream_t s = (hipStream_t)stream;
    if (a->M == 0) return clear_grad_codes(a, grad_codes, s, "vq_gumbel_backward_codes memset");
    GumbelParams p;
    SweepPlan pl;
    if ((rc = fill_gumbel_params(p, who, kStraightThrough, a, g, g_rs, g_hs, tau, {lse2, delta}))) return rc;
    if ((rc = fill_gumbel_codes(p, who, kWsStraightThrough, a, 0, workspace, workspace_bytes, pl))) return rc;
    if ((rc = pack_gumbel_rows(a, g, g_rs, g_hs, pl, (float *)workspace, s))) return rc;
    p.lse = (float *)lse2; p.delta = (float *)delta;
    return sweep_grad_codes(kGumC, p, a, pl, (float *)workspace, grad_codes, s);
}

int vq_gumbel_reinmax_stats_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, float *lse2_tau,
                                float *lse2_one, float *delta0, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    if ((rc = fill_gumbel_params(p, "vq_gumbel_reinmax_stats", kReinmax, a, g, g_rs, g_hs, tau, {lse2_tau, lse2_one, delta0}))) return rc;
    if (a->M == 0) return 0;
    if ((rc = fill_gumbel_rows(p, a))) return rc;
    p.lse = lse2_tau; p.lse1 = lse2_one; p.delta = delta0;
    return launch_gumbel(kRmStats, p, a, 1, (hipStream_t)stream);
}

int vq_gumbel_reinmax_columns_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2_tau,
                                  const int64_t *ind, int64_t ind_rs, int64_t ind_hs, float *col, float *e, void *workspace,
                                  int64_t workspace_bytes, void *stream) {
    static const char who[] = "vq_gumbel_reinmax_columns";
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    SweepPlan pl;
    if ((rc = fill_gumbel_params(p, who, kReinmax, a, g, g_rs, g_hs, tau, {lse2_tau, col, e}))) return rc;
    if (!ind) return fail(VQ_E_BADARG, who, "ind is null");
    if (a->M == 0) return 0;
    if ((rc = fill_gumbel_codes(p, who, kWsReinmax, a, 0, workspace, workspace_bytes, pl))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *ws = (float *)workspace;
    if ((rc = pack_gumbel_rows(a, g, g_rs, g_hs, pl, ws, s))) return rc;
    if ((rc = pack_gumbel_ind(p, a, ind, ind_rs, ind_hs, 0, nullptr, nullptr, s))) return rc;
    p.lse = (float *)lse2_tau;
    p.colp = ws + pl.off[kWsCols]; p.ep = p.colp + pl.unit[kWsCols];
    p.cp_zs = (long long)a->H * p.ck_hs;
    if ((rc = launch_gumbel(kRmCol, p, a, pl.splits, s))) return rc;
    return launch<vq_gumbel_reduce_cols>(dim3((unsigned)((p.cp_zs + 255) / 256)), dim3(256), 0, s, "vq_gumbel_reduce_cols launch",
                                         (const float *)p.colp, (const float *)p.ep, p.cp_zs, p.ck_hs, a->K, pl.splits, col, e);
}

int vq_gumbel_reinmax_backward_x_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2_tau,
                                     const float *lse2_one, const float *delta0, const int64_t *ind, int64_t ind_rs, int64_t ind_hs,
                                     const float *col, const float *e, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream) {
    static const char who[] = "vq_gumbel_reinmax_backward_x";
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    if ((rc = fill_gumbel_params(p, who, kReinmax, a, g, g_rs, g_hs, tau, {lse2_tau, lse2_one, delta0, col, e}))) return rc;
    if (!ind || !grad_x) return fail(VQ_E_BADARG, who, "null argument (ind / grad_x)");
    if (a->M == 0) return 0;
    if ((rc = fill_gumbel_rows(p, a))) return rc;
    p.lse = (float *)lse2_tau; p.lse1 = (float *)lse2_one; p.delta = (float *)delta0;
    p.ind = (const long long *)ind; p.ind_rs = ind_rs; p.ind_hs = ind_hs;
    p.col = (float *)col; p.e = (float *)e;
    p.out = grad_x; p.out_rs = gx_rs; p.out_hs = gx_hs;
    return launch_gumbel(kRmX, p, a, 1, (hipStream_t)stream);
}

int vq_gumbel_reinmax_backward_codes_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2_tau,
                                         const float *lse2_one, const float *delta0, const float *col, const float *e,
                                         float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream) {
    static const char who[] = "vq_gumbel_reinmax_backward_codes";
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    SweepPlan pl;
    if ((rc = fill_gumbel_params(p, who, kReinmax, a, g, g_rs, g_hs, tau, {lse2_tau, lse2_one, delta0, col, e}))) return rc;
    if (!grad_codes) return fail(VQ_E_BADARG, who, "grad_codes is null");
    hipStream_t s = (hipStream_t)stream;
    if (a->M == 0) return clear_grad_codes(a, grad_codes, s, "vq_gumbel_reinmax_backward_codes memset");
    if ((rc = fill_gumbel_codes(p, who, kWsReinmax, a, 0, workspace, workspace_bytes, pl))) return rc;
    p.lse = (float *)lse2_tau; p.lse1 = (float *)lse2_one; p.delta = (float *)delta0;
    p.col = (float *)col; p.e = (float *)e;
    return sweep_grad_codes(kRmC, p, a, pl, (float *)workspace, grad_codes, s);
}

// ---- codebook diversity loss: the kDiv* roles, vq_diversity.inc ----------------------------------------------------------
int vq_diversity_stats_f32(const vq_args *a, float T, float *lse2, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    if ((rc = fill_diversity_params(p, "vq_diversity_stats", a, T, 1, 1, {lse2}))) return rc;
    if (a->M == 0) return 0;
    if ((rc = fill_gumbel_rows(p, a))) return rc;
    p.lse = lse2;
    return launch_gumbel(kDivStats, p, a, 1, (hipStream_t)stream);
}

int vq_diversity_accumulate_f32(const vq_args *a, float T, int N, int pos_div, const float *lse2, float *A, void *workspace,
                                int64_t workspace_bytes, void *stream) {
    static const char who[] = "vq_diversity_accumulate";
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    SweepPlan pl;
    if ((rc = fill_diversity_params(p, who, a, T, N, pos_div, {lse2, A}))) return rc;
    if (!a->cb) return fail(VQ_E_BADARG, who, "cb is null");
    if (a->M == 0) return 0;
    if ((rc = fill_gumbel_codes(p, who, kWsDiversity, a, N, workspace, workspace_bytes, pl))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *ws = (float *)workspace;
    if ((rc = pack_gumbel_rows(a, nullptr, 0, 0, pl, ws, s, position_row_map(pl, a, N, pos_div, lse2, nullptr, ws)))) return rc;
    const long long rsK = p.U_rs, n = (long long)N * rsK;
    p.out = ws + pl.off[kWsA]; p.out_rs = rsK; p.out_hs = n;
    if ((rc = launch_gumbel(kDivAcc, p, a, pl.splits, s))) return rc;
    return launch<vq_diversity_reduce_heads>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, "vq_diversity_reduce_heads launch",
                                             (const float *)p.out, n, rsK, a->K, a->H, (float)((double)a->H * (double)pl.Ch), A);
}

int vq_diversity_delta_f32(const vq_args *a, float T, int N, int pos_div, const float *lse2, const float *U, float *delta,
                           void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    if ((rc = fill_diversity_params(p, "vq_diversity_delta", a, T, N, pos_div, {lse2, U, delta}))) return rc;
    if (a->M == 0) return 0;
    if ((rc = fill_gumbel_rows(p, a))) return rc;
    p.lse = (float *)lse2; p.delta = delta; p.U = U;
    return launch_gumbel(kDivDelta, p, a, 1, (hipStream_t)stream);
}

int vq_diversity_backward_x_f32(const vq_args *a, const float *live_packed, int64_t live_pk_hs, float T, int N, int pos_div,
                                const float *lse2, const float *delta, const float *U, float *grad_x, int64_t gx_rs, int64_t gx_hs,
                                void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    if ((rc = fill_diversity_params(p, "vq_diversity_backward_x", a, T, N, pos_div, {lse2, delta, U}))) return rc;
    if (!grad_x) return fail(VQ_E_BADARG, "vq_diversity_backward_x: grad_x is null");
    if (a->M == 0) return 0;
    if ((rc = fill_gumbel_rows(p, a))) return rc;
    p.lse = (float *)lse2; p.delta = (float *)delta; p.U = U;
    p.gimg = live_packed; p.gimg_hs = live_pk_hs;
    p.out = grad_x; p.out_rs = gx_rs; p.out_hs = gx_hs;
    return launch_gumbel(kDivX, p, a, 1, (hipStream_t)stream);
}

int vq_diversity_backward_codes_f32(const vq_args *a, float T, int N, int pos_div, const float *lse2, const float *delta,
                                    const float *U, float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream) {
    static const char who[] = "vq_diversity_backward_codes";
    int rc = check_common(a);
    if (rc) return rc;
    GumbelParams p;
    SweepPlan pl;
    if ((rc = fill_diversity_params(p, who, a, T, N, pos_div, {lse2, delta, U}))) return rc;
    if (!grad_codes || !a->cb) return fail(VQ_E_BADARG, who, "null argument (grad_codes / cb)");
    hipStream_t s = (hipStream_t)stream;
    if (a->M == 0) return clear_grad_codes(a, grad_codes, s, "vq_diversity_backward_codes memset");
    if ((rc = fill_gumbel_codes(p, who, kWsDiversityCodes, a, N, workspace, workspace_bytes, pl))) return rc;
    float *ws = (float *)workspace;
    // the image is packed again here: keeping the forward's alive until backward would double the activation memory of the rows
    if ((rc = pack_gumbel_rows(a, nullptr, 0, 0, pl, ws, s, position_row_map(pl, a, N, pos_div, lse2, delta, ws)))) return rc;
    p.U = U;
    return sweep_grad_codes(kDivC, p, a, pl, ws, grad_codes, s);
}

// ---- cross-entropy loss, the gradient with respect to a learnable codebook: the kCeC role ----------------------------------
int vq_ce_backward_codes_f32(const vq_args *a, const float *lse, const int64_t *target, int64_t tgt_rs, int64_t tgt_hs,
                             const float *coef, float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream) {
    static const char who[] = "vq_ce_backward_codes";
    int rc = check_common(a);
    if (rc) return rc;
    if (!grad_codes || !a->cb || !coef) return fail(VQ_E_BADARG, who, "null argument (grad_codes / cb / coef)");
    if (a->D > 256) return fail(VQ_E_UNSUPPORTED, who, "D > 256 (use row chunks of vq_similarities_f32)");
    hipStream_t s = (hipStream_t)stream;
    if (a->M == 0) return clear_grad_codes(a, grad_codes, s, "vq_ce_backward_codes memset");
    if (!lse || !target) return fail(VQ_E_BADARG, who, "null argument (lse / target)");
    GumbelParams p;
    SweepPlan pl;
    init_sweep_params(p, a, 0.0f);
    if ((rc = fill_gumbel_codes(p, who, kWsCeCodes, a, 0, workspace, workspace_bytes, pl))) return rc;
    float *ws = (float *)workspace;
    // the targets (-1: ignored, compared as 64-bit values) and the log-sum-exp at the sweep's 16-byte aligned head stride ...
    if ((rc = pack_gumbel_ind(p, a, target, tgt_rs, tgt_hs, a->K, lse, p.lse, s))) return rc;
    // ... then the x image, an ignored row as padding
    vqi::RowMap map{};
    map.keep = p.ind32; map.keep_hs = p.st_hs;
    if ((rc = pack_gumbel_rows(a, nullptr, 0, 0, pl, ws, s, map))) return rc;
    p.coef = coef;
    return sweep_grad_codes(kCeC, p, a, pl, ws, grad_codes, s);
}

// ---- orthogonal regularisation loss: the kOrth role -------------------------------------------------------------------------
// n = a->K rows on both sides: resident from a->x, streamed from a->packed (the dot image of the same rows)
int vq_orthogonal_gram_f32(const vq_args *a, float *rowsq, float *gram, int64_t g_rs, int64_t g_hs, void *stream) {
    static const char who[] = "vq_orthogonal_gram";
    if (!a) return fail(VQ_E_BADARG, who, "args is null");
    if (a->H <= 0 || a->K <= 0 || a->D <= 0) return fail(VQ_E_BADARG, who, "H, K (the number of rows n) and D must be positive");
    if (a->metric != VQ_METRIC_DOT) return fail(VQ_E_BADARG, who, "metric must be VQ_METRIC_DOT");
    if (!a->x) return fail(VQ_E_BADARG, who, "x is null");
    if (!a->packed) return fail(VQ_E_BADARG, who, "packed is null (the dot image of the rows)");
    if (!rowsq || !aligned16(rowsq)) return fail(VQ_E_BADARG, who, "rowsq is null or not 16-byte aligned");
    if (gram && !aligned16(gram)) return fail(VQ_E_BADARG, who, "gram is not 16-byte aligned");
    if (a->D > 256) return fail(VQ_E_UNSUPPORTED, who, "D > 256");
    if (vq_packed_floats(a->K, a->D) * 4 >= (1ll << 31)) return fail(VQ_E_UNSUPPORTED, who, "packed image >= 2 GiB");
    GumbelParams p;
    init_sweep_params(p, a, 0.0f);
    p.res = a->x; p.res_rs = a->x_rs; p.res_hs = a->x_hs;
    p.vec_res = vec4_ok(a->x, {a->D, a->x_rs, a->x_hs}) ? 1 : 0;
    p.img = a->packed; p.img_hs = a->pk_hs; p.img_bytes = (unsigned)(vq_packed_floats(a->K, a->D) * 4);
    p.NR = a->K; p.NS = a->K;
    const int tc = kTileCodes * sub_tiles(padded_dim(a->D));
    p.ntiles = (a->K + tc - 1) / tc;
    p.lse = rowsq; p.st_hs = vq_gumbel_row_stride(a->K);  // (the rows are the codes: a->M is not read)
    p.out = gram; p.out_rs = g_rs; p.out_hs = g_hs;
    return launch_gumbel(kOrth, p, a, 1, (hipStream_t)stream);
}
