// vq_search_host.inc -- host side of the nearest-code search: the executor of vq_search_plan.h's plans and the search's C ABI
// (vq_quantize_f32, vq_quantize_lse_f32, the keys-mode entries, the finalize entries).  Included by vq_kernels.hip in build
// part 0, at file scope.  The division of labour: vq_search_plan.h decides (pure arithmetic on values), this file reads what the
// decision depends on -- the device (dev_info), the environment (read_switches), the call (describe_call) -- exactly once per
// call, fills kernel parameters and launches.  Nothing below decides a launch shape on its own, and nothing below the three
// readers looks at the device or the environment.

namespace {

// ---- the readers -----------------------------------------------------------------------------------------------------------
struct DevInfo {
    int cus = 0;
    int clock_mhz = 2400;  // shader clock (hipDeviceProp_t::clockRate), what the launch plans price a sub-tile with
    bool ok = false;
    char name[128] = "";
};

const DevInfo &dev_info() {
    static thread_local DevInfo info;
    static thread_local int cached_dev = -1;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        info.ok = false;
        return info;
    }
    if (dev != cached_dev) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            info.cus = prop.multiProcessorCount;
            if (prop.clockRate > 0) info.clock_mhz = prop.clockRate / 1000;
            snprintf(info.name, sizeof(info.name), "%s", prop.gcnArchName);
            info.ok = true;
            cached_dev = dev;
        } else {
            info.ok = false;
        }
    }
    return info;
}

// the current device as the plans see it; 256 CUs at 2400 MHz when the device cannot be asked
Device plan_device() {
    const DevInfo &di = dev_info();
    return {di.ok && di.cus > 0 ? di.cus : 256, di.ok && di.clock_mhz > 0 ? di.clock_mhz : 2400};
}
inline int device_cus() { return plan_device().cus; }

// The environment switches of the search (A/B measurements and tests).  The first four are read once per process; the others
// per call: tests flip them inside one process.
Switches read_switches() {
    static const bool single_wave_512 = getenv("VQ_SINGLE_WAVE_512") != nullptr, no_persist = getenv("VQ_NO_PERSIST") != nullptr,
                      no_resident = getenv("VQ_NO_RESIDENT") != nullptr;
    static const char *res_skew = getenv("VQ_RES_SKEW");
    Switches sw;
    sw.single_wave_512 = single_wave_512;
    sw.no_persist = no_persist;
    sw.no_resident = no_resident;
    sw.res_skew = res_skew ? atoi(res_skew) : 0;
    sw.no_persist_train = getenv("VQ_NO_PERSIST_TRAIN") != nullptr;
    sw.no_screen = getenv("VQ_NO_SCREEN") != nullptr;
    sw.pair_no_multi = getenv("VQ_PAIR_NO_MULTI") != nullptr;
    sw.no_residual_tail = getenv("VQ_NO_RESIDUAL_TAIL") != nullptr;
    sw.no_stagger = getenv("VQ_NO_STAGGER") != nullptr;
    sw.resolve_no_split = getenv("VQ_RESOLVE_NO_SPLIT") != nullptr;
    return sw;
}

// what the plans need of a call: its sizes and flags, which buffers exist, and which of them take float4 accesses
Call describe_call(const vq_args *a, bool lse) {
    Call c = {};
    c.H = a->H; c.M = a->M; c.K = a->K; c.D = a->D; c.Q = a->Q; c.metric = a->metric;
    c.flags = a->flags;
    c.workspace_bytes = a->workspace_bytes;
    c.out = a->out != nullptr; c.idx = a->idx != nullptr; c.best = a->best != nullptr; c.sq_err = a->sq_err != nullptr;
    c.lse = lse; c.cb = a->cb != nullptr; c.packed = a->packed != nullptr; c.screen = a->screen != nullptr;
    const bool out4 = vec4_ok(a->out, {a->out_rs, a->out_hs});
    c.vec_x = vec4_ok(a->x, {a->D, a->x_rs, a->x_hs}, (a->flags & (VQ_F_X_F16 | VQ_F_X_BF16)) ? 8 : 16);  // (2-byte rows: four of them are 8 bytes)
    c.vec_fin = c.vec_x && (!a->out || out4) && (!a->cb || vec4_ok(a->cb, {a->cb_hs, a->cb_qs}));
    // (the resident kernel's deferred copy adds a 32-bit byte offset of up to 31 rows of out to a block's base: 32 rows of out
    //  must span less than 2^32 bytes; a wider, or a negative, row stride takes the tile-streaming kernels)
    const bool out_rs32 = a->out_rs >= 0 && a->out_rs * 128 < (1ll << 32);
    c.vec_res = vec4_ok(a->x, {a->x_rs, a->x_hs}) && out4 && out_rs32 && vec4_ok(a->cb, {a->cb_hs});
    c.vec_wide = vec4_ok(a->out, {a->D, a->out_rs, a->out_hs}) && vec4_ok(a->cb, {a->cb_hs});
    return c;
}

// the rows [m1, m1 + rows) of a call
vq_args rows_from(const vq_args &a, long long m1, long long rows) {
    vq_args t = a;
    t.M = rows;
    t.x = a.x + m1 * a.x_rs;
    if (a.out) t.out = a.out + m1 * a.out_rs;
    if (a.idx) t.idx = a.idx + m1 * a.idx_rs;
    if (a.best) t.best = a.best + m1 * a.idx_rs;
    return t;
}

// ---- parameters and launches -------------------------------------------------------------------------------------------------
// The screened sweep's fp16 images are built per call into the key area of the workspace, which a fused call does not use,
// and behind them the control block and the two lists of rows for the second pass (vq_resolve_rows_kernel): the layout of
// screen_bytes.  With the caller's image (c.cached: vq_args.screen, checked by check_screen) only the lists are in the workspace.
void set_screen_image(SearchParams &p, const vq_args *a, const SearchChoice &c) {
    const long long img = scr_image_bytes(p.ntiles);
    char *base = (char *)(c.cached ? a->screen : a->workspace);
    p.scr = (const float *)base;
    p.scr_hs = img;
    p.scr_bytes = (unsigned)img;
    p.scr_count = (unsigned *)(base + (long long)a->H * img);
    p.scr_list = c.cached ? (unsigned *)a->workspace : p.scr_count + kScrCtrlBytes / 4;
    p.scr_stagger = c.stagger;
}

// launches the kernel that choose_search picked for (DP, p, H, splits)
int launch_search(const SearchChoice &c, int DP, const SearchParams &p, int H, int splits, int metric, int cus, hipStream_t s) {
    switch (c.kind) {
        case kResident:  // (resident images exist for Dp <= 128 only)
            if (DP == 32) return vqi::part_resident<32>(p, H, cus, metric, s);
            if (DP == 64) return vqi::part_resident<64>(p, H, cus, metric, s);
            if (DP == 128) return vqi::part_resident<128>(p, H, cus, metric, s);
            break;
        case kPersist: return vqi::part_persist(c, p, H, cus, metric, s);
        case kPair: return vqi::part_pair(p, H, splits, metric, s);
        case kOneBlock:
            return with_padded_dim(DP, [&](auto dp) { return vqi::part_search<decltype(dp)::value>(c.waves, p, H, splits, metric, s); },
                                   [] { return fail(VQ_E_UNSUPPORTED, "vq_search: unsupported padded dim"); });
    }
    return fail(VQ_E_UNSUPPORTED, "vq_search: unsupported padded dim");
}

// one slice of a wide-row sweep, by the padded width of the slice; `pairs`: on the wave-pair kernel (512-dim slices)
int launch_wide(int wide, bool pairs, int DP, const SearchParams &p, int H, int splits, int metric, hipStream_t s) {
    return with_padded_dim(DP, [&](auto dp) { return vqi::part_wide<decltype(dp)::value>(wide, pairs, p, H, splits, metric, s); },
                           [] { return fail(VQ_E_UNSUPPORTED, "vq_search: unsupported padded dim"); });
}

// a caller-cached screen image must be THE image of this call's codebooks' shape: anything else is an argument error
int check_screen(const vq_args *a) {
    if (!a->screen && a->screen_bytes == 0) return 0;
    if (!a->screen || a->screen_bytes <= 0 || a->screen_bytes != vq_screen_image_bytes(a->H, a->K, a->D, a->metric))
        return fail(VQ_E_BADARG, "vq_quantize: screen / screen_bytes do not match vq_screen_image_bytes(H, K, D, metric)");
    if (!aligned16(a->screen)) return fail(VQ_E_BADARG, "vq_quantize: screen is not 16-byte aligned");
    return 0;
}

// the loss partials of a call of M rows lie behind its keys
inline float *ws_loss_part(const vq_args *a) { return (float *)((char *)a->workspace + ws_keys_bytes(a->H, a->M)); }

void fill_search_params(SearchParams &p, const vq_args *a) {
    memset(&p, 0, sizeof(p));
    p.x = a->x; p.x_rs = a->x_rs; p.x_hs = a->x_hs;
    p.cb = a->cb; p.cb_hs = a->cb_hs; p.cb_qs = a->cb_qs;
    p.packed = a->packed; p.pk_hs = a->pk_hs; p.pk_qs = a->pk_qs;
    p.out = a->out; p.out_rs = a->out_rs; p.out_hs = a->out_hs;
    p.idx = (long long *)a->idx; p.idx_rs = a->idx_rs; p.idx_hs = a->idx_hs; p.idx_qs = a->idx_qs;
    p.best = a->best;
    p.M = a->M; p.K = a->K; p.D = a->D; p.Q = a->Q;
    p.ntiles = tiles_of(a->K, padded_dim(a->D) ? padded_dim(a->D) : 256);
    p.tiles_per_split = p.ntiles;
    p.key_hs = a->M;
    p.pk_bytes = (unsigned)(vq_packed_floats(a->K, a->D) * 4);

    p.ste = (a->flags & VQ_F_STE) ? 1 : 0;
    p.xt = (a->flags & VQ_F_X_F16) ? 1 : ((a->flags & VQ_F_X_BF16) ? 2 : 0);
    p.vec_x = vec4_ok(a->x, {a->D, a->x_rs, a->x_hs}, p.xt ? 8 : 16) ? 1 : 0;  // (2-byte rows: four of them are 8 bytes)
    p.vec_fin = (p.vec_x && (!a->out || vec4_ok(a->out, {a->out_rs, a->out_hs})) && (!a->cb || vec4_ok(a->cb, {a->cb_hs, a->cb_qs}))) ? 1 : 0;
}

// one stage of a residual stack run stage by stage (run_staged_leg): where the next residual goes, whether `out` accumulates
struct ResidualStage {
    float *res_next;
    int out_acc;
};

int run_finalize(const vq_args *a, const long long *keys, float *loss_part, hipStream_t s, int *nparts_out, int key_planes = 1,
                 const ResidualStage *rst = nullptr) {
    FinalizeParams f;
    memset(&f, 0, sizeof(f));
    if (rst) {
        f.residual = 1;
        f.res_next = rst->res_next;
        f.out_acc = rst->out_acc;
    }
    f.keys = keys;
    f.nparts = key_planes;
    f.part_stride = (long long)a->H * a->M;
    f.x = a->x; f.x_rs = a->x_rs; f.x_hs = a->x_hs;
    f.cb = a->cb; f.cb_hs = a->cb_hs;
    f.out = a->out; f.out_rs = a->out_rs; f.out_hs = a->out_hs;
    f.idx = (long long *)a->idx; f.idx_rs = a->idx_rs; f.idx_hs = a->idx_hs;
    f.best = a->best;
    f.loss_part = loss_part;
    f.M = a->M; f.D = a->D; f.metric = a->metric; f.ste = (a->flags & VQ_F_STE) ? 1 : 0;
    f.vec = (vec4_ok(a->cb, {a->D, a->cb_hs}) && (!a->out || vec4_ok(a->out, {a->out_rs, a->out_hs})) &&
             (!(f.ste || loss_part || f.res_next) || vec4_ok(a->x, {a->x_rs, a->x_hs})) &&  // (x is read for these only)
             (!f.res_next || aligned16(f.res_next))) ? 1 : 0;
    long long blocks = (a->M + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks, (unsigned)a->H);
    const int rc = rst ? launch<vq_finalize_kernel<true>>(grid, dim3(256), 0, s, "vq_finalize launch", f)
                       : launch<vq_finalize_kernel<false>>(grid, dim3(256), 0, s, "vq_finalize launch", f);
    if (rc) return rc;
    if (nparts_out) *nparts_out = (int)(blocks * 4 * a->H);
    return 0;
}

// sums the loss partials of a launch: grid = (stages, heads or 1); `sq_err_hs` > 0: the heads' sums that many doubles apart
int reduce_loss(dim3 grid, hipStream_t s, const float *part, long long nparts, int Q, double *sq_err, int acc, int sq_err_hs = -1) {
    return launch<vq_loss_reduce_kernel>(grid, dim3(256), 0, s, "vq_loss_reduce launch", part, nparts, Q, sq_err, acc, sq_err_hs);
}

// squared-error sums of a call: one per stage, per head with VQ_F_SQERR_PER_HEAD
inline size_t sq_err_count(const vq_args *a) { return (size_t)a->Q * ((a->flags & VQ_F_SQERR_PER_HEAD) ? a->H : 1); }
int clear_sq_err(double *sq_err, size_t n, hipStream_t s, const char *what) {
    const hipError_t e = hipMemsetAsync(sq_err, 0, sizeof(double) * n, s);
    return e == hipSuccess ? 0 : hip_fail(e, what);
}

// ---- rows wider than 512 dims (the plan: wide_plan in vq_search_plan.h) --------------------------------------------------------
// `keys` (search: argmin into packed keys), `sims` (the similarity matrix itself) or `fused` (the whole inference call)
int run_wide(const vq_args *a, const WidePlan &w, long long idx_offset, long long *keys, float *sims, long long sims_rs, long long sims_hs,
             const Device &dev, const Switches &sw, hipStream_t s, bool fused = false) {
    if (!a->packed) return fail(VQ_E_BADARG, "vq: packed codebook is null");
    if (a->flags & (VQ_F_X_F16 | VQ_F_X_BF16)) return fail(VQ_E_UNSUPPORTED, "vq: 2-byte rows need D <= 512");
    const long long img = wide_image_floats(a->K);
    if (img * 4 >= (1ll << 31)) return fail(VQ_E_UNSUPPORTED, "vq: packed codebook image >= 2 GiB (shard the codebook)");
    if (!a->workspace || a->workspace_bytes < wide_workspace_bytes(a->H, a->M, w))
        return fail(VQ_E_BADARG, "vq: workspace too small for rows wider than 512 dims (see vq_workspace_bytes_wide)");
    const long long base = workspace_bytes(a->H, a->M, 1);
    float *acc_ws = (float *)((char *)a->workspace + base);
    float *xn_ws = (float *)((char *)a->workspace + base + w.acc_bytes);
    const int Kp = round_up(a->K, kTileCodes);
    const int d_last = wide_last_dims(a->D), dp_last = padded_dim(d_last);
    for (long long m0 = 0; m0 < a->M; m0 += w.mc) {
        const long long mrows = (a->M - m0 < w.mc) ? a->M - m0 : w.mc;
        const long long nblk = (mrows + kWideRows - 1) / kWideRows;
        const vq_args c = rows_from(*a, m0, mrows);
        for (int k0 = 0; k0 < Kp; k0 += w.kc) {
            const int kcodes = (a->K - k0 < w.kc) ? a->K - k0 : w.kc;  // real codes of this chunk (> 0: k0 < Kp, K > Kp - 32)
            const int nsub = sub_tiles_of(kcodes);
            for (int j = 0; j < w.nd; ++j) {
                const bool last = j + 1 == w.nd;
                const int DP = last ? dp_last : kWideSlice;
                const int rs = DP + 4;                                        // packed row stride of this slice's image
                const long long img_j = last ? wide_last_image_floats(a->K, a->D) : img;
                SearchParams p;
                memset(&p, 0, sizeof(p));
                p.x = c.x + (long long)j * kWideSlice;
                p.x_rs = a->x_rs; p.x_hs = a->x_hs;
                p.packed = a->packed + (long long)j * img + (long long)k0 * rs;
                p.pk_hs = a->pk_hs;
                p.pk_bytes = (unsigned)((img_j - (long long)k0 * rs) * 4);
                p.M = mrows; p.K = kcodes; p.D = last ? d_last : kWideSlice; p.Q = 1;
                p.ntiles = tiles_of(kcodes, DP);
                const TileSplit ts = wide_slice_splits(DP, a->H, nblk, mrows, kcodes, p.ntiles, fused, dev);
                p.tiles_per_split = ts.tiles_per_split;
                p.mode = fused ? kModeFused : kModeKeys;
                if (fused) {
                    p.cb = a->cb; p.cb_hs = a->cb_hs;
                    p.out = c.out; p.out_rs = a->out_rs; p.out_hs = a->out_hs;
                    p.idx = (long long *)c.idx; p.idx_rs = a->idx_rs; p.idx_hs = a->idx_hs;
                    p.best = c.best;
                    p.fin_D = a->D;
                }
                p.keys = keys ? keys + m0 : nullptr;
                p.key_hs = a->M;
                p.idx_offset = idx_offset + k0;
                p.vec_x = vec4_ok(a->x, {p.D, a->x_rs, a->x_hs}) ? 1 : 0;
                p.acc_ws = acc_ws;
                p.ws_hs = nblk * kWideWaves * (long long)nsub * 256;
                p.ws_nsub = nsub;
                p.acc_in = j > 0;
                p.xn_ws = xn_ws + ((j + 1) & 1) * (w.xn_bytes / 8);
                p.xn_out = xn_ws + (j & 1) * (w.xn_bytes / 8);
                p.xn_hs = w.mc;
                if (sims) {
                    p.sims = sims + m0 * sims_rs + k0;
                    p.sims_rs = sims_rs; p.sims_hs = sims_hs;
                    p.vec_s = vec4_ok(sims, {a->K, sims_rs, sims_hs}) ? 1 : 0;
                }
                const int rc = launch_wide(!last ? 1 : (sims ? 3 : 2), pairs_worth_it(DP, p.tiles_per_split, 1, sw), DP, p, a->H, ts.splits,
                                           a->metric, s);
                if (rc) return rc;
            }
        }
    }
    return 0;
}

// ---- keys-mode searches ------------------------------------------------------------------------------------------------------
inline KeysPlan plan_keys_of(const vq_args *a, int planned_splits, const Device &dev, const Switches &sw) {
    return plan_keys(a->H, a->M, a->K, a->D, a->flags, planned_splits, dev, sw);
}

// The search of `kp` into packed keys.  `part_stride` > 0: K split z stores its keys into plane z (planes part_stride keys
// apart, kp.splits of them, nothing to initialise); 0: all splits combine into ONE plane with atomic MIN (the caller initialised it).
int run_search_keys(const vq_args *a, const KeysPlan &kp, long long idx_offset, long long *keys, long long part_stride, const Device &dev,
                    const Switches &sw, hipStream_t s) {
    if (!kp.mfma && part_stride > 0) return fail(VQ_E_UNSUPPORTED, "vq: key planes need the MFMA kernel (D <= 512)");
    if (kp.wide_rows) return run_wide(a, kp.wide, idx_offset, keys, nullptr, 0, 0, dev, sw, s);
    if (!kp.mfma) {
        if (!a->cb) return fail(VQ_E_BADARG, "vq: natural codebook required for the scalar kernel");
        return with_metric(a->metric, [&](auto m) {
            return launch<vq_search_simple<decltype(m)::value>>(dim3((unsigned)((a->M + 63) / 64), (unsigned)a->H), dim3(64), 0, s, "vq_search_simple launch",
                                                                a->x, a->x_rs, a->x_hs, a->cb, a->cb_hs, a->M, a->K, a->D, idx_offset, keys);
        });
    }
    if (!a->packed) return fail(VQ_E_BADARG, "vq: packed codebook is null");
    if (vq_packed_floats(a->K, a->D) * 4 >= (1ll << 31))
        return fail(VQ_E_UNSUPPORTED, "vq: packed codebook image >= 2 GiB (shard the codebook)");
    SearchParams p;
    fill_search_params(p, a);
    p.mode = part_stride > 0 ? kModeKeyParts : kModeKeys;
    p.key_zs = part_stride;
    p.keys = keys;
    p.idx_offset = idx_offset;
    p.Q = 1;
    p.out = nullptr;
    p.loss_part = nullptr;
    p.tiles_per_split = kp.tiles_per_split;
    return launch_search(kp.choice, kp.DP, p, a->H, kp.splits, a->metric, dev.cus, s);
}

// ---- the legs of a plan ------------------------------------------------------------------------------------------------------
// (every leg is handed ITS rows as a call of their own: rows_from; its workspace sections are those of its row count)

// kLegKeys / kLegWideKeys / kLegScalar: search into key planes (K split over workgroups: every split stores its winners into a
// plane of its own, no init launch, no atomics; one plane + atomic MIN if the planes do not fit the workspace, or without the
// MFMA kernel)  +  finalize (MIN over the planes, gather, straight-through, squared error).  `rst`: the stage belongs to a
// residual stack run stage by stage.  `sq_err_hs` > 0: one squared-error sum per head, the heads `sq_err_hs` doubles apart (a
// stage of a grouped stack).
int run_keys_leg(const vq_args *a, const KeysPlan &kp, bool key_planes, int acc, const Device &dev, const Switches &sw, hipStream_t s,
                 const ResidualStage *rst = nullptr, int sq_err_hs = 0) {
    long long *keys = (long long *)a->workspace;
    float *loss_part = ws_loss_part(a);
    int rc;
    if (!key_planes) {
        rc = vq_keys_init((int64_t *)keys, (int64_t)a->H * a->M, s);
        if (rc) return rc;
    }
    rc = run_search_keys(a, kp, 0, keys, key_planes ? (long long)a->H * a->M : 0, dev, sw, s);
    if (rc) return rc;
    int nparts = 0;
    rc = run_finalize(a, keys, a->sq_err ? loss_part : nullptr, s, &nparts, key_planes ? kp.splits : 1, rst);
    if (rc) return rc;
    if (!a->sq_err) return 0;
    if (sq_err_hs > 0)  // the finalize's partials are [head][nparts / H]
        return reduce_loss(dim3(1, a->H), s, loss_part, nparts / a->H, 1, a->sq_err, acc, sq_err_hs);
    return reduce_loss(dim3(1), s, loss_part, nparts, 1, a->sq_err, acc);
}

// kLegStaged: the tail rows `t` of the residual stack `a`, stage by stage; the residual rows [H][rows][D] lie behind the keys
// and the loss partials of the whole call
int run_staged_leg(const vq_args *a, const vq_args &tail, const Leg &leg, const Device &dev, const Switches &sw, hipStream_t s) {
    float *R = (float *)((char *)a->workspace + ws_core_bytes(a->H, a->M, a->Q));
    for (int q = 0; q < a->Q; ++q) {
        vq_args t = tail;
        t.Q = 1;
        if (q > 0) {
            t.x = R;
            t.x_rs = a->D;
            t.x_hs = tail.M * a->D;
        }
        t.cb = a->cb + (long long)q * a->cb_qs;
        t.packed = a->packed + (long long)q * a->pk_qs;
        t.idx = tail.idx + (long long)q * a->idx_qs;
        if (a->best) t.best = tail.best + (long long)q * a->idx_qs;
        if (a->sq_err) t.sq_err = a->sq_err + q;
        t.workspace_bytes = ws_core_bytes(a->H, a->M, a->Q);
        ResidualStage rst;
        rst.res_next = (q + 1 < a->Q) ? R : nullptr;
        rst.out_acc = q > 0;
        t.flags &= ~VQ_F_SQERR_PER_HEAD;
        const int by_head_hs = ((a->flags & VQ_F_SQERR_PER_HEAD) && a->sq_err) ? a->Q : 0;  // sq_err is [H][Q]: stage q of head h at h * Q + q
        if (int rc = run_keys_leg(&t, leg.keys, leg.planes, /*acc=*/1, dev, sw, s, &rst, by_head_hs)) return rc;
    }
    return 0;
}

// kLegFused: one launch of the chosen kernel, then the sum of the partials it wrote
int run_fused_leg(const vq_args *a, const Leg &leg, float *lse, const Device &dev, const Switches &sw, hipStream_t s) {
    if (!a->packed) return fail(VQ_E_BADARG, "vq_quantize: packed codebook is null");
    if (vq_packed_floats(a->K, a->D) * 4 >= (1ll << 31))
        return fail(VQ_E_UNSUPPORTED, "vq_quantize: packed codebook image >= 2 GiB (shard the codebook)");
    float *loss_part = ws_loss_part(a);
    SearchParams p;
    fill_search_params(p, a);
    p.mode = kModeFused;
    p.loss_part = a->sq_err ? loss_part : nullptr;
    p.lse = lse;
    p.res_img_floats = leg.res_img_floats;
    if (leg.res_img_floats) {
        p.res_skew = sw.res_skew;
        p.res_nbuf = leg.res_nbuf;
    }
    const SearchChoice &c = leg.choice;  // the screen images, the launch and the partials' count all follow it
    if (c.screened) set_screen_image(p, a, c);
    const int rc = launch_search(c, leg.DP, p, a->H, 1, a->metric, dev.cus, s);
    if (rc || !a->sq_err) return rc;
    const long long per_head = loss_partials_per_head(c, a->M, a->H, dev.cus);
    const bool by_head = (a->flags & VQ_F_SQERR_PER_HEAD) != 0;
    return reduce_loss(dim3(a->Q, by_head ? a->H : 1), s, loss_part, by_head ? per_head : per_head * a->H, a->Q, a->sq_err, leg.accumulate);
}

int run_leg(const vq_args *a, const Leg &leg, float *lse, const Device &dev, const Switches &sw, hipStream_t s) {
    const vq_args rows = rows_from(*a, leg.row_begin, leg.rows);
    switch (leg.kind) {
        case kLegFused: return run_fused_leg(&rows, leg, lse, dev, sw, s);
        case kLegStaged: return run_staged_leg(a, rows, leg, dev, sw, s);
        case kLegWideFused: return run_wide(&rows, leg.wide, 0, nullptr, nullptr, 0, 0, dev, sw, s, true);
        case kLegKeys:
        case kLegWideKeys:
        case kLegScalar: return run_keys_leg(&rows, leg.keys, leg.planes, leg.accumulate, dev, sw, s);
        case kLegNoStack: return fail(VQ_E_UNSUPPORTED, "vq_quantize: residual stages need the MFMA kernel (D <= 512)");
        case kLegNoPerHead: break;
    }
    return fail(VQ_E_UNSUPPORTED, "vq_quantize: per-head squared errors need the MFMA kernel (D <= 512)");
}

// check the arguments, describe the call, plan, execute
int quantize_impl(const vq_args *a, void *stream, float *lse) {
    int rc = check_common(a);
    if (rc) return rc;
    rc = check_screen(a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (lse && (a->Q != 1 || padded_dim(a->D) == 0 || (a->flags & (VQ_F_FORCE_SIMPLE | VQ_F_FORCE_SPLIT))))
        return fail(VQ_E_UNSUPPORTED, "vq_quantize_lse: needs Q == 1, D <= 512 and the fused MFMA path");
    if ((a->flags & (VQ_F_X_F16 | VQ_F_X_BF16)) &&
        (a->Q != 1 || padded_dim(a->D) == 0 || lse || a->sq_err || (a->flags & (VQ_F_STE | VQ_F_FORCE_SIMPLE))))
        return fail(VQ_E_UNSUPPORTED, "vq_quantize: 2-byte rows are inference only (Q == 1, D <= 512, no STE / sq_err / lse)");
    if (a->M > 0 && !a->idx) return fail(VQ_E_BADARG, "vq_quantize: idx is null");
    if (a->M > 0 && !a->cb) return fail(VQ_E_BADARG, "vq_quantize: natural codebook is null");
    if (a->M == 0) return a->sq_err ? clear_sq_err(a->sq_err, sq_err_count(a), s, "vq_quantize: clearing sq_err") : 0;
    if (!a->workspace || a->workspace_bytes < vq_workspace_bytes(a->H, a->M, a->Q))
        return fail(VQ_E_BADARG, "vq_quantize: workspace too small (see vq_workspace_bytes)");

    const Device dev = plan_device();
    const Switches sw = read_switches();
    const CallPlan plan = plan_call(describe_call(a, lse != nullptr), dev, sw);
    if (plan.nlegs > 0 && plan.leg[0].accumulate && a->sq_err) {  // (nothing ran before it: its stages ADD their sums)
        rc = clear_sq_err(a->sq_err, sq_err_count(a), s, "vq_quantize: clearing sq_err");
        if (rc) return rc;
    }
    for (int i = 0; i < plan.nlegs; ++i) {
        rc = run_leg(a, plan.leg[i], lse, dev, sw, s);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

// =================================================================================================
// C ABI of the search
// =================================================================================================
extern "C" {

int vq_quantize_f32(const vq_args *a, void *stream) { return quantize_impl(a, stream, nullptr); }

int vq_quantize_lse_f32(const vq_args *a, float *lse, void *stream) {
    if (!lse && a && a->M > 0) return fail(VQ_E_BADARG, "vq_quantize_lse: lse is null");
    return quantize_impl(a, stream, lse);
}

int vq_keys_init(int64_t *keys, int64_t n, void *stream) {
    if (!keys || n < 0) return fail(VQ_E_BADARG, "vq_keys_init: bad argument");
    if (n == 0) return 0;
    return launch<vq_keys_init_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, "vq_keys_init launch", (long long *)keys,
                                       (long long)n);
}

static int check_keys_entry(const vq_args *a, int64_t idx_offset, const int64_t *keys, const char *who) {
    if (int rc = check_common(a)) return rc;
    if (a->Q != 1) return fail(VQ_E_BADARG, who, "Q must be 1");
    if (!keys) return fail(VQ_E_BADARG, who, "keys is null");
    if (idx_offset < 0 || idx_offset + a->K > 0xFFFFFFFFll) return fail(VQ_E_BADARG, who, "index range");
    return 0;
}

int vq_search_keys_f32(const vq_args *a, int64_t idx_offset, int64_t *keys, void *stream) {
    if (int rc = check_keys_entry(a, idx_offset, keys, "vq_search_keys")) return rc;
    if (a->M == 0) return 0;
    const Device dev = plan_device();
    const Switches sw = read_switches();
    return run_search_keys(a, plan_keys_of(a, 0, dev, sw), idx_offset, (long long *)keys, 0, dev, sw, (hipStream_t)stream);
}

int vq_key_planes(const vq_args *a) {
    if (check_common(a) || a->Q != 1 || a->M == 0) return 1;
    const KeysPlan kp = plan_keys_of(a, 0, plan_device(), read_switches());
    return kp.mfma ? kp.splits : 1;
}

int vq_search_key_planes_f32(const vq_args *a, int64_t idx_offset, int64_t *keys, void *stream) {
    if (int rc = check_keys_entry(a, idx_offset, keys, "vq_search_key_planes")) return rc;
    if (a->M == 0) return 0;
    const Device dev = plan_device();
    const Switches sw = read_switches();
    const KeysPlan kp = plan_keys_of(a, 0, dev, sw);
    if (!kp.mfma)  // scalar kernel / wide rows: one plane, combined with atomic MIN
        if (int rc = vq_keys_init(keys, (int64_t)a->H * a->M, stream)) return rc;
    return run_search_keys(a, kp, idx_offset, (long long *)keys, kp.mfma ? (long long)a->H * a->M : 0, dev, sw, (hipStream_t)stream);
}

int vq_finalize_keys_f32(const vq_args *a, const int64_t *keys, void *stream) { return vq_finalize_key_planes_f32(a, keys, 1, stream); }

int vq_finalize_key_planes_f32(const vq_args *a, const int64_t *keys, int n_planes, void *stream) {
    int rc = check_common(a);
    if (rc) return rc;
    if (n_planes < 1) return fail(VQ_E_BADARG, "vq_finalize_keys: n_planes must be >= 1");
    if (a->Q != 1) return fail(VQ_E_BADARG, "vq_finalize_keys: Q must be 1");
    if (a->M == 0) {  // (no rows: no keys either -- an empty tensor's address is null, as x's may be in check_common)
        return a->sq_err ? clear_sq_err(a->sq_err, 1, (hipStream_t)stream, "vq_finalize_keys: clearing sq_err") : 0;
    }
    if (!keys || !a->cb) return fail(VQ_E_BADARG, "vq_finalize_keys: keys / cb is null");
    hipStream_t s = (hipStream_t)stream;
    float *loss_part = nullptr;
    if (a->sq_err) {
        if (!a->workspace || a->workspace_bytes < vq_workspace_bytes(a->H, a->M, 1))
            return fail(VQ_E_BADARG, "vq_finalize_keys: workspace too small");
        loss_part = ws_loss_part(a);
    }
    int nparts = 0;
    rc = run_finalize(a, (const long long *)keys, loss_part, s, &nparts, n_planes);
    if (rc) return rc;
    return a->sq_err ? reduce_loss(dim3(1), s, loss_part, nparts, 1, a->sq_err, 0) : 0;
}

}  // extern "C"
