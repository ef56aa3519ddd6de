// vq_search_resident.inc -- small codebooks: the WHOLE packed image stays in LDS and the waves stream row blocks past it.
// Included by vq_kernels.hip after vq_search.inc (same SearchParams, fragment pipeline, epilogue, tie rule, non-finite repair).
//
// Why: with K = 256 a row block's sweep is 8 sub-tiles (17 k cycles per wave at Dp = 64) -- as long as the fixed work around
// it: staging a tile per barrier, the row prologue (an HBM read burst), the fused finalize (an HBM write burst).  The
// one-block kernel reaches 0.43-0.52 of the MFMA peak there (profiles/r02_shape_scan.md), whatever the row count.
// Here (BASELINE configs[0]'s class: K = 256, D = 64)
//   * the image (Kp x (Dp + 4) floats, <= ~140 KB) is copied to LDS ONCE per workgroup; after that there is no tile DMA
//     and NO BARRIER: the 8 waves of the (one) workgroup per CU are independent, each walks its own 32-row blocks
//     (block id = wave slot, + number of wave slots, ...);
//   * the rows of the NEXT block arrive during the current sweep: 16 dims of 32 rows (2 KiB) per LDS-DMA job into a
//     wave-private slab -- lane l fetches piece l / 16 of row l % 16, so a slab is [piece][row] and the fragment reads
//     (ds_read_b128, lane (c, h) <- its row's four pieces) are conflict free -- and are turned into the next block's
//     MFMA fragments one slab per sub-tile: both lane halves read the whole 16 dims and keep their k-parity (two
//     v_cndmask per float4, no cross-lane traffic), the lower half also walks the d-ordered |x|^2 chain;
//   * the rows of the PREVIOUS block are copied out (out[row] = codebook[idx[row]]) during the sweep as well, a
//     64-lane float4 access covering 64 / (Dp / 4) rows: load at sub-tile n, store at sub-tile n + 1 (vq_search_persist's
//     scheme).
// Everything that decides results -- the k-ordered MFMA chain with the augmented column, the min3 tree, the parked
// sub-tile, the rounding-band resolve, the non-finite repair -- is vq_search_mfma's code: same bits.
template <int DP>
struct ResGeo {
    static constexpr int RS = DP + 4, RS4 = RS / 4;
    static constexpr int NSLAB = DP / 16;          // 16-dim slabs per row
    static constexpr int SLAB_F = 32 * 16;         // floats of one wave's slab (2 KiB)
    static constexpr int LPR = DP / 4;             // lanes per natural row in the copy (one float4 each)
    static constexpr int RPI = 64 / LPR;           // rows per copy access
    static constexpr int CPS = DP >= 128 ? 1 : (32 / RPI + 7) / 8;  // copy accesses per sub-tile: everything is hidden from 8
                                                   // sub-tiles on (Dp = 128: from 16 on -- registers)
    static constexpr int RPSTEP = RPI * CPS;       // rows per copy step
    // LDS: image | 8 waves x nbuf slabs | winners of two blocks (resident_lds_bytes, vq_search_plan.h).  nbuf = NSLAB (a whole
    // block of rows in flight per wave) when that fits beside the image, else 1 (resident_buffers)
    static_assert(resident_lds_bytes(0, 1) == (size_t)8 * SLAB_F * 4 + 2 * 8 * 32 * 4, "vq_search_plan.h sizes this kernel's LDS");
};

// global_load_lds_dwordx4: 16 bytes per lane from src + OFF (an instruction immediate) -> LDS at lds_dst + lane * 16.
// The hardware adds the immediate to BOTH addresses (memory and LDS), so the LDS base handed to the instruction is
// lds_dst - OFF.
template <int OFF = 0>
__device__ __forceinline__ void glds16(const float *src, float *lds_dst) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)(lds_dst - OFF / 4), 16, OFF, 0);
#else
    (void)src; (void)lds_dst;
#endif
}

// (vector instructions are not free beside fp32 MFMA: every one of them costs the matrix pipe ~7 cycles -- at K = 256 a
//  block has only 264 MFMAs to hide them behind; hence immediates, uniform bases and static schedules below)

// slab J of the block staged in `slab` -> fragments xf[8 J .. 8 J + 7] (+ 16 steps of the |x|^2 chain).  J is a compile-time
// constant everywhere: the fragment registers must never be indexed at run time (they would become a stack array)
template <int DP, int J, bool EUCLID>
__device__ __forceinline__ void slab_take(const float *slab, int c, int h, int D, float (&xf)[DP / 2], float &xn) {
    (void)D;
    const float *rp = slab + (c >> 4) * 256 + (c & 15) * 4;  // [half of the rows][piece][row % 16][4 floats]
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) {
        const f32x4 v = *(const f32x4 *)(rp + pc * 64);
        if (EUCLID) {
            xn = fmaf(v.x, v.x, xn);
            xn = fmaf(v.y, v.y, xn);
            xn = fmaf(v.z, v.z, xn);
            xn = fmaf(v.w, v.w, xn);
        }
        xf[8 * J + 2 * pc] = h ? v.y : v.x;      // dim 16 J + 4 pc + h
        xf[8 * J + 2 * pc + 1] = h ? v.w : v.z;  // dim 16 J + 4 pc + 2 + h
    }
}

// compile-time loop: f(IntC<0>{}), f(IntC<1>{}), ...
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(IntC<I>{});
        static_for<N, I + 1>(f);
    }
}

// RING: a slab buffer per slab of a block (Dp <= 64 and the image leaves room: the launcher's choice is a kernel instantiation);
// else one buffer, slab g + 1 requested when slab g has been taken.
template <int DP, int METRIC, bool RING>
__global__ void __launch_bounds__(512, 2) vq_search_resident(const SearchParams p) {
    constexpr int WAVES = 8;
    using RG = ResGeo<DP>;
    constexpr int RS = RG::RS, RS4 = RG::RS4, NS = DP / 2, NG = DP / 8, NSLAB = RG::NSLAB;
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    constexpr bool TWO_ACC = DP < 128;
    constexpr int NBUF = RING ? NSLAB : 1;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float *pk = p.packed + (long long)head * p.pk_hs;
    const float *cbh = p.cb + (long long)head * p.cb_hs;
    float *outh = p.out + (long long)head * p.out_hs;
    const float INF = __builtin_inff();
    const int img_floats = p.res_img_floats;
    const f32x4 *img4 = (const f32x4 *)smem;
    float *slab = smem + img_floats + wave * NBUF * RG::SLAB_F;           // this wave's slab buffer(s)
    int *sidx = (int *)(smem + img_floats + WAVES * NBUF * RG::SLAB_F);   // [2][WAVES][32]: winners of the current / previous block
    const int nsub = (p.K + kTileCodes - 1) / kTileCodes;                 // >= NSLAB (the launcher's rule)
    const long long nwb = (p.M + 31) / 32;                                // 32-row wave blocks
    const long long wstride = (long long)gridDim.x * WAVES;
    long long wb = (long long)blockIdx.x * WAVES + wave;

#ifdef VQ_EXP_STAMPS
    unsigned long long st_sweep = 0, st_left = 0, st_post = 0, st_blocks = 0, st_t = 0;
#define RSTAMP_BEGIN() (st_t = __builtin_amdgcn_s_memtime())
#define RSTAMP_ADD(acc) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc += now_ - st_t; st_t = now_; } while (0)
#else
#define RSTAMP_BEGIN() do { } while (0)
#define RSTAMP_ADD(acc) do { } while (0)
#endif
    STAMP(0);
    STAMP_RT(60);
    // ---------------- the image: global -> LDS, once (LDS-DMA, 1 KiB per wave copy) ----------------
    for (int ck = wave; ck * 256 < img_floats; ck += WAVES)
        lds_dma16(pk, p.pk_bytes, lane * 16, ck * 1024, (lds_f32x4 *)smem + ck * 64);

    // Slab jobs: 16 dims of the 32 rows from `row0` on -> a slab buffer, [half of the rows][piece][row % 16].  The two per-lane
    // row pointers are computed once per block; the slab's position in the row is the instruction's immediate offset.
    const int srow = lane & 15, spiece = lane >> 4;
    const float *rp0 = xh, *rp1 = xh;  // this lane's two rows of the block being fetched
    auto slab_rows = [&](long long row0) {
        long long g0 = row0 + srow, g1 = row0 + srow + 16;
        g0 = g0 < p.M ? g0 : p.M - 1;
        g1 = g1 < p.M ? g1 : p.M - 1;
        rp0 = xh + g0 * p.x_rs + spiece * 4;
        rp1 = xh + g1 * p.x_rs + spiece * 4;
    };
    auto slab_issue = [&](auto jc) {  // slab J of the rows set by slab_rows
        constexpr int J = decltype(jc)::value;
        if (J * 16 < p.D) {
            glds16<J * 64>(rp0, slab + (RING ? J * RG::SLAB_F : 0));
            glds16<J * 64>(rp1, slab + (RING ? J * RG::SLAB_F : 0) + 256);
        }
    };
    auto slab_issue_all = [&](long long row0) {  // RING: a whole block of rows
        slab_rows(row0);
        static_for<NSLAB>([&](auto jc) { slab_issue(jc); });
    };

    // ---------------- the first block's rows, in the open ----------------
    float xf[NS], xfn[NS];
    float xn0 = 0.0f, xnn = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        xf[s] = 0.0f;
        xfn[s] = 0.0f;  // (slabs past the row's real dims are never taken: they stay zero)
    }
    if (wb < nwb) {
        slab_rows(wb * 32);
        if constexpr (RING) static_for<NSLAB>([&](auto jc) { slab_issue(jc); });
        static_for<NSLAB>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J * 16 < p.D) {
                if constexpr (!RING) slab_issue(jc);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                slab_take<DP, J, EUCLID>(slab + (RING ? J * RG::SLAB_F : 0), c, h, p.D, xf, xn0);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read before the buffer is refilled
            }
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // the image is complete for every wave -- the only barrier of this kernel
    STAMP(1);
    if (wave >= 4)
        for (int i = 0; i < p.res_skew; ++i) __builtin_amdgcn_s_sleep(127);  // (diagnostic: start-up skew of a SIMD's second wave)

    // deferred copy of the previous block's rows
    // (addresses = a wave-uniform base + a 32-bit per-lane byte offset: one v_mad per access instead of 64-bit arithmetic)
    constexpr int LPR = RG::LPR, RPI = RG::RPI, CPS = RG::CPS, RPSTEP = RG::RPSTEP;
    const int csub = lane / LPR, cdl = 4 * (lane % LPR);
    const bool cdok = cdl < p.D;
    const unsigned out_rs4 = (unsigned)p.out_rs * 4u, d4 = (unsigned)p.D * 4u, cdl4 = (unsigned)cdl * 4u;
    int cp_rows = 0, cp_next = 0, cp_pend = -1;
    long long cp_row0 = 0;
    const int *cp_idx = sidx;
    f32x4 cp_v[CPS];
#pragma unroll
    for (int k = 0; k < CPS; ++k) cp_v[k] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    auto copy_step = [&]() {
        if (cp_pend >= 0) {
            const char *obase = (const char *)(outh + cp_row0 * p.out_rs);  // (uniform)
#pragma unroll
            for (int k = 0; k < CPS; ++k) {
                const int rr = cp_pend + k * RPI + csub;
                if (rr < cp_rows && cdok) __builtin_nontemporal_store(cp_v[k], (f32x4 *)(obase + ((unsigned)rr * out_rs4 + cdl4)));
            }
            cp_pend = -1;
        }
        if (cp_next < cp_rows) {
#pragma unroll
            for (int k = 0; k < CPS; ++k) {
                int rr = cp_next + k * RPI + csub;
                rr = rr < cp_rows ? rr : cp_rows - 1;
                const unsigned i = (unsigned)cp_idx[rr];
                if (cdok) cp_v[k] = *(const f32x4 *)((const char *)cbh + (i * d4 + cdl4));
            }
            cp_pend = cp_next;
            cp_next += RPSTEP;
        }
    };

    const float start_value = sweep_start_value<METRIC>(codebook_flag(pk, p.pk_bytes));  // (one load for the whole kernel)
    // The rows of a block are requested as early as their buffers allow.  RING: all slabs of block b + 2 when the last slab of
    // block b + 1 has been taken (a whole sweep ahead).  One buffer: slab g + 1 when slab g has been taken, slab 0 of block
    // b + 2 after the last one.  Here: the second block's.
    if (wb + wstride < nwb) {
        slab_rows((wb + wstride) * 32);
        if constexpr (RING) static_for<NSLAB>([&](auto jc) { slab_issue(jc); });
        else slab_issue(IntC<0>{});
    }
    int it = 0;
    for (; wb < nwb; wb += wstride, ++it) {
        const long long row0 = wb * 32;
        const bool has_next = wb + wstride < nwb, has_next2 = wb + 2 * wstride < nwb;
        const long long nrow0 = (wb + wstride) * 32;
        const long long row = row0 + c;
        const bool row_ok = row < p.M;
        const float b_aug = EUCLID ? (h ? 1.0f : xn0) : 1.0f;

        LaneBest lb = lane_best_start<METRIC>(start_value);
        xnn = 0.0f;
        RSTAMP_BEGIN();

        // one sub-tile: Dp/2 + 1 MFMAs against sub-tile u of the resident image; `job` = this sub-tile's share of the next
        // block's rows (a slab take, compile-time slab index) or nothing; one step of the previous block's copy
        auto run_sub = [&](f32x16 &acc, f32x16 &prev, int u, bool have_prev, auto &&job) {
            const f32x4 *ta = img4 + (u * kTileCodes + c) * RS4 + h;
            constexpr int G1 = NG >= 2 ? 1 : NG;
            f32x4 a[NG];
            acc = (f32x16){0};
            const float a_aug = EUCLID ? smem[(u * kTileCodes + c) * RS + DP + 1 - h] : 0.0f;
            mfma_prefetch<DP>(a, ta);
#ifdef VQ_EXP_STAMPS
            if (it == 2 && u < 24) STAMP(8 + u);
#endif
            job();
            copy_step();
            mfma_range<DP, 0, G1>(acc, a, ta, xf);
            if constexpr (TWO_ACC) {
                if (have_prev) tile_epilogue<METRIC, DP, false>(prev, u - 1, h, p.K, lb);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_range<DP, G1, NG>(acc, a, ta, xf);
            if (EUCLID) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
        };
        auto no_job = [] {};
        // slab G of the NEXT block -> xfn (static fragment registers), then the request its buffer allows
        auto take_job = [&](auto gc) {
            constexpr int G = decltype(gc)::value;
            if (!has_next) return;
            if (G * 16 < p.D) {
                if (!RING || G == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (requested a sub-tile / a whole sweep ago)
                slab_take<DP, G, EUCLID>(slab + (RING ? G * RG::SLAB_F : 0), c, h, p.D, xfn, xnn);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read before the buffer is refilled
            }
            if constexpr (G + 1 < NSLAB) {
                if constexpr (!RING) slab_issue(IntC<G + 1>{});
            } else if (has_next2) {
                slab_rows(nrow0 + wstride * 32);
                if constexpr (RING) static_for<NSLAB>([&](auto jc) { slab_issue(jc); });
                else slab_issue(IntC<0>{});
            }
        };
        if constexpr (!RING) {
            if (has_next) slab_rows(nrow0);  // (one buffer: the row pointers of the block being fetched slab by slab)
        }

        f32x16 acc0, acc1;
        // head: the first NSLAB sub-tiles also take the NSLAB slabs of the next block (nsub >= NSLAB)
        static_for<NSLAB>([&](auto gc) {
            constexpr int G = decltype(gc)::value;
            if constexpr (TWO_ACC) {
                run_sub((G & 1) ? acc1 : acc0, (G & 1) ? acc0 : acc1, G, G > 0, [&] { take_job(gc); });
            } else {
                run_sub(acc0, acc0, G, false, [&] { take_job(gc); });
                tile_epilogue<METRIC, DP, false>(acc0, G, h, p.K, lb);
            }
        });
        // tail: the rest of the codebook (NSLAB is even: acc0 is next)
        if constexpr (TWO_ACC) {
            int u = NSLAB;
            for (; u + 1 < nsub; u += 2) {
                run_sub(acc0, acc1, u, true, no_job);
                run_sub(acc1, acc0, u + 1, true, no_job);
            }
            if (u < nsub) {
                run_sub(acc0, acc1, u, true, no_job);
                tile_epilogue<METRIC, DP, false>(acc0, u, h, p.K, lb);
            } else {
                tile_epilogue<METRIC, DP, false>(acc1, u - 1, h, p.K, lb);
            }
        } else {
            for (int u = NSLAB; u < nsub; ++u) {
                run_sub(acc0, acc0, u, false, no_job);
                tile_epilogue<METRIC, DP, false>(acc0, u, h, p.K, lb);
            }
        }
#ifdef VQ_EXP_STAMPS
        if (it == 2) STAMP(32);
#endif
        RSTAMP_ADD(st_sweep);
        // what the sweep was too short to hide: the rest of the copy
        while (cp_next < cp_rows || cp_pend >= 0) copy_step();
        RSTAMP_ADD(st_left);

        float best_s;
        int best_i;
        row_winner<METRIC>(lb, h, p.K, best_s, best_i);
        // non-finite inputs (rare, out of line; see repair_nonfinite_rows).  The row buffer is slab buffer 0, which may hold (or
        // be receiving) rows of the block after next: wait for them, use it, fetch them again.
        if (const unsigned todo = nonfinite_rows(best_s, row_ok); __builtin_expect(todo != 0u, 0)) {
            auto fill_row = [&](int rr) -> float { return fill_row_from_memory<METRIC, DP, 0, 0>(p, head, row0 + rr, slab, lane); };
            auto acc_init = [&](int, int) -> float { return 0.0f; };
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            repair_nonfinite_rows<METRIC, DP>(todo, slab, pk, 0, p.K, lane, fill_row, acc_init, best_s, best_i);
            if (has_next2) {
                slab_rows(nrow0 + wstride * 32);
                slab_issue(IntC<0>{});
            }
        }
        if (h == 0 && row_ok) store_winner(p, head, row, 0, best_s, best_i);
        int *mine = sidx + ((it & 1) * WAVES + wave) * 32;
        mine[c] = best_i;
        // this block becomes the one to copy during the next sweep (wave-private LDS: in order, no barrier needed)
        cp_rows = (p.M - row0 >= 32) ? 32 : (int)(p.M - row0);
        cp_row0 = row0;
        cp_idx = mine;
        cp_next = 0;
        cp_pend = -1;
        if (has_next) {
#pragma unroll
            for (int s = 0; s < NS; ++s) xf[s] = xfn[s];
            xn0 = xnn;
        }
        RSTAMP_ADD(st_post);
#ifdef VQ_EXP_STAMPS
        if (it == 2) STAMP(33);
        ++st_blocks;
#endif
    }
    // ---------------- the last block of this wave: copy in the open ----------------
    while (cp_next < cp_rows || cp_pend >= 0) copy_step();
    STAMP(2);
    STAMP(3);
    STAMP_RT(61);
#ifdef VQ_EXP_STAMPS
    if (lane == 0) {
        unsigned long long *sp = g_stamps + (((long long)blockIdx.x * WAVES + wave) & 8191) * VQ_NSTAMP;
        sp[4] = st_sweep; sp[5] = st_left; sp[6] = st_post; sp[7] = st_blocks;
    }
#endif
#undef RSTAMP_BEGIN
#undef RSTAMP_ADD
}
