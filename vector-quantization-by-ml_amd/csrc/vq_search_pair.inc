// vq_search_pair.inc -- the search kernel for 256 < D <= 512: the dims of a row block are split over a PAIR of waves.
// Included by vq_kernels.hip after vq_search.inc (same SearchParams, epilogue, tie rule, residual arithmetic).
//
// Why: 512 dims of 32 rows are 256 fragment registers per lane, i.e. one wave per SIMD -- nothing covers that wave's own
// epilogue, LDS waits and barriers (vq_search_mfma<512, 4>: the sweep runs at 86 % of the MFMA issue floor, against 96 % for
// Dp = 256 with two waves per SIMD).  Here wave A of a pair holds dims 0..255 of the pair's 32 rows and wave B dims 256..511
// (128 registers each, two waves per SIMD again).  For every 32-code tile A runs its 128 k-steps and hands the 32 x 32
// accumulator to B through LDS; B loads it as ITS accumulator, continues the SAME k-ordered chain over dims 256..511, adds
// the augmented column and owns the epilogue -- so every distance is bit for bit the single-wave chain
// fma(.., fma(x_1 * -2c_1, fma(x_0 * -2c_0, 0))) of oracle/vq_oracle.c.  B runs one tile behind A; tiles are staged as
// half rows (1 KiB = one buffer_load ... lds each), A-halves one tile ahead of the B-halves, so LDS holds four half tiles
// (the same 133 KB as two whole tiles) + 16 KB of hand-off slots.
//
// Hand-off protocol of a pair (one slot): A writes accumulator s at the END of step s, after it has seen flag >= s; B reads
// it at the START of step s + 1, waits for the read (lgkmcnt) and then sets flag = s + 1.  The workgroup barrier that ends
// every step (it also publishes the staged tiles) orders A's write before B's read; the flag orders B's read before A's
// next write.
struct PairGeo {
    static constexpr int HT_F = 32 * (256 + 4);        // floats per half-tile buffer (32 half rows, stride 260)
    static constexpr int TILE_FLOATS = 4 * HT_F;       // A-halves and B-halves, double buffered (also: prologue staging,
                                                       // gather regions of the residual update -- both 8 x 2176 floats)
    static constexpr int HAND_FLOATS = 4 * 1024;       // one accumulator slot per pair
    static constexpr int FIXED_FLOATS = TILE_FLOATS + HAND_FLOATS + 128 + 8;  // + |x|^2 hand-off + flags
    // (+ the winners of every stage; the per-stage squared-error partials of a residual launch live in the tile buffers, idle by then)
    static constexpr size_t lds_bytes(int Q) { return (size_t)FIXED_FLOATS * 4 + (size_t)4 * Q * 32 * 4; }
    static constexpr int max_stages() {
        int q = 1;
        while (q < 64 && lds_bytes(q + 1) <= 160 * 1024) ++q;  // (64: 8 waves x Q x 64 partials must fit the tile buffers)
        return q;
    }
};
static_assert(PairGeo::max_stages() == kPairMaxStages, "vq_search_plan.h plans with this kernel's stage limit");

// MULTI (round 3): residual stacks (1 eval arithmetic, 2 straight-through arithmetic, as in vq_search_mfma).  After every
// sweep B publishes the winners, then BOTH waves of a pair gather their half (1 KiB) of the winners' packed rows slice by
// slice through their wave-private LDS regions and update their 128 residual registers in place; A walks its half of the
// next stage's |r|^2 chain during the update and publishes it, B continues it at the start of the next sweep (exactly as
// for stage 0).  Non-finite rows (rare): A dumps its half of the flagged rows to LDS, B adds its own and runs the repair.
// WIDE (rows wider than 512 dims, swept in 512-dim slices; see vq_search_mfma): 1 a full slice whose accumulators go to
// `acc_ws` instead of the argmin, 2 the last slice (starts from `acc_ws`, ends in the argmin: keys, or the whole inference
// call), 3 the last slice emitting the similarity matrix.  From the second slice on wave A STARTS each tile from the chain the
// earlier slices left in the workspace (loaded one tile ahead); the hand-off to B and B's half are unchanged.
template <int METRIC, bool LSE = false, int XT = 0, int WIDE = 0, int MULTI = 0>
__global__ void __launch_bounds__(512, 2) vq_search_pair512(const SearchParams p) {
    static_assert(WIDE == 0 || (!LSE && XT == 0), "wide rows: plain fp32 slices");
    static_assert(MULTI == 0 || (WIDE == 0 && !LSE && XT == 0), "residual stacks: plain fp32 rows");
    constexpr bool WIDE_OUT = (WIDE == 1 || WIDE == 3);
    constexpr int HD = 256;            // dims per wave
    constexpr int NS = HD / 2;         // MFMA k-steps per wave and tile
    constexpr int RSH = HD + 4;        // LDS half-row stride, floats (same bank rotation as the Dp = 256 tiles)
    constexpr int RSH4 = RSH / 4;
    constexpr int RSP = 512 + 4;       // packed row stride, floats
    constexpr int HT_F = 32 * RSH;     // floats per half-tile buffer
    constexpr int CH = 32, XS = 64 + 4;  // (row chunks of 32 dims: the 64-dim chunks of the other kernels cost 32 more registers here, spilled)
    constexpr int WAVES = 8;
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    using G = Geo<256, 8>;             // gather geometry of one 256-dim half (slices of 64 dims)
    using PG = PairGeo;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *hand_all = smem + PG::TILE_FLOATS;              // [4 pairs][1024]
    float *xn_a = hand_all + PG::HAND_FLOATS;              // [4 pairs][32]: A's part of the |x|^2 chain
    volatile int *flags = (volatile int *)(xn_a + 128);    // [4 pairs] (+ pad)
    int *sidx = (int *)(xn_a + 128 + 8);                   // [4 pairs][Q][32]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Waves 2p and 2p + 1 form pair p.  With the dispatcher's round-robin wave -> SIMD placement this puts two A waves (or
    // two B waves) on a SIMD; measured 2.5 % faster than keeping a pair's own A and B on one SIMD (waves w, w + 4: 0.894 vs
    // 0.918 of peak at cfg3b) and 0.8 % faster than mixing the A and B of different pairs.  Correctness does not depend on it.
    const int pair = wave >> 1, role = wave & 1;
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const long long row0 = ((long long)blockIdx.x * 4 + pair) * 32;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float INF = __builtin_inff();
    const int dbase = role * HD;                           // first dim this wave owns

    // ---------------- prologue: this wave's half of the pair's 32 rows -> MFMA fragments ----------------
    STAMP(0);
    STAMP_RT(60);
    __builtin_amdgcn_s_setprio(2);
    float xf[NS];
    float xn0 = 0.0f;
    if constexpr (WIDE != 0) {
        if (EUCLID && role == 0 && p.acc_in) {  // the |x|^2 chain over the dims of the earlier slices
            long long grow = row0 + c;
            if (grow >= p.M) grow = p.M - 1;
            xn0 = p.xn_ws[(long long)head * p.xn_hs + grow];
        }
    }
    {  // (load_x_fragments of vq_search.inc written out in place for this wave's half of the dims: see there)
        float *xs = smem + wave * (32 * XS);
        constexpr int NCHUNK = HD / CH;
        constexpr int LPL = CH / 8;
        f32x4 v[2][LPL];
        auto load_chunk = [&](int ch, f32x4 (&dst)[LPL]) {
#pragma unroll
            for (int it = 0; it < LPL; ++it) {
                const int f = it * 64 + lane;
                const int r = f / (CH / 4), c4 = f % (CH / 4);
                long long grow = row0 + r;
                if (grow >= p.M) grow = p.M - 1;
                const int d0 = dbase + ch * CH + c4 * 4;
                f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (XT == 0) {
                    const float *src = xh + grow * p.x_rs + d0;
                    if (p.vec_x) {
                        if (d0 < p.D) t = __builtin_nontemporal_load((const f32x4 *)src);
                    } else {
                        if (d0 + 0 < p.D) t.x = src[0];
                        if (d0 + 1 < p.D) t.y = src[1];
                        if (d0 + 2 < p.D) t.z = src[2];
                        if (d0 + 3 < p.D) t.w = src[3];
                    }
                } else {
                    const unsigned short *src = (const unsigned short *)p.x + (long long)head * p.x_hs + grow * p.x_rs + d0;
                    if (p.vec_x) {
                        if (d0 < p.D) {
                            typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
                            const u16x4 raw = __builtin_nontemporal_load((const u16x4 *)src);
                            t = (f32x4){widen16<XT>(raw.x), widen16<XT>(raw.y), widen16<XT>(raw.z), widen16<XT>(raw.w)};
                        }
                    } else {
                        if (d0 + 0 < p.D) t.x = widen16<XT>(src[0]);
                        if (d0 + 1 < p.D) t.y = widen16<XT>(src[1]);
                        if (d0 + 2 < p.D) t.z = widen16<XT>(src[2]);
                        if (d0 + 3 < p.D) t.w = widen16<XT>(src[3]);
                    }
                }
                dst[it] = t;
            }
        };
        load_chunk(0, v[0]);
#pragma unroll
        for (int ch = 0; ch < NCHUNK; ++ch) {
            if (ch + 1 < NCHUNK) load_chunk(ch + 1, v[(ch + 1) & 1]);
#pragma unroll
            for (int it = 0; it < LPL; ++it) {
                const int f = it * 64 + lane;
                const int r = f / (CH / 4), c4 = f % (CH / 4);
                *(f32x4 *)(xs + r * XS + c4 * 4) = v[ch & 1][it];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const float *rp = xs + c * XS;
#pragma unroll
            for (int j = 0; j < CH / 8; ++j) {
                const f32x4 lo = *(const f32x4 *)(rp + 8 * j);
                const f32x4 hi = *(const f32x4 *)(rp + 8 * j + 4);
                if (EUCLID && role == 0) {  // A's part of the d-ordered |x|^2 chain (B continues it from A's value below)
                    xn0 = fmaf(lo.x, lo.x, xn0);
                    xn0 = fmaf(lo.y, lo.y, xn0);
                    xn0 = fmaf(lo.z, lo.z, xn0);
                    xn0 = fmaf(lo.w, lo.w, xn0);
                    xn0 = fmaf(hi.x, hi.x, xn0);
                    xn0 = fmaf(hi.y, hi.y, xn0);
                    xn0 = fmaf(hi.z, hi.z, xn0);
                    xn0 = fmaf(hi.w, hi.w, xn0);
                    asm volatile("" : "+v"(xn0));
                }
                const f32x4 m = h ? hi : lo;
                const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(m.x), __float_as_uint(m.y), false, false);
                const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m.z), __float_as_uint(m.w), false, false);
                const int sb = ch * (CH / 2) + 4 * j;
                xf[sb + 0] = __uint_as_float(xy[0]);
                xf[sb + 1] = __uint_as_float(zw[0]);
                xf[sb + 2] = __uint_as_float(xy[1]);
                xf[sb + 3] = __uint_as_float(zw[1]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (EUCLID && role == 0 && h == 0) xn_a[pair * 32 + c] = xn0;
        __syncthreads();  // staging region is reused as tile buffers; A's chain values are visible to B
    }
    __builtin_amdgcn_s_setprio(0);
    // (the swaps above define the fragments as register PAIRS; from here on every user wants single registers -- cut the
    //  pairing here, or the allocator drags 64-bit tuples through both role paths and spills them)
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(xf[s]));
    const long long row = row0 + c;
    const bool row_ok = row < p.M;

    // B continues the |x|^2 chain of its row over the registers it holds (the lower lane half walks the chain and fetches
    // the odd dims from its partner lane), starting from A's value
    auto chain_from = [&](float xn) {
        const int partner = (lane ^ 32) * 4;  // ds_bpermute address of the lane holding the other k-parity of this row
#pragma unroll
        for (int s0 = 0; s0 < NS; s0 += 4) {
            float t1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)  // LDS crossbar, not the vector lanes; does not clobber its operand like a swap
                t1[k] = __uint_as_float(__builtin_amdgcn_ds_bpermute(partner, __float_as_uint(xf[s0 + k])));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                xn = __builtin_fmaf(xf[s0 + k], xf[s0 + k], xn);
                xn = __builtin_fmaf(t1[k], t1[k], xn);
            }
            asm volatile("" : "+v"(xn));  // (one batch at a time: hoisting all 128 exchanges ahead of the chain spills)
        }
        return xn;
    };

    constexpr int NG = HD / 8;
    f32x4 *hand = (f32x4 *)(hand_all + pair * 1024);
    const float *pk = p.packed + (long long)head * p.pk_hs;  // (residual stacks: advanced per stage)
    const int t0 = blockIdx.z * p.tiles_per_split;
    const int t1 = (t0 + p.tiles_per_split < p.ntiles) ? t0 + p.tiles_per_split : p.ntiles;
    const int T = t1 - t0;
    // this pair's accumulator slots in the workspace: float4 index (tile * 4 + g) * 64 + lane (vq_search_mfma's layout: the
    // pair's 32-row block is row block blockIdx.x * 4 + pair of the launch)
    f32x4 *wsw = nullptr;
    if constexpr (WIDE != 0)
        wsw = (f32x4 *)p.acc_ws + (long long)head * p.ws_hs + (((long long)blockIdx.x * 4 + pair) * p.ws_nsub) * 256 + lane;
    auto ws_load = [&](f32x16 &v, int tile) {
        const f32x4 *s4 = wsw + (long long)tile * 256;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 t = s4[g * 64];
            v[4 * g + 0] = t.x; v[4 * g + 1] = t.y; v[4 * g + 2] = t.z; v[4 * g + 3] = t.w;
        }
    };

    // one half tile: 32 half rows of 1 KiB, four per wave, LDS-DMA (lane part in voffset, row position scalar)
    auto dma_half = [&](int tile, int half, int buf) {
        float *dst = smem + (half * 2 + buf) * HT_F;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = wave + 8 * i;
            lds_dma16(pk, p.pk_bytes, lane * 16, ((tile * 32 + r) * RSP + half * HD) * 4, (lds_f32x4 *)(dst + r * RSH));
        }
    };
    STAMP(1);
    for (int q = 0; q < (MULTI ? p.Q : 1); ++q) {
    if constexpr (MULTI != 0) pk = p.packed + (long long)head * p.pk_hs + (long long)q * p.pk_qs;
    if (tid < 4) flags[tid] = 0;
    dma_half(t0, 0, 0);
    __syncthreads();

    if (role == 0) {
        // ---------------- wave A: dims 0..255, one tile ahead ----------------
        f32x16 nxt = {0};  // (WIDE, from the second slice on: the next tile's chain so far, loaded one tile ahead)
        if constexpr (WIDE != 0) {
            if (p.acc_in && T > 0) ws_load(nxt, t0);
        }
        for (int s = 0; s <= T; ++s) {
            if (s < T) {
                const f32x4 *ta = (const f32x4 *)(smem + (s & 1) * HT_F) + c * RSH4 + h;
                f32x4 a[NG];
                f32x16 acc = {0};
                if constexpr (WIDE != 0) {
                    if (p.acc_in) acc = nxt;
                }
                mfma_prefetch<HD>(a, ta);
                mfma_range<HD, 0, 1>(acc, a, ta, xf);
                if constexpr (WIDE != 0) {
                    if (p.acc_in && s + 1 < T) ws_load(nxt, t0 + s + 1);
                }
                if (s + 1 < T) dma_half(t0 + s + 1, 0, (s + 1) & 1);
                dma_half(t0 + s, 1, s & 1);
                __builtin_amdgcn_sched_barrier(0);
                mfma_range<HD, 1, NG>(acc, a, ta, xf);
                while (flags[pair] < s) __builtin_amdgcn_s_sleep(1);  // B has taken accumulator s - 1 out of the slot
#pragma unroll
                for (int j = 0; j < 4; ++j) hand[j * 64 + lane] = (f32x4){acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
            }
            __syncthreads();
        }
    } else {
        // ---------------- wave B: dims 256..511, the augmented column and the epilogue, one tile behind ----------------
        // step 0: nothing to consume yet -- finish |x|^2 from A's value and issue this wave's share of the copies
        if (T > 1) dma_half(t0 + 1, 0, 1);
        dma_half(t0, 1, 0);
        float b_aug = 1.0f;
        if (EUCLID) {
            const float xn = chain_from(xn_a[pair * 32 + c]);
            b_aug = h ? 1.0f : xn;
            if constexpr (WIDE == 1) {
                if (h == 0 && row_ok) p.xn_out[(long long)head * p.xn_hs + row] = xn;  // the chain including this slice
            }
        }
        // where the accumulators leave the wave instead of entering the argmin (WIDE = 1: the workspace; 3: the similarities)
        auto ws_store = [&](const f32x16 &v, int tile) {
            if constexpr (WIDE == 3) {
                store_sims_subtile<EUCLID>(v, tile, h, row_ok, p.sims + (long long)head * p.sims_hs + row * p.sims_rs, p.K, p.vec_s);
            } else {
                f32x4 *s4 = wsw + (long long)tile * 256;
#pragma unroll
                for (int g = 0; g < 4; ++g) s4[g * 64] = (f32x4){v[4 * g + 0], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
            }
        };
        // (declared after the chain: its 16 parked registers would be live across it otherwise)
        LaneBest lb = lane_best_start<METRIC>(sweep_start_value<METRIC>(codebook_flag(pk, p.pk_bytes)));
        f32x16 acc;
        // One step of B.  The previous tile's 32 x 32 result is reduced FIRST and its registers are then reloaded from the
        // hand-off slot: B keeps ONE accumulator (two would not fit beside 128 row registers without spilling in the loop).
        auto b_step = [&](int s, bool have_prev) {
            const int tile = t0 + s - 1;
            const float cnv = EUCLID ? pk[(long long)(tile * 32 + c) * RSP + 512] : 0.0f;
            const f32x4 *ta = (const f32x4 *)(smem + (2 + ((s - 1) & 1)) * HT_F) + c * RSH4 + h;
            f32x4 a[NG];
            mfma_prefetch<HD>(a, ta);
            if (have_prev) {
                if constexpr (WIDE_OUT) ws_store(acc, tile - 1);
                else tile_epilogue<METRIC, 512, LSE>(acc, tile - 1, h, p.K, lb);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 t = hand[j * 64 + lane];
                acc[4 * j] = t.x; acc[4 * j + 1] = t.y; acc[4 * j + 2] = t.z; acc[4 * j + 3] = t.w;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) flags[pair] = s;  // the slot may be overwritten
            mfma_range<HD, 0, 2>(acc, a, ta, xf);
            if (s < T) {
                if (s + 1 < T) dma_half(t0 + s + 1, 0, (s + 1) & 1);
                dma_half(t0 + s, 1, s & 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_range<HD, 2, NG>(acc, a, ta, xf);
            if (EUCLID && WIDE != 1) {  // (wide rows: the norms close the chain, in the last slice)
                const float a_aug = h ? cnv : 1.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
            }
        };
        __syncthreads();
        for (int s = 1; s <= T; ++s) {
            b_step(s, s > 1);
            __syncthreads();
        }
        if constexpr (WIDE_OUT) {
            if (T >= 1) ws_store(acc, t0 + T - 1);
        } else {
        if (T >= 1) tile_epilogue<METRIC, 512, LSE>(acc, t0 + T - 1, h, p.K, lb);

        float best_s;
        int best_i;
        row_winner<METRIC>(lb, h, p.K, best_s, best_i);
        if constexpr (LSE) {
            // (closed here, before the repair, which runs after the roles have joined: the NaN rule needs the repaired `best_s`
            //  and is applied there -- hence a value that is no NaN in its place)
            const float lse_v = close_lse(lb, 0.0f);  // (both lane halves: it exchanges their partial sums)
            if (h == 0 && row_ok) p.lse[(long long)head * p.M + row] = lse_v;
        }
        // The winners leave the role-specific code through this wave's own staging region: what follows (the non-finite
        // repair, the stores) is compiled after the roles have joined, where no fragment register is live any more -- with
        // the repair inside this branch the allocator put scratch reloads into the step loop.
        // (residual stacks: through the pair's hand-off slot, idle since B took the last accumulator -- the staging regions
        //  alias the dump of the non-finite protocol below)
        float *mine = MULTI ? hand_all + pair * 1024 : smem + wave * (32 * XS);
        mine[lane] = best_s;
        ((int *)mine)[64 + lane] = best_i;
        }
    }
    if constexpr (WIDE_OUT) return;  // (every wave has passed the sweep's last barrier)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (MULTI != 0) {
        // ---------------- residual stacks: winners of stage q -> next-stage residual in both waves ----------------
        volatile int *todo_sh = flags + 4;           // [4 pairs]: rows of the pair that take the non-finite repair
        float *mine = hand_all + pair * 1024;        // B's winners [64] + [64], then the repair's row buffer [512]
        float *rowbuf = mine + 256;
        float *dump = smem + pair * HT_F;            // A's halves of the flagged rows [32][256] (the tile buffers are idle)
        float best_s = 0.0f;
        int best_i = 0;
        unsigned todo = 0;
        if (role == 1) {
            best_s = mine[lane];
            best_i = ((int *)mine)[64 + lane];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            todo = nonfinite_rows(best_s, row_ok);
            if (lane == 0) todo_sh[pair] = (int)todo;
        }
        __syncthreads();
        if (role == 0) {
            todo = (unsigned)todo_sh[pair];
            if (__builtin_expect(todo != 0u, 0)) {  // the residual this stage searched IS the fragment registers: A's half -> LDS
                unsigned td = todo;
                while (td) {
                    const int rr = __builtin_ctz(td);
                    td &= td - 1;
                    if (c == rr) {
#pragma unroll
                        for (int s2 = 0; s2 < NS; ++s2) dump[rr * HD + 2 * s2 + h] = xf[s2];
                    }
                }
            }
        }
        __syncthreads();
        if (role == 1) {
            if (__builtin_expect(todo != 0u, 0)) {
                auto fill_row = [&](int rr) -> float {
                    if (c == rr) {
#pragma unroll
                        for (int s2 = 0; s2 < NS; ++s2) rowbuf[HD + 2 * s2 + h] = xf[s2];
                    }
#pragma clang loop unroll(disable)
                    for (int d = lane; d < HD; d += 64) rowbuf[d] = dump[rr * HD + d];
                    return 0.0f;
                };
                auto acc_init = [&](int, int) -> float { return 0.0f; };
                const int k1 = (t1 * 32 < p.K) ? t1 * 32 : p.K;
                repair_nonfinite_rows<METRIC, 512>(todo, rowbuf, pk, t0 * 32, k1, lane, fill_row, acc_init, best_s, best_i);
            }
            if (h == 0 && row_ok) store_winner(p, head, row, q, best_s, best_i);
            sidx[(pair * p.Q + q) * 32 + c] = best_i;
        }
        __syncthreads();  // the winners are visible to both waves; the dump is dead
        if (q + 1 < p.Q) {
            // A lane's float4 at piece 2g + h of its winner's packed HALF row is its four k-parity values of group g (the
            // half rows of a 512-dim image are the Dp = 256 layout at a 1-KiB offset): vq_search_mfma's slice gather.
            char *gb = (char *)smem + wave * (G::GWAVE_F * 4);
            const int grho = lane / G::GPP, gk = lane % G::GPP;
            int roff[G::GNI];
#pragma unroll
            for (int i = 0; i < G::GNI; ++i)
                roff[i] = sidx[(pair * p.Q + q) * 32 + i * G::GRPI + grho] * (RSP * 4) + dbase * 4 + ((gk ^ grho) * 16);
            auto gather = [&](int sl) {
#pragma unroll
                for (int i = 0; i < G::GNI; ++i)
                    lds_dma16(pk, p.pk_bytes, roff[i], sl * (G::GS * 32), (lds_f32x4 *)(gb + i * G::GIB));
            };
            const int crho = c % G::GRPI;
            const char *rbase = gb + (c / G::GRPI) * G::GIB + crho * (G::GPP * 16);
            const int wx = h ^ crho;
            // ONE update path for both roles, and no |r|^2 chain inside it (vq_search_mfma walks the chain during the update with
            // v_permlane32_swap; here that costs ~90 spilled registers): A walks its half afterwards, like B does at the start
            // of every sweep
            {
                gather(0);
#pragma unroll
                for (int sl = 0; sl < G::GNSL; ++sl) {
                    f32x4 pv[G::GS];
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                    for (int k = 0; k < G::GS; ++k) pv[k] = *(const f32x4 *)(rbase + (((2 * k) ^ wx) * 16));
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    if (sl + 1 < G::GNSL) gather(sl + 1);
#pragma unroll
                    for (int k = 0; k < G::GS; ++k)
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            float &r = xf[4 * (sl * G::GS + k) + u];
                            residual_step<METRIC, MULTI == 2>(r, pv[k][u]);
                        }
                }
            }
            if (EUCLID && role == 0) {  // A's half of the next stage's |r|^2 (d-ordered chain; B continues it from xn_a)
                const float xn = chain_from(0.0f);
                if (h == 0) xn_a[pair * 32 + c] = xn;
            }
        }
        __syncthreads();  // gather regions and hand-off slot are free again; A's chain values are visible to B
    } else
    if (role == 1) {
        float *mine = smem + wave * (32 * XS);
        float best_s = mine[lane];
        int best_i = ((int *)mine)[64 + lane];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // non-finite inputs (rare, out of line; see repair_nonfinite_rows): the whole 512-dim row from memory
        if (const unsigned todo = nonfinite_rows(best_s, row_ok); __builtin_expect(todo != 0u, 0)) {
            float *rowbuf = mine;  // (2176 floats, idle since the sweep's last barrier)
            auto fill_row = [&](int rr) -> float { return fill_row_from_memory<METRIC, 512, XT, WIDE>(p, head, row0 + rr, rowbuf, lane); };
            auto acc_init = [&](int rr, int k) -> float {
                if constexpr (WIDE == 2) return wide_acc_init(p, head, (long long)blockIdx.x * 4 + pair, rr, k);
                return 0.0f;
            };
            const int k1 = (t1 * 32 < p.K) ? t1 * 32 : p.K;
            repair_nonfinite_rows<METRIC, 512>(todo, rowbuf, pk, t0 * 32, k1, lane, fill_row, acc_init, best_s, best_i);
            if constexpr (LSE) {
                if (best_s != best_s && h == 0 && row_ok) p.lse[(long long)head * p.M + row] = best_s;  // logsumexp of a row with a NaN
            }
        }
        if (p.mode != kModeFused) {
            if (h == 0 && row_ok) store_key<METRIC>(p, head, row, best_s, best_i);
        } else {
            if (h == 0 && row_ok) store_winner(p, head, row, 0, best_s, best_i);
            sidx[pair * 32 + c] = best_i;
        }
    }
    }  // stages
    STAMP(2);
    if (p.mode != kModeFused) return;

    __builtin_amdgcn_s_setprio(2);
    if (p.out == nullptr && p.loss_part == nullptr) return;
    __syncthreads();  // the last stage's winners (written by the B waves) are visible to the A waves
    if constexpr (WIDE == 2) {  // (each wave of a pair takes 16 rows)
        const int prow = (p.M - row0 >= 32) ? 32 : (p.M - row0 > 0 ? (int)(p.M - row0) : 0);
        const int lo = role * 16, hi = (lo + 16 < prow) ? lo + 16 : prow;
        gather_wide_rows(p, head, row0, lo, hi, sidx + pair * 32, lane);
        return;
    }

    // ---------------- fused finalize (natural layout): each wave of a pair takes 16 of the pair's 32 rows ----------------
    const bool need_r = p.ste || p.loss_part;
    float *lerr = smem + (wave * p.Q) * 64 + lane;  // [8][Q][64], MULTI with loss only: in the tile buffers (idle; Q <= 64)
    if (MULTI && p.loss_part)
        for (int q = 0; q < p.Q; ++q) lerr[q * 64] = 0.0f;
    float e0 = 0.0f;
    const float *cbh = p.cb + (long long)head * p.cb_hs;
    float *outh = p.out ? p.out + (long long)head * p.out_hs : nullptr;
    const int pair_rows = (p.M - row0 >= 32) ? 32 : (p.M - row0 > 0 ? (int)(p.M - row0) : 0);
    const int r_lo = role * 16, r_hi = (r_lo + 16 < pair_rows) ? r_lo + 16 : pair_rows;  // this wave's rows [r_lo, r_hi)
    const int nq = MULTI ? p.Q : 1;
    if (p.vec_fin) {
        constexpr int RB = 4;
        for (int rr0 = r_lo; rr0 < r_hi; rr0 += RB) {
            f32x4 r[RB][2], o[RB][2];
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const int rr = (rr0 + k < r_hi) ? rr0 + k : r_hi - 1;
                const float *xr = xh + (row0 + rr) * p.x_rs;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int d = 4 * (lane + 64 * j);
                    o[k][j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                    r[k][j] = o[k][j];
                    if (need_r && d < p.D) r[k][j] = *(const f32x4 *)(xr + d);
                }
            }
            constexpr int QB = 4;
            for (int q0 = 0; q0 < nq; q0 += QB) {
                f32x4 cv[QB][RB][2];
#pragma unroll
                for (int kq = 0; kq < QB; ++kq) {
                    if (q0 + kq < nq) {
#pragma unroll
                        for (int k = 0; k < RB; ++k) {
                            const int rr = (rr0 + k < r_hi) ? rr0 + k : r_hi - 1;
                            const int i = sidx[(pair * p.Q + q0 + kq) * 32 + rr];
                            const float *crow = cbh + (long long)(q0 + kq) * p.cb_qs + (long long)i * p.D;
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const int d = 4 * (lane + 64 * j);
                                cv[kq][k][j] = (d < p.D) ? *(const f32x4 *)(crow + d) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                            }
                        }
                    }
                }
#pragma unroll
                for (int kq = 0; kq < QB; ++kq) {
                    if (q0 + kq < nq) {
                        float e = 0.0f;
#pragma unroll
                        for (int k = 0; k < RB; ++k) {
                            const bool live = rr0 + k < r_hi;
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                f32x4 quant = cv[kq][k][j];
                                if (need_r) {
                                    const f32x4 diff = cv[kq][k][j] - r[k][j];
                                    if (live) {
                                        e = fmaf(diff.x, diff.x, e);
                                        e = fmaf(diff.y, diff.y, e);
                                        e = fmaf(diff.z, diff.z, e);
                                        e = fmaf(diff.w, diff.w, e);
                                    }
                                    if (p.ste) quant = r[k][j] + diff;
                                    r[k][j] = r[k][j] - quant;
                                }
                                o[k][j] = o[k][j] + quant;
                            }
                        }
                        if (MULTI) {
                            if (p.loss_part) lerr[(q0 + kq) * 64] += e;
                        } else {
                            e0 += e;
                        }
                    }
                }
            }
            if (outh) {
#pragma unroll
                for (int k = 0; k < RB; ++k) {
                    if (rr0 + k < r_hi) {
                        float *orow = outh + (row0 + rr0 + k) * p.out_rs;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int d = 4 * (lane + 64 * j);
                            if (d < p.D) __builtin_nontemporal_store(o[k][j], (f32x4 *)(orow + d));
                        }
                    }
                }
            }
        }
    } else {
        for (int rr = r_lo; rr < r_hi; ++rr) {
            const long long grow = row0 + rr;
            const float *xr = xh + grow * p.x_rs;
            float *orow = outh ? outh + grow * p.out_rs : nullptr;
            float r[8], o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = lane + 64 * j;
                o[j] = 0.0f;
                r[j] = (need_r && d < p.D) ? xr[d] : 0.0f;
            }
            for (int q = 0; q < nq; ++q) {
                const int i = sidx[(pair * p.Q + q) * 32 + rr];
                const float *crow = cbh + (long long)q * p.cb_qs + (long long)i * p.D;
                float e = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int d = lane + 64 * j;
                    if (d < p.D) {
                        const float cv = crow[d];
                        float quant = cv;
                        if (need_r) {
                            const float diff = cv - r[j];
                            e = fmaf(diff, diff, e);
                            if (p.ste) quant = r[j] + diff;
                            r[j] = r[j] - quant;
                        }
                        o[j] = o[j] + quant;
                    }
                }
                if (MULTI) {
                    if (p.loss_part) lerr[q * 64] += e;
                } else {
                    e0 += e;
                }
            }
            if (orow) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int d = lane + 64 * j;
                    if (d < p.D) orow[d] = o[j];
                }
            }
        }
    }
    if (p.loss_part) store_loss_partials<WAVES, MULTI != 0>(p, head, lerr, e0, wave, lane);
    STAMP(3);
    STAMP_RT(61);
}
