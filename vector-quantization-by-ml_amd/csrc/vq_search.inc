// vq_search.inc -- the hot kernel: MFMA nearest-codebook search with fused finalize.  Included by vq_kernels.hip.
// ------------------------------------------------------------------------------------------------
// search kernel
// ------------------------------------------------------------------------------------------------
}  // namespace
namespace vqi {
struct SearchParams {
    const float *x;
    long long x_rs, x_hs;
    const float *cb;
    long long cb_hs, cb_qs;
    const float *packed;
    long long pk_hs, pk_qs;
    float *out;
    long long out_rs, out_hs;
    long long *idx;
    long long idx_rs, idx_hs, idx_qs;
    float *best;
    float *loss_part;  // [H * gridDim.x * WAVES][Q] or NULL
    long long *keys;   // kModeKeys
    long long idx_offset;
    long long M;
    int K, D, Q;
    int ntiles, tiles_per_split;
    unsigned pk_bytes;  // bytes of one packed image (buffer descriptor range)
    int mode;
    int ste;
    int vec_x;    // x rows may be read as float4 (D % 4 == 0, strides % 4 == 0, 16-B aligned base)
    int vec_fin;  // finalize may use float4 on x / out / cb
    float *lse;   // [H * M] log-sum-exp of the similarities (LSE kernel variant) or NULL
    int xt;       // element type of x: 0 fp32, 1 fp16, 2 bf16 (2-byte types: inference only, strides in elements)
    long long key_hs;  // keys of head h start at keys + h * key_hs (= M unless the launch covers a row chunk)
    long long key_zs;  // kModeKeyParts: K split z (blockIdx.z) stores into plane z, planes key_zs apart
    int res_img_floats;  // > 0: the resident-codebook kernel (vq_search_resident.inc) with this many floats of image in LDS
    int res_skew;        // that kernel: waves 4..7 start this many s_sleep(127) later (diagnostic; 0)
    int res_nbuf;        // that kernel: slab buffers per wave (slabs per row, or 1 when LDS is short)
    // rows wider than 512 dims (WIDE kernels): the distance chain is carried from one slice's launch to the next through
    // `acc_ws`, in the accumulators' own fragment layout: float4 [head][row block of 32][sub-tile][r / 4][lane]
    float *acc_ws;
    long long ws_hs;   // float4 per head
    int ws_nsub;       // sub-tiles per row block in acc_ws
    int acc_in;        // continue the chains stored in acc_ws / xn_ws (not the first slice)
    float *sims;         // WIDE = 3: the similarity matrix of this (row chunk, code chunk), element (h, m, k) at sims[h*sims_hs + m*sims_rs + k]
    long long sims_rs, sims_hs;
    int vec_s;           // float4 stores into sims are aligned
    int fin_D;           // WIDE = 2 in fused mode: dims of a whole row (the slice's own width is D)
    const float *xn_ws;  // [head][xn_hs]: |x|^2 chain over the dims of the earlier slices
    float *xn_out;       // the chain including this slice (another buffer: the workgroups of a K split share the rows)
    long long xn_hs;
    // Dp = 256 screened sweep (vq_search_persist.inc, SCREEN): the fp16 screen image of every head, `scr_hs` bytes apart, each
    // `scr_bytes` long (NULL: the fp32 sweep)
    const float *scr;
    long long scr_hs;
    unsigned scr_bytes;
    // rows the screen cannot bound, as entries head * M + row in `scr_list` (room for all H M rows), behind the images:
    // scr_count[0] rows to search in full from the front, scr_count[1] rows to rescore (candidate codes in their idx element)
    // from the back; both counts are zeroed by vq_pack_scr_kernel, the entries are decided by vq_resolve_rows_kernel
    unsigned *scr_count;
    unsigned *scr_list;
    // that sweep: waves 4..7 fold the previous sub-tile's values in half a sub-tile after their SIMD partners 0..3 (0: all
    // eight waves right after the first MFMA group; the results are the same bit for bit)
    int scr_stagger;
};
}  // namespace vqi
namespace {
using vqi::SearchParams;

typedef __attribute__((address_space(3))) f32x4 lds_f32x4;


#ifdef VQ_EXP_STAMPS
#define VQ_NSTAMP 64
__device__ unsigned long long g_stamps[8192 * VQ_NSTAMP];
#define STAMP(i) do { if (lane == 0 && (i) < VQ_NSTAMP) g_stamps[(((long long)blockIdx.x * WAVES + wave) & 8191) * VQ_NSTAMP + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
// constant-rate (100 MHz) counter beside the shader-clock one: their ratio over a wave's life is the clock it ran at
#define STAMP_RT(i) do { if (lane == 0) g_stamps[(((long long)blockIdx.x * WAVES + wave) & 8191) * VQ_NSTAMP + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define STAMP(i) do { } while (0)
#define STAMP_RT(i) do { } while (0)
#endif

// buffer_load_dwordx4 ... lds: `base` + voffset (per lane) + soffset (scalar) -> LDS at l + lane * 16
__device__ __forceinline__ void lds_dma16(const float *base, unsigned bytes, int voffset, int soffset, lds_f32x4 *l) {
#if defined(__HIP_DEVICE_COMPILE__)
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)l, 16, voffset, soffset, 0, 0);
#else
    (void)base; (void)bytes; (void)voffset; (void)soffset; (void)l;
#endif
}

template <int DP, int WAVES>
struct Geo {
    static constexpr int RS = DP + 4;                       // packed row stride, floats
    static constexpr int RS4 = RS / 4;
    static constexpr int SUB = sub_tiles(DP);               // 32-code MFMA sub-tiles per staged tile / barrier
    static constexpr int TILE_CODES = kTileCodes * SUB;
    static constexpr int TILE_F4 = TILE_CODES * RS / 4;     // float4 per staged tile image
    static constexpr int TILE_CHUNKS = (TILE_F4 + 63) / 64; // 1-KiB wave copies per tile (over-copy)
    static constexpr int BUF_F4 = TILE_CHUNKS * 64;
    static constexpr int CH = DP < 64 ? DP : 64;            // prologue column chunk
    static constexpr int XS = CH + 4;                       // prologue scratch row stride, floats (16-B rows)
    static constexpr int NS = DP / 2;                       // MFMA k-steps
    static constexpr int NBUF = 2;
    static constexpr int MAIN_FLOATS = (NBUF * BUF_F4 * 4 > WAVES * 32 * XS) ? NBUF * BUF_F4 * 4 : WAVES * 32 * XS;
    static constexpr int NCH4 = DP >= 256 ? DP / 256 : 1;   // float4 chunks per lane in finalize
    static constexpr int NEL = DP >= 64 ? DP / 64 : 1;      // scalars per lane in finalize
    // Residual stages: the winners' packed rows are gathered slice by slice through a wave-private LDS region that
    // aliases the (idle) tile buffers.  A slice = GS groups of 8 dims = GPP 16-B pieces per row; one LDS-DMA instruction
    // copies that slice of GRPI rows (64 lanes x 16 B, contiguous per row: whole cache lines, unlike a per-lane gather).
    static constexpr int GS = DP / 8 < 8 ? DP / 8 : 8;      // groups of 8 dims per slice
    static constexpr int GPP = 2 * GS;                      // 16-B pieces per row and slice (even / odd k-parity halves)
    static constexpr int GRPI = 64 / GPP;                   // rows per DMA instruction
    static constexpr int GNI = 32 / GRPI;                   // DMA instructions per slice (a wave owns 32 rows)
    static constexpr int GNSL = DP / 8 / GS;                // slices
    static constexpr int GIB = 1024 + 64;                   // LDS bytes per instruction block; the 64-B pad rotates the banks
    static constexpr int GWAVE_F = GNI * GIB / 4;           // floats of gather region per wave
    static constexpr int MAIN_FLOATS_M = MAIN_FLOATS > WAVES * GWAVE_F ? MAIN_FLOATS : WAVES * GWAVE_F;  // MULTI kernels
    // Single-stage kernels that run ONE 8-wave workgroup per CU anyway (Dp = 256: 219 VGPRs) have LDS to spare: the prologue
    // stages the rows BEHIND the tile buffers instead of inside them, so the first codebook tile can be on its way before the
    // rows are even loaded (the sweep otherwise starts with one exposed DMA latency per row block: ~6 k cycles, 1 % at K = 1024)
    static constexpr bool SEP_STAGE = (DP == 256 && WAVES == 8);
    static constexpr int MAIN_FLOATS_S = SEP_STAGE ? NBUF * BUF_F4 * 4 + WAVES * 32 * XS : MAIN_FLOATS;  // MULTI == 0 kernels
};

// LDS-DMA of one packed tile image into the tile buffer `dst`: buffer_load ... lds with the per-lane part (lane * 16 B) in
// voffset and the tile / chunk position in the SCALAR offset -> no vector instructions at all per issue (on gfx950 VALU
// work is not free beside f32 MFMA: it executes on the same lanes).  The 1-KiB chunks go round the workgroup's waves.
// Used by the kernels whose register allocation it leaves as it was (vq_search_persist, vq_ce_backward_roles); the other
// sweeps spell the same loop out in a `stage` lambda (profiles/prologue_refactor_codegen.md has the figures).
template <typename G, int WAVES>
__device__ __forceinline__ void stage_tile(const float *img, unsigned bytes, int tile, lds_f32x4 *dst, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < (G::TILE_CHUNKS + WAVES - 1) / WAVES; ++i) {
        const int ck = i * WAVES + wave;
        if (ck < G::TILE_CHUNKS) lds_dma16(img, bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16, dst + ck * 64);
    }
}

// ---- prologue of the fp32 MFMA sweeps: a wave's 32 rows -> B fragments in registers --------------------------------------
// xf[s] = x[row0 + c][2 s + h] for the NCHUNK * CH dims from `x` on: lane half h holds the k = h operand of MFMA step s of
// v_mfma_f32_32x32x2_f32.  Rows past M repeat row M - 1, dims past D are zeros.  The rows go through the wave-private LDS
// region number `region` of `stage` ([32][XS] floats each; no workgroup barriers: a wave's LDS operations execute in order)
// CH dims at a time, the global loads of chunk i + 1 in flight while chunk i goes through LDS.  On the way every lane extends
// xn0 = |x|^2 of its row c (both lane halves read the same row): the d-ordered fmaf chain of oracle/vq_oracle.c
// (sumsq_chain), continued from the value the caller passes in (0, or the chain over the dims in front of these) -- when
// EUCLID and `walk_chain`.
// `x` points at dim 0 of the head's first row -- a wave that owns the dims from d on passes x + d and D - d; `vec_x`: rows may
// be read as float4.  No barrier at the end: the caller knows whether the region is about to be reused by other waves.
// Shared by the similarity / softmax-statistics / sampling sweeps, the cross-entropy backward kernels and the Gumbel sweeps.
// The three inference search kernels (vq_search_mfma below, vq_search_pair512, vq_search_persist) keep this body written out
// in place, with their own variations (fp16 / bf16 rows, non-temporal loads, the screened sweep's fp16 pairing): routed
// through this function their VGPR / AGPR counts move (profiles/prologue_refactor_codegen.md), and those kernels are tuned
// to their register budgets.  A change to the chain or the swaps has to be made in all four places.
template <int CH, int XS, int NCHUNK, bool EUCLID>
__device__ __forceinline__ void load_x_fragments(const float *x, long long x_rs, long long M, int D, int vec_x, long long row0,
                                                 bool walk_chain, float *stage, int region, int lane,
                                                 float (&xf)[NCHUNK * CH / 2], float &xn0) {
    constexpr int LPL = CH / 8;  // float4 loads per lane per chunk
    const int c = lane & 31, h = lane >> 5;
    float *xs = stage + region * (32 * XS);
    f32x4 v[2][LPL];
    auto load_chunk = [&](int ch, f32x4 (&dst)[LPL]) {
#pragma unroll
        for (int it = 0; it < LPL; ++it) {
            const int f = it * 64 + lane;
            const int r = f / (CH / 4), c4 = f % (CH / 4);
            long long grow = row0 + r;
            if (grow >= M) grow = M - 1;
            const int d0 = ch * CH + c4 * 4;
            f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
            const float *src = x + grow * x_rs + d0;
            if (vec_x) {
                if (d0 < D) t = *(const f32x4 *)src;
            } else {
                if (d0 + 0 < D) t.x = src[0];
                if (d0 + 1 < D) t.y = src[1];
                if (d0 + 2 < D) t.z = src[2];
                if (d0 + 3 < D) t.w = src[3];
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
            *(f32x4 *)(xs + r * XS + c4 * 4) = v[ch & 1][it];  // XS = 4 mod 8: b128 accesses conflict-free
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const float *rp = xs + c * XS;  // this lane's row
#pragma unroll
        for (int j = 0; j < CH / 8; ++j) {
            const f32x4 lo = *(const f32x4 *)(rp + 8 * j);
            const f32x4 hi = *(const f32x4 *)(rp + 8 * j + 4);
            if (EUCLID && walk_chain) {
                xn0 = fmaf(lo.x, lo.x, xn0);
                xn0 = fmaf(lo.y, lo.y, xn0);
                xn0 = fmaf(lo.z, lo.z, xn0);
                xn0 = fmaf(lo.w, lo.w, xn0);
                xn0 = fmaf(hi.x, hi.x, xn0);
                xn0 = fmaf(hi.y, hi.y, xn0);
                xn0 = fmaf(hi.z, hi.z, xn0);
                xn0 = fmaf(hi.w, hi.w, xn0);
                asm volatile("" : "+v"(xn0));  // pin the chain here: do not keep lo/hi alive to finish it later
            }
            // lower half-wave keeps dims 8j..8j+3, upper 8j+4..8j+7; two half-wave exchanges de-interleave
            // them into the MFMA k-parity layout: lower gets the even dims, upper the odd dims.
            const f32x4 m = h ? hi : lo;
            const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(m.x), __float_as_uint(m.y), false, false);
            const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m.z), __float_as_uint(m.w), false, false);
            const int sb = ch * (CH / 2) + 4 * j;
            xf[sb + 0] = __uint_as_float(xy[0]);  // dim 8j + 0 + h
            xf[sb + 1] = __uint_as_float(zw[0]);  // dim 8j + 2 + h
            xf[sb + 2] = __uint_as_float(xy[1]);  // dim 8j + 4 + h
            xf[sb + 3] = __uint_as_float(zw[1]);  // dim 8j + 6 + h
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next chunk overwrites
    }
}

// code fragments: one ds_read_b128 feeds 4 MFMAs (256 cycles of matrix pipe).  `a` is the whole tile's fragment
// array (compile-time indexed -> registers); reads run PF groups ahead of the MFMAs and the order is pinned so the
// scheduler cannot hoist every read to the top (register pressure).  Groups [G0, G1) of 8 dims.
template <int DP>
struct FragPipe {
    static constexpr int NG = DP / 8;
    static constexpr int PF = NG < 3 ? NG : 3;
};

template <int V>
struct IntC {
    static constexpr int value = V;
};

template <int DP>
__device__ __forceinline__ void mfma_prefetch(f32x4 (&a)[DP / 8], const f32x4 *ta) {
#pragma unroll
    for (int g = 0; g < FragPipe<DP>::PF; ++g) a[g] = ta[2 * g];
}

template <int DP, int G0, int G1>
__device__ __forceinline__ void mfma_range(f32x16 &acc, f32x4 (&a)[DP / 8], const f32x4 *ta, const float (&xf)[DP / 2]) {
    constexpr int NG = FragPipe<DP>::NG, PF = FragPipe<DP>::PF;
#pragma unroll
    for (int g = G0; g < G1; ++g) {
        if (g + PF < NG) a[g + PF] = ta[2 * (g + PF)];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].x, xf[4 * g + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].y, xf[4 * g + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].z, xf[4 * g + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].w, xf[4 * g + 3], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// End of a 32-code tile for one wave: augmented-column MFMA (Euclid), tail masking, in-lane reduction.
// A lane holds 16 codes of ONE row: acc[r] <-> code t*32 + 4*h + (r&3) + 8*(r>>2), ascending in r.
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float o;  // raw instruction: no canonicalising v_max in front (MFMA outputs are already canonical)
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
    return o;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float o;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
    return o;
}

// Per-lane running state of the argmin over the codes a lane has seen (16 per 32-code sub-tile, ascending).
// `pend` parks the 16 values of the sub-tile that produced the current record low; the expensive part of the
// tie-exact rule (correctly rounded sqrt, rounding-band threshold, lowest index inside the band) is resolved ONCE at
// the end of the sweep instead of on every record (with 64 lanes x few tiles some lane sets a record on nearly every
// tile, and on gfx950 those vector instructions are not hidden behind the f32 MFMA stream).
struct LaneBest {
    float best_t;   // Euclid: min clamped squared distance so far; dot: max similarity so far
    int pend_u;     // sub-tile that produced it
    f32x16 pend;    // its 16 values
    float run_m, run_s;  // LSE variant only: running max (log2 units) and sum of exp2(logit - run_m) over the codes seen
};

// LSE variant of the epilogue: online softmax over the 16 similarities a lane holds (logit = similarity), reusing the
// sub-tile extreme `tm` the argmin already computed as the running-max candidate.  Native sqrt / exp2 (1e-6 relative).
template <int METRIC>
__device__ __forceinline__ void lse_update(const f32x16 &acc, float tm, LaneBest &st) {
    constexpr float LOG2E = 1.4426950408889634f;
    const float NINF = -__builtin_inff();
    const float mx2 = (METRIC == VQ_METRIC_EUCLID) ? -__builtin_amdgcn_sqrtf(tm) * LOG2E : tm * LOG2E;
    if (mx2 > st.run_m) {
        st.run_s *= __builtin_amdgcn_exp2f(st.run_m - mx2);  // exp2(-inf) = 0 on the first visit
        st.run_m = mx2;
    }
    if (st.run_m > NINF) {
        const f32x2 nm = {-st.run_m, -st.run_m};
        f32x2 s2 = {0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            f32x2 e;
            if (METRIC == VQ_METRIC_EUCLID) {
                const f32x2 d = {__builtin_amdgcn_sqrtf(vmax3(acc[r], 0.0f, 0.0f)), __builtin_amdgcn_sqrtf(vmax3(acc[r + 1], 0.0f, 0.0f))};
                e = __builtin_elementwise_fma(d, (f32x2){-LOG2E, -LOG2E}, nm);
            } else {
                e = __builtin_elementwise_fma((f32x2){acc[r], acc[r + 1]}, (f32x2){LOG2E, LOG2E}, nm);
            }
            s2 += (f32x2){__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};  // masked codes: exp2(-inf) = 0
        }
        st.run_s += s2.x + s2.y;
    }
}

__device__ __forceinline__ float rounding_band_hi(float sq) {
    // largest fp32 t whose correctly rounded sqrt is still `sq`:  t < (sq + ulp(sq)/2)^2, exact in fp64
    const float up = __uint_as_float(__float_as_uint(sq) + 1u);  // next float above (sq >= 0)
    const double mid = (double)sq + 0.5 * ((double)up - (double)sq);
    const double lim = mid * mid;
    float hi = (float)lim;
    if ((double)hi >= lim) hi = __uint_as_float(__float_as_uint(hi) - 1u);
    return hi;
}

// End of a 32-code sub-tile for one wave: in-lane reduction of the 32x32 result (`acc` already tail-masked if needed).
// A lane holds 16 codes of ONE row: acc[r] <-> code u*32 + 4*h + (r&3) + 8*(r>>2), ascending in r.
template <int METRIC, bool LSE>
__device__ __forceinline__ void reduce_and_record(const f32x16 &acc, int u, LaneBest &st) {
    if (METRIC == VQ_METRIC_EUCLID) {
        // min over the 16 values, clamped at 0 (clamp_min_(0) commutes with min): ONE asm block, so the compiler neither
        // pads the dependent chain with s_nop nor canonicalises the operands (MFMA outputs are canonical already)
        float tm;
        asm("v_min3_f32 %0, %1, %2, %3\n\t"
            "v_min3_f32 %0, %0, %4, %5\n\t"
            "v_min3_f32 %0, %0, %6, %7\n\t"
            "v_min3_f32 %0, %0, %8, %9\n\t"
            "v_min3_f32 %0, %0, %10, %11\n\t"
            "v_min3_f32 %0, %0, %12, %13\n\t"
            "v_min3_f32 %0, %0, %14, %15\n\t"
            "v_min_f32 %0, %0, %16"
            : "=&v"(tm)
            : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]),
              "v"(acc[8]), "v"(acc[9]), "v"(acc[10]), "v"(acc[11]), "v"(acc[12]), "v"(acc[13]), "v"(acc[14]), "v"(acc[15]));
        if constexpr (LSE) lse_update<METRIC>(acc, vmax3(tm, 0.0f, 0.0f), st);
        if (tm < st.best_t) {
            // The clamp at 0 (clamp_min_(0) commutes with min) is only needed once a value gets this far: best_t >= 0, so
            // an unclamped tm below it is either a real candidate or a negative rounding residue that clamps to 0.
            // (It must not run before the compare: v_max3 turns the NaN of a non-finite row into 0, a "winner" that would
            //  hide the row from the non-finite repair.)
            tm = vmax3(tm, 0.0f, 0.0f);
            // A new record low of the squared distance.  It replaces the parked sub-tile unless its sqrt ROUNDS to the
            // same value as the parked minimum's (then the earlier sub-tile keeps the win: lower codes).  Two values
            // more than 2^-21 apart (relative) cannot share a rounded sqrt, so only near-ties pay for the two sqrts.
            bool take = true;
            if (tm * 1.0000004768371582f >= st.best_t) take = sqrtf(tm) < sqrtf(st.best_t);
            if (take) {
                st.best_t = tm;
                st.pend_u = u;
                st.pend = acc;
            }
        }
    } else {
        float tm;
        asm("v_max3_f32 %0, %1, %2, %3\n\t"
            "v_max3_f32 %0, %0, %4, %5\n\t"
            "v_max3_f32 %0, %0, %6, %7\n\t"
            "v_max3_f32 %0, %0, %8, %9\n\t"
            "v_max3_f32 %0, %0, %10, %11\n\t"
            "v_max3_f32 %0, %0, %12, %13\n\t"
            "v_max3_f32 %0, %0, %14, %15\n\t"
            "v_max_f32 %0, %0, %16"
            : "=&v"(tm)
            : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]),
              "v"(acc[8]), "v"(acc[9]), "v"(acc[10]), "v"(acc[11]), "v"(acc[12]), "v"(acc[13]), "v"(acc[14]), "v"(acc[15]));
        if constexpr (LSE) lse_update<METRIC>(acc, tm, st);
        if (tm > st.best_t) {  // strictly better than everything earlier
            st.best_t = tm;
            st.pend_u = u;
            st.pend = acc;
        }
    }
}

// Tail masking happens on a COPY inside the rare branch: the common path reduces the accumulator registers where they
// are (merging a masked and an unmasked value set at a join made the compiler copy all 16 registers on every sub-tile).
template <int METRIC, int DP, bool LSE = false>
__device__ __forceinline__ void tile_epilogue(const f32x16 &acc, int u, int h, int K, LaneBest &st) {
    // Euclid needs no masking at all: the packed image gives every padding row |c|^2 = +inf (vq_pack.inc), so its distance
    // is +inf and can neither win nor tie (and contributes exp2(-inf) = 0 to the LSE).  Only the dot metric, whose padding
    // rows score 0, masks the codebook's tail.
    if (METRIC != VQ_METRIC_EUCLID && u * kTileCodes + kTileCodes > K) {
        const float worst = (METRIC == VQ_METRIC_EUCLID) ? __builtin_inff() : -__builtin_inff();
        const int cbase = u * kTileCodes + 4 * h;
        f32x16 m = acc;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (cbase + (r & 3) + 8 * (r >> 2) >= K) m[r] = worst;
        reduce_and_record<METRIC, LSE>(m, u, st);
    } else {
        reduce_and_record<METRIC, LSE>(acc, u, st);
    }
}

// End of a sweep: turn the parked sub-tile into (value in the compared space, lowest winning code of this lane).
template <int METRIC>
__device__ __forceinline__ void resolve_best(const LaneBest &st, int h, int K, float &best_s, int &best_i) {
    int bi = 0;
    if (METRIC == VQ_METRIC_EUCLID) {
        best_s = sqrtf(st.best_t);  // correctly rounded; +inf if the lane saw no finite distance
        const float hi = (st.best_t < __builtin_inff()) ? rounding_band_hi(best_s) : __builtin_inff();
#pragma unroll
        for (int r = 15; r >= 0; --r) bi = (st.pend[r] <= hi) ? (r & 3) + 8 * (r >> 2) : bi;  // unclamped: t < 0 -> 0 <= hi
    } else {
        best_s = st.best_t;
#pragma unroll
        for (int r = 15; r >= 0; --r) bi = (st.pend[r] == st.best_t) ? (r & 3) + 8 * (r >> 2) : bi;
    }
    best_i = st.pend_u * kTileCodes + 4 * h + bi;
    // Euclid does not mask the padding rows (their distance is +inf); a row of non-finite inputs -- outside the arithmetic
    // contract -- could still park one of them, and the index must stay inside the codebook whatever the row holds
    if (METRIC == VQ_METRIC_EUCLID) best_i = best_i < K ? best_i : K - 1;
}

// ---- non-finite inputs ----------------------------------------------------------------------------------------------
// ATen's argmax (utils/general.py:128 over codebooks.py:128-129,386) treats NaN as the maximum and returns the FIRST one;
// clamp_min_ and sqrt propagate NaN.  The sweep's reduction cannot follow that rule (v_min3 / v_max3 return the non-NaN
// operand), so the rows it may have got wrong are searched again here, out of line, by the plain rule:
//   * a row holding a NaN or an inf: every one of its distances is NaN or +inf (|x|^2 is), so the sweep's winner is not
//     finite -- that is the trigger, it costs one compare per row and sweep;
//   * a codebook holding a non-finite value (flagged once by vq_pack_flag_kernel): every row -- a code with a NaN wins
//     EVERY row, a code with an inf the rows on one side of it.
// One row at a time: the row goes to wave-private LDS (`rowbuf`, >= Dp floats; `fill_row(rr)` writes it, zero padded, and
// returns the start of its |x|^2 chain), the 64 lanes stride over the codes [k0, k1) of the packed image and each runs
// the k-ordered chain of oracle/vq_oracle.c on its code (`acc_init(rr, k)` = the chain's start: 0, or the earlier slices'
// value for wide rows), keeps its first NaN / else its first minimum, and a 6-step butterfly picks the wave's winner
// (NaN first, then value, then index).  Finite inputs whose products overflow inside a chain are outside the contract
// (ATen's own result then depends on MKL's summation order).
template <int METRIC, int DP, typename FillRow, typename AccInit>
__device__ __forceinline__ void repair_nonfinite_rows(unsigned todo, float *rowbuf, const float *pk, int k0, int k1, int lane,
                                                      FillRow fill_row, AccInit acc_init, float &best_s, int &best_i) {
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    constexpr int RS = DP + 4;
    const int c = lane & 31;
    while (todo) {
        const int rr = __builtin_ctz(todo);  // wave-uniform
        todo &= todo - 1;
        float xn = fill_row(rr);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (EUCLID) {
#pragma clang loop unroll(disable)
            for (int d = 0; d < DP; ++d) xn = fmaf(rowbuf[d], rowbuf[d], xn);  // d-ordered chain (the padding adds +0)
        }
        float bv = EUCLID ? __builtin_inff() : -__builtin_inff();
        int bi = (k0 + lane < k1) ? k0 + lane : 0x7FFFFFFF;  // nothing better than the start value: the lowest code
        bool bn = false;
        // (rolled loops on purpose: this path must stay small -- it sits behind the sweep of kernels that live at the edge
        //  of their register budget)
#pragma clang loop unroll(disable)
        for (int k = k0 + lane; k < k1; k += 64) {
            const float *prow = pk + (long long)k * RS;
            float acc = acc_init(rr, k);
#pragma clang loop unroll(disable)
            for (int g = 0; g < DP / 8; ++g) {
                const f32x4 ev = *(const f32x4 *)(prow + 8 * g), od = *(const f32x4 *)(prow + 8 * g + 4);
                const f32x4 xa = *(const f32x4 *)(rowbuf + 8 * g), xb = *(const f32x4 *)(rowbuf + 8 * g + 4);
                acc = fmaf(xa.x, ev.x, acc);
                acc = fmaf(xa.y, od.x, acc);
                acc = fmaf(xa.z, ev.y, acc);
                acc = fmaf(xa.w, od.y, acc);
                acc = fmaf(xb.x, ev.z, acc);
                acc = fmaf(xb.y, od.z, acc);
                acc = fmaf(xb.z, ev.w, acc);
                acc = fmaf(xb.w, od.w, acc);
            }
            float s = acc;
            if (EUCLID) {
                float t = fmaf(1.0f, xn, acc);
                t = fmaf(prow[DP], 1.0f, t);
                t = (t < 0.0f) ? 0.0f : t;  // clamp_min_(0): keeps NaN
                s = sqrtf(t);
            }
            if (!bn) {
                if (s != s) {
                    bn = true;
                    bv = s;
                    bi = k;
                } else if (EUCLID ? (s < bv) : (s > bv)) {
                    bv = s;
                    bi = k;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int on = __shfl_xor((int)bn, o);
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            bool take;
            if (on != (int)bn) take = on != 0;
            else if (bn) take = oi < bi;
            else take = (EUCLID ? (ov < bv) : (ov > bv)) || (ov == bv && oi < bi);
            if (take) {
                bn = on != 0;
                bv = ov;
                bi = oi;
            }
        }
        if (c == rr) {
            best_s = bv;
            best_i = bi;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the row buffer is rewritten by the next row
    }
}

// The "codebook holds a non-finite value" word of a packed image (vq_pack_flag_kernel): the last 16 bytes of the image,
// `pk_bytes` = the bytes from `pk` to the image's end (what the tile DMA's buffer descriptor uses).
__device__ __forceinline__ unsigned codebook_flag(const float *pk, unsigned pk_bytes) {
    return ((const unsigned *)pk)[pk_bytes / 4 - 4];
}

// A flagged codebook sends EVERY row through the repair.  Nothing stays live across the sweep for that: the sweep starts
// from a record value no candidate can beat (Euclid -inf, dot +inf), so it parks nothing and its "winner" comes out non-finite
// (sqrt(-inf) = NaN, resp. +inf) -- the same trigger a non-finite row pulls.
template <int METRIC>
__device__ __forceinline__ float sweep_start_value(unsigned cb_flag) {
    const float INF = __builtin_inff();
    if (METRIC == VQ_METRIC_EUCLID) return cb_flag ? -INF : INF;
    return cb_flag ? INF : -INF;
}

// A lane's state at the start of a sweep: nothing parked yet (Euclid: pend[0] <= +inf still selects code 0), `best_t` = the
// record every candidate has to beat (sweep_start_value, or +inf for the screened sweep)
template <int METRIC>
__device__ __forceinline__ LaneBest lane_best_start(float best_t) {
    const float INF = __builtin_inff();
    LaneBest lb;
    lb.best_t = best_t;
    lb.pend_u = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) lb.pend[r] = (METRIC == VQ_METRIC_EUCLID) ? INF : -INF;
    lb.run_m = -INF;
    lb.run_s = 0.0f;
    return lb;
}

// Similarities of sub-tile u leave for memory (the WIDE = 3 variants of vq_search_mfma and vq_search_pair512): a lane holds
// codes u*32 + 4h + 8g + (0..3) of ITS row (`srow`) -> one float4 per g.  sim = -sqrt(max(0, t)) (Euclid; correctly rounded,
// like the values the search compares, and it keeps NaN) / x.c (dot): codebooks.py:386,435.  `vec_s`: float4 stores are
// aligned (then K % 4 == 0).
// (Scalar arguments by reference, as the lambdas this replaces captured them: by value the allocator packs these kernels
//  tighter -- vq_search_mfma<32, 4, EUCLID, .., WIDE 3> 118 -> 87 VGPRs, <256, 4, ..> 206 -> 198, <512, 4, ..> 104 -> 96 AGPRs --
//  a change of its own to measure, not part of sharing the code.)
template <bool EUCLID>
__device__ __forceinline__ void store_sims_subtile(const f32x16 &acc, const int &u, const int &h, const bool &row_ok, float *const &srow,
                                                   const int &K, const int &vec_s) {
    if (!row_ok) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = EUCLID ? -sqrtf(acc[4 * g + e] < 0.0f ? 0.0f : acc[4 * g + e]) : acc[4 * g + e];
        const int code = u * kTileCodes + 4 * h + 8 * g;
        if (vec_s) {
            if (code < K) *(f32x4 *)(srow + code) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (code + e < K) srow[code + e] = o[e];
        }
    }
}

// which rows of this wave take the repair: bit r = row r (lanes r and r + 32 agree on `best_s` after the merge)
__device__ __forceinline__ unsigned nonfinite_rows(float best_s, bool row_ok) {
    return (unsigned)__ballot(row_ok && !(__builtin_fabsf(best_s) < __builtin_inff()));
}

// Next-stage residual of one element, IN PLACE (the asm ties input and output to one register: the 128 residual
// registers are carried around the stage loop, and an update that defines new values lets the allocator split them).
//   eval : r <- r - c                          (residual_vq.py:232 with quantize = codebook[idx])
//   train: r <- r - (r + (c - r))              (the straight-through value the layer returns, vector_quantize_pytorch.py:273)
// `pv` is the packed value: -2 c for Euclid (so c = -0.5 pv and r - c = fma(pv, 0.5, r) exactly), c itself for the dot metric.
template <int METRIC, bool STE>
__device__ __forceinline__ void residual_step(float &r, float pv) {
    float t;
    if (METRIC == VQ_METRIC_EUCLID) {
        if (STE)
            asm("v_fma_f32 %1, %2, -0.5, -%0\n\tv_add_f32 %1, %0, %1\n\tv_sub_f32 %0, %0, %1" : "+v"(r), "=&v"(t) : "v"(pv));
        else
            asm("v_fmac_f32 %0, 0.5, %1" : "+v"(r) : "v"(pv));
    } else {
        if (STE)
            asm("v_sub_f32 %1, %2, %0\n\tv_add_f32 %1, %0, %1\n\tv_sub_f32 %0, %0, %1" : "+v"(r), "=&v"(t) : "v"(pv));
        else
            asm("v_sub_f32 %0, %0, %1" : "+v"(r) : "v"(pv));
    }
}

// XT: element type of x -- 0 fp32, 1 fp16, 2 bf16.  The 2-byte variants widen in the prologue (the reference's x.float(),
// codebooks.py:354: same values) and exist for inference only: no straight-through / squared-error finalize reads of x.
template <int XT>
__device__ __forceinline__ float widen16(unsigned short b) {
    if (XT == 1) return (float)__builtin_bit_cast(_Float16, b);
    return __uint_as_float((unsigned)b << 16);
}

// ---- the back end shared by the search kernels: what follows the last MFMA of a sweep ------------------------------
// Called by vq_search_mfma and vq_search_pair512; row_winner, fill_row_from_memory and store_winner by vq_search_persist
// and vq_search_resident too.  Shared is what left every kernel's register allocation as it was; the residual update, the
// fused finalize's row bodies and vq_search_mfma's own lane-half merge did not and are written out in their kernels
// (profiles/search_backend_refactor.md has the figures).

// The row's winner: resolve_best, then the two lane halves of each row merge (they saw disjoint codes; ties go to the
// lowest index).  Lanes c and c + 32 leave with the same pair.  (vq_search_mfma spells the merge out: through this
// helper one of its residual kernels is allocated one VGPR fewer.)
template <int METRIC>
__device__ __forceinline__ void row_winner(const LaneBest &lb, int h, int K, float &best_s, int &best_i) {
    resolve_best<METRIC>(lb, h, K, best_s, best_i);
    const float os = __shfl_xor(best_s, 32);
    const int oi = __shfl_xor(best_i, 32);
    const bool take = (METRIC == VQ_METRIC_EUCLID) ? (os < best_s || (os == best_s && oi < best_i))
                                                   : (os > best_s || (os == best_s && oi < best_i));
    if (take) {
        best_s = os;
        best_i = oi;
    }
}

// log-sum-exp of a row's similarities over the whole codebook from the two lane halves' running (max, sum) pairs (fused
// sweeps only: no K split).  Lane half 0 always saw code 0, so the merged maximum is finite.  A NaN similarity in the row
// (`best_s` is NaN then, after the repair) makes the logsumexp NaN.  Every lane of the wave calls it (it shuffles).
__device__ __forceinline__ float close_lse(const LaneBest &lb, float best_s) {
    const float INF = __builtin_inff();
    const float om = __shfl_xor(lb.run_m, 32), os = __shfl_xor(lb.run_s, 32);
    const float mm = fmaxf(lb.run_m, om);
    const float ssum = (lb.run_m > -INF ? lb.run_s * __builtin_amdgcn_exp2f(lb.run_m - mm) : 0.0f) +
                       (om > -INF ? os * __builtin_amdgcn_exp2f(om - mm) : 0.0f);
    const float lse_v = (mm + __builtin_amdgcn_logf(ssum)) * 0.6931471805599453f;
    return (best_s != best_s) ? best_s : lse_v;
}

// keys mode: the row's (value, index) key, by atomic MIN or into this K split's own plane.  Called by lane c of a live row.
template <int METRIC>
__device__ __forceinline__ void store_key(const SearchParams &p, int head, long long row, float best_s, int best_i) {
    const long long key = make_key<METRIC>(best_s, p.idx_offset + best_i);
    long long *dst = p.keys + (long long)head * p.key_hs + row;
    if (p.mode == kModeKeys) atomicMin(dst, key);
    else dst[(long long)blockIdx.z * p.key_zs] = key;  // this K split's own plane
}

// fused mode: stage q's winner of a row (`idx_v`: the index, or the persistent kernel's packed candidates).  Called by
// lane c of a live row.
__device__ __forceinline__ void store_winner(const SearchParams &p, int head, long long row, int q, float best_s, long long idx_v) {
    const long long o = (long long)head * p.idx_hs + row * p.idx_rs + (long long)q * p.idx_qs;
    p.idx[o] = idx_v;
    if (p.best) p.best[o] = best_s;
}

// The repair's `fill_row` for a row that is still in memory: row `grow`, widened and zero padded to DP floats, into
// `rowbuf`; returns the start of its |x|^2 chain (the earlier slices' value for the last slice of a wide row, else 0).
template <int METRIC, int DP, int XT, int WIDE>
__device__ __forceinline__ float fill_row_from_memory(const SearchParams &p, int head, long long grow, float *rowbuf, int lane) {
#pragma clang loop unroll(disable)
    for (int d = lane; d < DP; d += 64) {
        float v = 0.0f;
        if (d < p.D) {
            if constexpr (XT == 0)
                v = p.x[(long long)head * p.x_hs + grow * p.x_rs + d];
            else
                v = widen16<XT>(((const unsigned short *)p.x)[(long long)head * p.x_hs + grow * p.x_rs + d]);
        }
        rowbuf[d] = v;
    }
    if constexpr (WIDE == 2) {
        if (METRIC == VQ_METRIC_EUCLID && p.acc_in) return p.xn_ws[(long long)head * p.xn_hs + grow];
    }
    return 0.0f;
}

// The repair's `acc_init` for the last slice of a wide row: the chain the earlier slices left for (row rr of 32-row block
// `rblock`, code k), read back from the accumulators' fragment layout (float4 index (sub-tile * 4 + g) * 64 + lane).
__device__ __forceinline__ float wide_acc_init(const SearchParams &p, int head, long long rblock, int rr, int k) {
    if (!p.acc_in) return 0.0f;
    const float *wb = (const float *)((const f32x4 *)p.acc_ws + (long long)head * p.ws_hs + (rblock * p.ws_nsub) * 256);
    const int r5 = k & 31;
    return wb[((long long)((k >> 5) * 4 + (r5 >> 3)) * 64 + ((r5 >> 2) & 1) * 32 + rr) * 4 + (r5 & 3)];
}

// WIDE = 2 finish (rows wider than one launch holds, inference call, no K split): out[row] = codebook[widx[row]] over the
// WHOLE row width for rows [lo, hi) of the 32-row block at row0 (natural layout, float4 per lane and 256 dims, four rows
// in flight).
__device__ __forceinline__ void gather_wide_rows(const SearchParams &p, int head, long long row0, int lo, int hi, const int *widx, int lane) {
    const float *cbw = p.cb + (long long)head * p.cb_hs;
    float *outw = p.out + (long long)head * p.out_hs;
    constexpr int RBW = 4;
    for (int rr0 = lo; rr0 < hi; rr0 += RBW) {
        for (int d0 = 4 * lane; d0 < p.fin_D; d0 += 256) {
            f32x4 v[RBW];
#pragma unroll
            for (int k = 0; k < RBW; ++k) {
                const int rr = (rr0 + k < hi) ? rr0 + k : hi - 1;
                v[k] = *(const f32x4 *)(cbw + (long long)widx[rr] * p.fin_D + d0);
            }
#pragma unroll
            for (int k = 0; k < RBW; ++k)
                if (rr0 + k < hi) __builtin_nontemporal_store(v[k], (f32x4 *)(outw + (row0 + rr0 + k) * p.out_rs + d0));
        }
    }
}

// The per-wave loss partials [head][workgroup][wave][Q]: each stage's per-lane partials (MULTI: `lerr`, element q at
// lerr[q * 64]; one stage: `e0`) summed over the wave.
template <int NWAVES, bool MULTI>
__device__ __forceinline__ void store_loss_partials(const SearchParams &p, int head, const float *lerr, float e0, int wave, int lane) {
    float *lp = p.loss_part + (((long long)head * gridDim.x + blockIdx.x) * NWAVES + wave) * p.Q;
    for (int q = 0; q < (MULTI ? p.Q : 1); ++q) {
        float e = MULTI ? lerr[q * 64] : e0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        if (lane == 0) lp[q] = e;
    }
}

// MULTI: 0 one stage; 1 residual stages, eval arithmetic (r <- r - c); 2 residual stages, straight-through arithmetic.
// (The two residual variants are separate instantiations: one update path per kernel keeps the stage loop's 128
//  loop-carried residual registers in place -- with both paths behind a branch the allocator spills ~90 of them.)
// WIDE: 0 rows of up to 512 dims, the whole distance in one launch; 1 / 2 one slice of wider rows -- 1: a full slice, the
// accumulators go to `acc_ws` instead of the argmin (all slices but the last), 2: the sweep starts from `acc_ws` and ends
// in the argmin (last slice, keys mode; padded like a narrow row), 3: the last slice again, but the closed distances are
// written out as the similarity matrix (-sqrt / dot) instead of being reduced.  The MFMA chain of a code is the same k-ordered fmaf chain either way.
template <int DP, int WAVES, int METRIC, int MULTI, bool LSE = false, int XT = 0, int WIDE = 0>
__global__ void __launch_bounds__(WAVES * 64, (DP <= 256 ? 2 : 1)) vq_search_mfma(const SearchParams p) {
    static_assert(WIDE == 0 || (MULTI == 0 && !LSE && XT == 0 && (DP >= 256 || WIDE >= 2)), "wide rows: plain slices, full width but the last");
    constexpr bool WIDE_OUT = (WIDE == 1 || WIDE == 3);  // the accumulators leave the wave instead of entering the argmin
    using G = Geo<DP, WAVES>;
    constexpr int RS = G::RS, RS4 = G::RS4, CH = G::CH, XS = G::XS, NS = G::NS;
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);

    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4 *tile4 = (f32x4 *)smem;
    lds_f32x4 *tile4_lds = (lds_f32x4 *)smem;  // same bytes, LDS address space (LDS-DMA destinations)
    constexpr bool SEP = G::SEP_STAGE && MULTI == 0;
    int *sidx = (int *)(smem + (MULTI ? G::MAIN_FLOATS_M : G::MAIN_FLOATS_S));  // [WAVES][Q][32]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const long long row0 = ((long long)blockIdx.x * WAVES + wave) * 32;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float INF = __builtin_inff();

    // ---------------- prologue: this wave's 32 rows -> MFMA fragments in registers ----------------
    // xf[s] = x[row0 + c][2 s + h]   (lane half h holds the k = h operand of MFMA step s)
    // (load_x_fragments written out in place, with fp16 / bf16 rows and non-temporal loads: see there)
    STAMP(0);
    STAMP_RT(60);
    // Memory-bound phases (prologue, finalize) run at raised priority: when another workgroup's wave is streaming
    // MFMAs on the same SIMD, these few load/store/LDS instructions must not be starved by it.
    __builtin_amdgcn_s_setprio(2);
    if constexpr (SEP) {  // the sweep's first tile, issued before the rows are loaded (its buffer is not the staging region here)
        const float *pk0 = p.packed + (long long)head * p.pk_hs;
        const int tile0 = blockIdx.z * p.tiles_per_split;
#pragma unroll
        for (int i = 0; i < (G::TILE_CHUNKS + WAVES - 1) / WAVES; ++i) {
            const int ck = i * WAVES + wave;
            if (ck < G::TILE_CHUNKS) lds_dma16(pk0, p.pk_bytes, lane * 16, (tile0 * G::TILE_F4 + ck * 64) * 16, tile4_lds + ck * 64);
        }
    }
    float xf[NS];
    float xn0 = 0.0f;  // |x|^2 of row c: d-ordered fmaf chain (the oracle's sumsq_chain)
    if constexpr (WIDE != 0) {
        if (EUCLID && p.acc_in) {  // the chain over the dims of the earlier slices
            long long grow = row0 + c;
            if (grow >= p.M) grow = p.M - 1;
            xn0 = p.xn_ws[(long long)head * p.xn_hs + grow];
        }
    }
    {
        // Wave-private staging region, no workgroup barriers: a wave's LDS operations execute in order.
        // Global loads of chunk i+1 are in flight while chunk i goes through LDS.
        float *xs = smem + (SEP ? G::NBUF * G::BUF_F4 * 4 : 0) + wave * (32 * XS);
        constexpr int NCHUNK = DP / CH;
        constexpr int LPL = CH / 8;  // float4 loads per lane per chunk
        f32x4 v[2][LPL];
        auto load_chunk = [&](int ch, f32x4 (&dst)[LPL]) {
#pragma unroll
            for (int it = 0; it < LPL; ++it) {
                const int f = it * 64 + lane;
                const int r = f / (CH / 4), c4 = f % (CH / 4);
                long long grow = row0 + r;
                if (grow >= p.M) grow = p.M - 1;
                const int d0 = ch * CH + c4 * 4;
                f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (XT == 0) {
                    const float *src = xh + grow * p.x_rs + d0;
                    if (p.vec_x) {
                        if (d0 < p.D) t = __builtin_nontemporal_load((const f32x4 *)src);  // each row is read once
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
                *(f32x4 *)(xs + r * XS + c4 * 4) = v[ch & 1][it];  // XS = CH + 4: b128 accesses conflict-free
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const float *rp = xs + c * XS;  // this lane's row (both lane halves read the same row)
#pragma unroll
            for (int j = 0; j < CH / 8; ++j) {
                const f32x4 lo = *(const f32x4 *)(rp + 8 * j);
                const f32x4 hi = *(const f32x4 *)(rp + 8 * j + 4);
                if (EUCLID) {
                    xn0 = fmaf(lo.x, lo.x, xn0);
                    xn0 = fmaf(lo.y, lo.y, xn0);
                    xn0 = fmaf(lo.z, lo.z, xn0);
                    xn0 = fmaf(lo.w, lo.w, xn0);
                    xn0 = fmaf(hi.x, hi.x, xn0);
                    xn0 = fmaf(hi.y, hi.y, xn0);
                    xn0 = fmaf(hi.z, hi.z, xn0);
                    xn0 = fmaf(hi.w, hi.w, xn0);
                    asm volatile("" : "+v"(xn0));  // pin the chain here: do not keep lo/hi alive to finish it later
                }
                // lower half-wave keeps dims 8j..8j+3, upper 8j+4..8j+7; two half-wave exchanges de-interleave
                // them into the MFMA k-parity layout: lower gets the even dims, upper the odd dims.
                const f32x4 m = h ? hi : lo;
                const auto xy = __builtin_amdgcn_permlane32_swap(__float_as_uint(m.x), __float_as_uint(m.y), false, false);
                const auto zw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m.z), __float_as_uint(m.w), false, false);
                const int sb = ch * (CH / 2) + 4 * j;
                xf[sb + 0] = __uint_as_float(xy[0]);  // dim 8j + 0 + h
                xf[sb + 1] = __uint_as_float(zw[0]);  // dim 8j + 2 + h
                xf[sb + 2] = __uint_as_float(xy[1]);  // dim 8j + 4 + h
                xf[sb + 3] = __uint_as_float(zw[1]);  // dim 8j + 6 + h
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next chunk overwrites
        }
        if constexpr (!SEP) __syncthreads();  // the staging region is about to be reused as codebook tile buffers
    }

    STAMP(1);
    __builtin_amdgcn_s_setprio(0);
    const long long row = row0 + c;
    const bool row_ok = row < p.M;
    if constexpr (WIDE == 1) {
        if (EUCLID && h == 0 && row_ok) p.xn_out[(long long)head * p.xn_hs + row] = xn0;
    }
    // this wave's accumulator slots: float4 index (u * 4 + g) * 64 + lane
    f32x4 *wsw = nullptr;
    if constexpr (WIDE != 0)
        wsw = (f32x4 *)p.acc_ws + (long long)head * p.ws_hs + (((long long)blockIdx.x * WAVES + wave) * p.ws_nsub) * 256 + lane;
    auto ws_load = [&](f32x16 &v, int u) {
        const f32x4 *s4 = wsw + (long long)u * 256;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 t = s4[g * 64];
            v[4 * g + 0] = t.x; v[4 * g + 1] = t.y; v[4 * g + 2] = t.z; v[4 * g + 3] = t.w;
        }
    };
    auto ws_store = [&](const f32x16 &v, int u) {
        if constexpr (WIDE == 3) {
            store_sims_subtile<EUCLID>(v, u, h, row_ok, p.sims + (long long)head * p.sims_hs + row * p.sims_rs, p.K, p.vec_s);
        } else {
            f32x4 *s4 = wsw + (long long)u * 256;
#pragma unroll
            for (int g = 0; g < 4; ++g) s4[g * 64] = (f32x4){v[4 * g + 0], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
        }
    };

    for (int q = 0; q < (MULTI ? p.Q : 1); ++q) {
        const float *pk = p.packed + (long long)head * p.pk_hs + (long long)q * p.pk_qs;
        STAMP(4 + 5 * q + 3);

        // |x|^2 of the current residual (d-ordered fmaf chain, the oracle's sumsq_chain): stage 0 has it from the prologue,
        // later stages from the residual update at the end of the previous stage (`xn0` is carried in the lower lane half)
        const float b_aug = EUCLID ? (h ? 1.0f : xn0) : 1.0f;  // B[k=0][row] = |x|^2, B[k=1][row] = 1
        STAMP(4 + 5 * q + 0);
        LaneBest lb = lane_best_start<METRIC>(sweep_start_value<METRIC>(codebook_flag(pk, p.pk_bytes)));

        const int t0 = blockIdx.z * p.tiles_per_split;
        const int t1 = (t0 + p.tiles_per_split < p.ntiles) ? t0 + p.tiles_per_split : p.ntiles;

        // LDS-DMA of one tile image: buffer_load ... lds with the per-lane part (lane * 16 B) in voffset and the
        // tile / chunk position in the SCALAR offset -> no vector instructions at all per issue (on gfx950 VALU
        // work is not free beside f32 MFMA: it executes on the same lanes).
        auto stage = [&](int tile, int buf) {
#pragma unroll
            for (int i = 0; i < (G::TILE_CHUNKS + WAVES - 1) / WAVES; ++i) {
                const int ck = i * WAVES + wave;
                if (ck < G::TILE_CHUNKS)
                    lds_dma16(pk, p.pk_bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16,
                              tile4_lds + buf * G::BUF_F4 + ck * 64);
            }
        };
        constexpr int SUB = G::SUB;
        const int ws_end = (t1 * SUB < p.ws_nsub) ? t1 * SUB : p.ws_nsub;  // (a staged tile may end in sub-tiles past the last code)
        // One 32-code sub-tile: Dp/2 MFMAs into `acc`, then the augmented-column MFMA (|x|^2 * 1 + 1 * |c|^2).
        // Software pipelined inside the wave: the PREVIOUS sub-tile's reduction (`prev`, finished long ago, so no
        // MFMA drain) and the NEXT tile's LDS-DMA issue are expanded between MFMA groups.  `u` counts 32-code
        // sub-tiles from code 0.  (Measured alternatives -- explicit wave roles, half-tile stagger -- are slower:
        // f32 MFMA runs on the SIMD's FMA lanes, so a streaming wave starves its SIMD partner; see DESIGN.md.)
        // `stc`: the sub-tile's position inside its staged tile when the caller knows it at compile time (tiles of several
        // sub-tiles, Dp < 256: the LDS offsets become immediates and the stage / barrier tests disappear), else IntC<-1>.
        auto run_sub = [&](f32x16 &acc, f32x16 &prev, int u, bool have_prev, auto stc, int tile = 0) {
            constexpr int STC = decltype(stc)::value;
            const int t = STC >= 0 ? tile : u / SUB, st = STC >= 0 ? STC : u % SUB;
            const int cur = (t - t0) & 1;
            const f32x4 *tb = tile4 + cur * G::BUF_F4 + st * (kTileCodes * RS4);
            constexpr int NG = DP / 8;
            constexpr int G1 = NG >= 2 ? 1 : NG, G2 = NG >= 4 ? 3 : NG;
            const f32x4 *ta = tb + c * RS4 + h;
            f32x4 a[NG];
            if (WIDE == 0 || !p.acc_in) acc = (f32x16){0};  // (else: loaded from acc_ws during the previous sub-tile)
            // |c|^2 of this lane's code for the augmented MFMA: read now so its LDS latency is not paid at the tail
            // (float Dp of a packed row is |c|^2, float Dp + 1 is 1.0: lane half h reads A[code][k = h] directly)
            const float a_aug = (EUCLID && WIDE != 1) ? ((const float *)tb)[c * RS + DP + 1 - h] : 0.0f;
            mfma_prefetch<DP>(a, ta);
            mfma_range<DP, 0, G1>(acc, a, ta, xf);
            if constexpr (WIDE_OUT) {
                if (have_prev) ws_store(prev, u - 1);
            } else {
                if (have_prev) tile_epilogue<METRIC, DP, LSE>(prev, u - 1, h, p.K, lb);
            }
            if constexpr (WIDE != 0) {
                if (p.acc_in && u + 1 < ws_end) ws_load(prev, u + 1);  // `prev` is the next sub-tile's accumulator
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_range<DP, G1, G2>(acc, a, ta, xf);
            if (st == 0 && t + 1 < t1) stage(t + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_range<DP, G2, NG>(acc, a, ta, xf);
            if (EUCLID && WIDE != 1) {  // (wide rows: the norms close the chain, in the last slice)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);  // A[code][k=0] = 1, A[code][k=1] = |c|^2
            }
            if (st == SUB - 1) __syncthreads();  // next tile landed (vmcnt(0)), everybody is done reading this one
        };

        if (MULTI && q > 0) __syncthreads();  // every wave is done with its gather region (it aliases the tile buffers)
        if constexpr (!SEP) stage(t0, 0);     // (SEP: issued before the prologue)
        __syncthreads();
        {
            f32x16 acc0, acc1;
            int u = t0 * SUB;
            const int u1 = t1 * SUB;
            bool have_prev = false;
            if constexpr (WIDE != 0) {
                if (p.acc_in && u < ws_end) ws_load(acc0, u);
            }
            if constexpr (SUB >= 2) {
                // whole tiles (a K split is a range of tiles), sub-tile positions as compile-time constants
                int tile = t0;
                auto pair = [&](bool hp, auto stc) {
                    constexpr int ST = decltype(stc)::value;
                    run_sub(acc0, acc1, u + ST, hp, IntC<ST>{}, tile);
                    run_sub(acc1, acc0, u + ST + 1, true, IntC<ST + 1>{}, tile);
                };
                for (; u < u1; u += SUB, ++tile) {
                    pair(have_prev, IntC<0>{});
                    if constexpr (SUB >= 4) pair(true, IntC<2>{});
                    if constexpr (SUB >= 8) {
                        pair(true, IntC<4>{});
                        pair(true, IntC<6>{});
                    }
                    have_prev = true;
                }
            } else {
                for (; u + 1 < u1; u += 2) {
                    run_sub(acc0, acc1, u, have_prev, IntC<-1>{});
                    run_sub(acc1, acc0, u + 1, true, IntC<-1>{});
                    have_prev = true;
                }
            }
            if constexpr (WIDE_OUT) {
                if (u < u1) {
                    run_sub(acc0, acc1, u, have_prev, IntC<-1>{});
                    ws_store(acc0, u);
                } else if (have_prev) {
                    ws_store(acc1, u - 1);
                }
                return;  // every wave has passed the sweep's last barrier
            } else {
                if (u < u1) {
                    run_sub(acc0, acc1, u, have_prev, IntC<-1>{});
                    tile_epilogue<METRIC, DP, LSE>(acc0, u, h, p.K, lb);
                } else if (have_prev) {
                    tile_epilogue<METRIC, DP, LSE>(acc1, u - 1, h, p.K, lb);
                }
            }
        }

        STAMP(4 + 5 * q + 1);
        float best_s;
        int best_i;
        resolve_best<METRIC>(lb, h, p.K, best_s, best_i);

        // merge the two lane halves of each row (they saw disjoint codes)
        {
            const float os = __shfl_xor(best_s, 32);
            const int oi = __shfl_xor(best_i, 32);
            const bool take = EUCLID ? (os < best_s || (os == best_s && oi < best_i))
                                     : (os > best_s || (os == best_s && oi < best_i));
            if (take) {
                best_s = os;
                best_i = oi;
            }
        }

        // non-finite inputs (rare, out of line): rows whose winner is not finite, every row of a flagged codebook
        if (const unsigned todo = nonfinite_rows(best_s, row_ok); __builtin_expect(todo != 0u, 0)) {
            float *rowbuf = MULTI ? smem + wave * G::GWAVE_F : smem + (SEP ? G::NBUF * G::BUF_F4 * 4 : 0) + wave * (32 * XS);
            auto fill_row = [&](int rr) -> float {
                const long long grow = row0 + rr;
                if constexpr (MULTI != 0) {
                    // the residual this stage searches IS this wave's fragment registers: lanes (rr, h) hold dims 2 s + h of
                    // row rr (the padding dims are zeros there too).  No memory traffic and no extra scalar state: rebuilding
                    // the residual from the earlier stages' winners cost these kernels their scratch-free register allocation.
                    if (c == rr) {
#pragma unroll
                        for (int s = 0; s < NS; ++s) rowbuf[2 * s + h] = xf[s];
                    }
                    return 0.0f;
                }
                return fill_row_from_memory<METRIC, DP, XT, WIDE>(p, head, grow, rowbuf, lane);
            };
            auto acc_init = [&](int rr, int k) -> float {
                if constexpr (WIDE == 2) return wide_acc_init(p, head, (long long)blockIdx.x * WAVES + wave, rr, k);
                return 0.0f;
            };
            const int k0 = t0 * G::TILE_CODES;
            const int k1 = (t1 * G::TILE_CODES < p.K) ? t1 * G::TILE_CODES : p.K;
            repair_nonfinite_rows<METRIC, DP>(todo, rowbuf, pk, k0, k1, lane, fill_row, acc_init, best_s, best_i);
        }

        if constexpr (LSE) {
            const float lse_v = close_lse(lb, best_s);
            if (h == 0 && row_ok) p.lse[(long long)head * p.M + row] = lse_v;
        }

        if constexpr (!MULTI) {
            // keys mode is single-stage by contract, so the multi-stage kernels do not contain this exit at all: a second
            // latch on the stage loop made the allocator split the 128 loop-carried residual registers (187 spilled VGPRs)
            if (p.mode != kModeFused) {
                if (h == 0 && row_ok) store_key<METRIC>(p, head, row, best_s, best_i);
                continue;  // (single trip: leaves the stage loop)
            }
        }

        if (h == 0 && row_ok) store_winner(p, head, row, q, best_s, best_i);
        sidx[(wave * p.Q + q) * 32 + c] = best_i;
        STAMP(4 + 5 * q + 2);

        // winners' packed rows -> next-stage residual, in fragment layout  (residual_vq.py:232)
        if (MULTI && q + 1 < p.Q) {
            // A lane's float4 at piece 2g + h of its winner's packed row is exactly its four k-parity values of group g.
            // Slice by slice: LDS-DMA copies [GRPI rows][GPP pieces] per instruction (piece index XOR row-in-block, so that
            // the fragment reads below are bank-conflict free), the wave waits for its own copies only (wave-private region,
            // no workgroup barrier), reads its pieces, re-issues the next slice's copies and updates the registers.
            char *gb = (char *)smem + wave * (G::GWAVE_F * 4);
            const int grho = lane / G::GPP, gk = lane % G::GPP;
            int roff[G::GNI];  // byte offset of this lane's piece inside the stage's packed image, slice 0
#pragma unroll
            for (int i = 0; i < G::GNI; ++i)
                roff[i] = sidx[(wave * p.Q + q) * 32 + i * G::GRPI + grho] * (RS * 4) + ((gk ^ grho) * 16);
            auto gather = [&](int sl) {
#pragma unroll
                for (int i = 0; i < G::GNI; ++i)
                    lds_dma16(pk, p.pk_bytes, roff[i], sl * (G::GS * 32), (lds_f32x4 *)(gb + i * G::GIB));
            };
            const int crho = c % G::GRPI;
            const char *rbase = gb + (c / G::GRPI) * G::GIB + crho * (G::GPP * 16);
            const int wx = h ^ crho;  // piece (2 g + h) ^ crho = (2 g) ^ wx
            float xn = 0.0f;
            gather(0);
#pragma unroll
            for (int sl = 0; sl < G::GNSL; ++sl) {
                f32x4 pv[G::GS];
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's copies have landed
#pragma unroll
                for (int k = 0; k < G::GS; ++k) pv[k] = *(const f32x4 *)(rbase + (((2 * k) ^ wx) * 16));
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the region is overwritten
                __builtin_amdgcn_sched_barrier(0);                  // (keeps the reads back to back, ahead of the arithmetic)
                if (sl + 1 < G::GNSL) gather(sl + 1);
#pragma unroll
                for (int k = 0; k < G::GS; ++k)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        float &r = xf[4 * (sl * G::GS + k) + u];
                        residual_step<METRIC, MULTI == 2>(r, pv[k][u]);
                        if (EUCLID) {
                            // |r|^2 for the next stage: the lower lane half walks the row's chain, fetching the odd dims
                            // from its partner lane (the upper half computes a value nobody reads)
                            // (the builtin, not inline asm: v_permlane32_swap needs wait states after a vector write of
                            //  its operands, which the compiler's hazard recognizer only inserts for instructions it knows)
                            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r), 0u, false, false);
                            const float t1 = __uint_as_float(sw[1]);  // lower half: the partner lane's r (odd dim)
                            xn = __builtin_fmaf(r, r, xn);
                            xn = __builtin_fmaf(t1, t1, xn);
                        }
                    }
            }
            xn0 = xn;
        }
        STAMP(4 + 5 * q + 4);
    }

    STAMP(2);
    __builtin_amdgcn_s_setprio(2);
    if (WIDE == 1 || WIDE == 3 || p.mode != kModeFused) return;
    if constexpr (WIDE == 2) {
        gather_wide_rows(p, head, row0, 0, (p.M - row0 >= 32) ? 32 : (int)(p.M - row0), sidx + wave * 32, lane);
        return;
    }
    if (p.out == nullptr && p.loss_part == nullptr) return;

    // ---------------- fused finalize (natural layout) ----------------
    //   quant_q = c_q[idx_q]                       (eval)      vector_quantize_pytorch.py:227
    //           = r_q + (c_q[idx_q] - r_q)         (train)     vector_quantize_pytorch.py:273
    //   r_{q+1} = r_q - quant_q ; out = ((0 + quant_1) + quant_2) + ...   residual_vq.py:232-233
    //   sq_err_q += (c_q[idx_q] - r_q)^2                                   vector_quantize_pytorch.py:362
    const bool need_r = p.ste || p.loss_part;
    float *lerr = (float *)(sidx + WAVES * p.Q * 32) + (wave * p.Q) * 64 + lane;  // [WAVES][Q][64], MULTI only
    if (MULTI && p.loss_part)
        for (int q = 0; q < p.Q; ++q) lerr[q * 64] = 0.0f;
    float e0 = 0.0f;
    const float *cbh = p.cb + (long long)head * p.cb_hs;
    float *outh = p.out ? p.out + (long long)head * p.out_hs : nullptr;
    const int nrows = (p.M - row0 >= 32) ? 32 : (int)(p.M - row0);  // wave-uniform, >= 1 ... rows of this wave
    constexpr int RB = 4;  // rows in flight: the gathers are latency-bound, so issue RB rows' loads before using them
    if constexpr (DP <= 128) {
        // Short rows: a 64-lane float4 access covers 64 / (Dp / 4) ROWS (8 / 4 / 2 at Dp = 32 / 64 / 128) instead of one row
        // with three quarters of the lanes idle: 4x fewer gathers, stores and address computations at D = 64.  (The
        // finalize of a wave runs beside other waves' MFMA streams, which starve its vector work: at cfg3a it took a
        // median 90 k cycles, 4 % of a wave's life.)
        constexpr int LPR = DP / 4;    // lanes per row
        constexpr int RPI = 64 / LPR;  // rows per instruction
        constexpr int NI = 4;          // instructions in flight
        constexpr int QBS = 4;         // stages gathered together (residual kernels; more would cost occupancy here)
        const int sub = lane / LPR, dl = 4 * (lane % LPR);
        const bool dok = dl < p.D;
        const int nq = MULTI ? p.Q : 1;
        for (int rr0 = 0; rr0 < (p.vec_fin ? nrows : 0); rr0 += NI * RPI) {
            f32x4 r[NI], o[NI];
            int rrc[NI];
            bool live[NI];
#pragma unroll
            for (int k = 0; k < NI; ++k) {
                const int rr = rr0 + k * RPI + sub;
                live[k] = rr < nrows;
                rrc[k] = live[k] ? rr : nrows - 1;  // clamp: duplicates are computed, not stored
                o[k] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                r[k] = o[k];
                if (need_r && dok) r[k] = *(const f32x4 *)(xh + (row0 + rrc[k]) * p.x_rs + dl);
            }
            for (int q0 = 0; q0 < nq; q0 += QBS) {
                f32x4 cv[QBS][NI];
#pragma unroll
                for (int kq = 0; kq < QBS; ++kq) {
                    if (q0 + kq < nq) {
#pragma unroll
                        for (int k = 0; k < NI; ++k) {
                            const int i = sidx[(wave * p.Q + q0 + kq) * 32 + rrc[k]];
                            const float *crow = cbh + (long long)(q0 + kq) * p.cb_qs + (long long)i * p.D;
                            cv[kq][k] = dok ? *(const f32x4 *)(crow + dl) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                        }
                    }
                }
#pragma unroll
                for (int kq = 0; kq < QBS; ++kq) {
                    if (q0 + kq < nq) {
                        float e = 0.0f;
#pragma unroll
                        for (int k = 0; k < NI; ++k) {
                            f32x4 quant = cv[kq][k];
                            if (need_r) {
                                const f32x4 diff = cv[kq][k] - r[k];
                                if (live[k]) {
                                    e = fmaf(diff.x, diff.x, e);
                                    e = fmaf(diff.y, diff.y, e);
                                    e = fmaf(diff.z, diff.z, e);
                                    e = fmaf(diff.w, diff.w, e);
                                }
                                if (p.ste) quant = r[k] + diff;
                                r[k] = r[k] - quant;
                            }
                            o[k] = o[k] + quant;
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
                for (int k = 0; k < NI; ++k)
                    if (live[k] && dok) __builtin_nontemporal_store(o[k], (f32x4 *)(outh + (row0 + rrc[k]) * p.out_rs + dl));
            }
        }
    } else
    for (int rr0 = 0; rr0 < (p.vec_fin ? nrows : 0); rr0 += RB) {
        f32x4 r[RB][G::NCH4], o[RB][G::NCH4];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int rr = (rr0 + k < nrows) ? rr0 + k : nrows - 1;  // clamp: duplicates are computed, not stored
            const float *xr = xh + (row0 + rr) * p.x_rs;
#pragma unroll
            for (int j = 0; j < G::NCH4; ++j) {
                const int d = 4 * (lane + 64 * j);
                o[k][j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                r[k][j] = o[k][j];
                if (need_r && d < p.D) r[k][j] = *(const f32x4 *)(xr + d);
            }
        }
        if constexpr (MULTI != 0) {
            // Residual stages: the gathers of QB stages x RB rows are issued together (the chain over the stages is cheap
            // arithmetic; issued stage by stage, the latency of Q dependent rounds of loads dominated the finalize).
            constexpr int QB = (G::NCH4 == 1) ? 8 : 4;
            for (int q0 = 0; q0 < p.Q; q0 += QB) {
                f32x4 cv[QB][RB][G::NCH4];
#pragma unroll
                for (int kq = 0; kq < QB; ++kq) {
                    if (q0 + kq < p.Q) {
#pragma unroll
                        for (int k = 0; k < RB; ++k) {
                            const int rr = (rr0 + k < nrows) ? rr0 + k : nrows - 1;
                            const int i = sidx[(wave * p.Q + q0 + kq) * 32 + rr];
                            const float *crow = cbh + (long long)(q0 + kq) * p.cb_qs + (long long)i * p.D;
#pragma unroll
                            for (int j = 0; j < G::NCH4; ++j) {
                                const int d = 4 * (lane + 64 * j);
                                cv[kq][k][j] = (d < p.D) ? *(const f32x4 *)(crow + d) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                            }
                        }
                    }
                }
#pragma unroll
                for (int kq = 0; kq < QB; ++kq) {
                    if (q0 + kq < p.Q) {
                        float e = 0.0f;
#pragma unroll
                        for (int k = 0; k < RB; ++k) {
                            const bool live = rr0 + k < nrows;
#pragma unroll
                            for (int j = 0; j < G::NCH4; ++j) {
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
                        if (p.loss_part) lerr[(q0 + kq) * 64] += e;
                    }
                }
            }
        } else {
            for (int q = 0; q < (MULTI ? p.Q : 1); ++q) {
                f32x4 cv[RB][G::NCH4];
    #pragma unroll
                for (int k = 0; k < RB; ++k) {
                    const int rr = (rr0 + k < nrows) ? rr0 + k : nrows - 1;
                    const int i = sidx[(wave * p.Q + q) * 32 + rr];
                    const float *crow = cbh + (long long)q * p.cb_qs + (long long)i * p.D;
    #pragma unroll
                    for (int j = 0; j < G::NCH4; ++j) {
                        const int d = 4 * (lane + 64 * j);
                        cv[k][j] = (d < p.D) ? *(const f32x4 *)(crow + d) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                    }
                }
                float e = 0.0f;
    #pragma unroll
                for (int k = 0; k < RB; ++k) {
                    const bool live = rr0 + k < nrows;
    #pragma unroll
                    for (int j = 0; j < G::NCH4; ++j) {
                        f32x4 quant = cv[k][j];
                        if (need_r) {
                            const f32x4 diff = cv[k][j] - r[k][j];
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
                    if (p.loss_part) lerr[q * 64] += e;
                } else {
                    e0 += e;
                }
            }
        }
        if (outh) {
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                if (rr0 + k < nrows) {
                    float *orow = outh + (row0 + rr0 + k) * p.out_rs;
#pragma unroll
                    for (int j = 0; j < G::NCH4; ++j) {
                        const int d = 4 * (lane + 64 * j);
                        if (d < p.D) __builtin_nontemporal_store(o[k][j], (f32x4 *)(orow + d));  // streamed once, never re-read
                    }
                }
            }
        }
    }
    for (int rr = 0; rr < (p.vec_fin ? 0 : nrows); ++rr) {
        const long long grow = row0 + rr;
        const float *xr = xh + grow * p.x_rs;
        float *orow = outh ? outh + grow * p.out_rs : nullptr;
        {
            float r[G::NEL], o[G::NEL];
#pragma unroll
            for (int j = 0; j < G::NEL; ++j) {
                const int d = lane + 64 * j;
                o[j] = 0.0f;
                r[j] = (need_r && d < p.D) ? xr[d] : 0.0f;
            }
            for (int q = 0; q < (MULTI ? p.Q : 1); ++q) {
                const int i = sidx[(wave * p.Q + q) * 32 + rr];
                const float *crow = cbh + (long long)q * p.cb_qs + (long long)i * p.D;
                float e = 0.0f;
#pragma unroll
                for (int j = 0; j < G::NEL; ++j) {
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
                for (int j = 0; j < G::NEL; ++j) {
                    const int d = lane + 64 * j;
                    if (d < p.D) orow[d] = o[j];
                }
            }
        }
    }
    STAMP(3);
    STAMP_RT(61);
    if (p.loss_part) store_loss_partials<WAVES, MULTI != 0>(p, head, lerr, e0, wave, lane);
}

