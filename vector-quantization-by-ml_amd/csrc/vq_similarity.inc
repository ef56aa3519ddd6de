// vq_similarity.inc -- consumers of the similarity matrix on the same sweep: emission, online-softmax statistics,
// Gumbel-max sampling, fused cross-entropy backward.  Included by vq_kernels.hip (after vq_search.inc: shares its tile geometry and fragment pipeline).
// ------------------------------------------------------------------------------------------------
// similarity consumers (SURVEY 8f rank 3): the same MFMA sweep with three other epilogues.
//   kAuxSims   write sim[h, m, k] = -sqrt(max(0, t)) (Euclid) / x.c (dot) -- the third return value of
//              Codebook.forward (codebooks.py:386,435), bit-identical to the values the search compares.
//   kAuxStats  online softmax over logits = scale * sim: per row log-sum-exp and the logit of a given target code
//              (F.cross_entropy(distances, codes) -- vector_quantize_pytorch.py:287-297 -- without [M, K] in memory).
//   kAuxSample Gumbel-max sampling (utils/general.py:112-129): key = sim * tau + gumbel noise (counter-based, made in
//              registers: vq_sample.inc), running first-index argmax per row -- no [M, K] tensor, no noise tensor.
// Performance is secondary here (training-only losses): plain loop, no in-wave software pipeline.
// ------------------------------------------------------------------------------------------------
constexpr int kAuxSims = 0;
constexpr int kAuxStats = 1;
constexpr int kAuxSample = 2;

}  // namespace
namespace vqi {
struct AuxParams {
    const float *x;
    long long x_rs, x_hs;
    const float *packed;
    long long pk_hs;
    unsigned pk_bytes;
    long long M;
    int K, D, ntiles, vec_x;
    float *sims;  // kAuxSims
    long long sims_rs, sims_hs;
    int vec_s;
    float scale;  // kAuxStats
    const long long *target;
    long long tgt_rs, tgt_hs;
    float *lse, *tgt_logit;  // [H * M]
    float tau;  // kAuxSample: 1 / temperature
    const long long *seed;  // two words on the device
    long long *idx;
    long long idx_rs, idx_hs;
};
}  // namespace vqi
namespace {
using vqi::AuxParams;

template <int DP, int WAVES, int METRIC, int MODE>
__global__ void __launch_bounds__(WAVES * 64, (DP <= 256 ? 2 : 1)) vq_sweep_aux(const AuxParams p) {
    using G = Geo<DP, WAVES>;
    constexpr int RS = G::RS, RS4 = G::RS4, SUB = G::SUB, NG = DP / 8;
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);

    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4 *tile4 = (f32x4 *)smem;
    lds_f32x4 *tile4_lds = (lds_f32x4 *)smem;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const long long row0 = ((long long)blockIdx.x * WAVES + wave) * 32;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float INF = __builtin_inff();

    float xf[DP / 2];
    float xn0 = 0.0f;
    load_x_fragments<G::CH, G::XS, DP / G::CH, EUCLID>(xh, p.x_rs, p.M, p.D, p.vec_x, row0, true, smem, wave, lane, xf, xn0);
    __syncthreads();  // the staging region is about to be reused as codebook tile buffers

    const long long row = row0 + c;
    const bool row_ok = row < p.M;
    const float *pk = p.packed + (long long)head * p.pk_hs;
    const float b_aug = h ? 1.0f : xn0;

    // kAuxStats state: running max / sum of exp over the codes this lane has seen, and the target's logit.  A NaN logit makes
    // the row's log-sum-exp NaN (ATen's logsumexp; the search's LSE variant does the same).  Once a lane has a running max, the
    // accumulation carries a NaN logit into run_s by itself (exp(NaN) is NaN, and it survives every rescaling); fmaxf drops a
    // NaN, so a lane that has seen nothing but NaN / -inf logits never gets that far and remembers the NaN in a flag.
    float run_m = -INF, run_s = 0.0f, tgt_l = -INF;
    bool saw_nan = false;
    int tgt = -1;
    if (MODE == kAuxStats && p.target && row_ok) {
        const long long tv = p.target[(long long)head * p.tgt_hs + row * p.tgt_rs];
        tgt = (tv >= 0 && tv < p.K) ? (int)tv : (tv < 0 ? -1 : -2);  // -2: out of range -> logit stays -inf
    }
    // kAuxSample state: the best key this lane has seen and its code.  ATen's argmax rule: a NaN key is the maximum, among equal
    // maxima the first code wins -- a lane sees its codes in ascending order, so only a strictly better key replaces the record.
    // (A lane half whose first code 4h is past K never updates: its -inf loses every tie against lane half 0's lower code.)
    float best_key = -INF;
    int best_code = 4 * h;
    unsigned long long seed0 = 0, seed1 = 0;
    if (MODE == kAuxSample) {
        seed0 = (unsigned long long)p.seed[0];
        seed1 = (unsigned long long)p.seed[1];
    }
    // sub-tile and register that hold the target for THIS lane (-1: never)
    const int tgt_u = (tgt >= 0 && ((tgt >> 2) & 1) == h) ? (tgt >> 5) : -1;
    const int tgt_r = (tgt & 3) + 4 * ((tgt >> 3) & 3);

    auto stage = [&](int tile, int buf) {
#pragma unroll
        for (int i = 0; i < (G::TILE_CHUNKS + WAVES - 1) / WAVES; ++i) {
            const int ck = i * WAVES + wave;
            if (ck < G::TILE_CHUNKS)
                lds_dma16(pk, p.pk_bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16,
                          tile4_lds + buf * G::BUF_F4 + ck * 64);
        }
    };

    // what happens to a finished 32 x 32 result (sub-tile u): the similarity values leave for memory, or feed the online softmax
    auto epilogue = [&](const f32x16 &acc, int u) {
        const int cbase = u * kTileCodes + 4 * h;
        if (MODE == kAuxSims) {
            float *srow = p.sims + (long long)head * p.sims_hs + row * p.sims_rs;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float tv = acc[4 * g + e];
                    v[e] = EUCLID ? -sqrtf(tv < 0.0f ? 0.0f : tv) : tv;  // correctly rounded, like the search; keeps NaN
                }
                const int code = cbase + 8 * g;
                if (row_ok) {
                    if (p.vec_s) {
                        if (code < p.K) *(f32x4 *)(srow + code) = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (code + e < p.K) srow[code + e] = v[e];
                    }
                }
            }
        } else if (MODE == kAuxSample) {
            const bool tail = u * kTileCodes + kTileCodes > p.K;  // wave-uniform
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int code = cbase + 8 * g;
                const f32x4 nz = gumbel_noise4(seed0, seed1, head, row, code >> 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float tv = acc[4 * g + e];
                    const float s = EUCLID ? -sqrtf(tv < 0.0f ? 0.0f : tv) : tv;  // the value kAuxSims writes
                    const float key = __fadd_rn(__fmul_rn(s, p.tau), nz[e]);      // two roundings, like ATen's mul and add
                    bool better = !(key <= best_key) && best_key == best_key;     // greater, or the first NaN
                    if (tail) better = better && code + e < p.K;                  // padding codes never compete
                    best_key = better ? key : best_key;
                    best_code = better ? code + e : best_code;
                }
            }
        } else {
            float l[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float tv = acc[r];
                l[r] = EUCLID ? -p.scale * __builtin_amdgcn_sqrtf(tv < 0.0f ? 0.0f : tv) : p.scale * tv;  // keeps NaN, like kAuxSims
            }
            if (u * kTileCodes + kTileCodes > p.K) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (cbase + (r & 3) + 8 * (r >> 2) >= p.K) l[r] = -INF;
            }
            if (u == tgt_u) {
#pragma unroll
                for (int r = 0; r < 16; ++r) tgt_l = (r == tgt_r) ? l[r] : tgt_l;
            }
            float tm = l[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) tm = fmaxf(tm, l[r]);
            if (tm > run_m) {
                run_s *= __expf(run_m - tm);  // exp(-inf) = 0 on the first visit
                run_m = tm;
            }
            if (run_m > -INF) {
#pragma unroll
                for (int r = 0; r < 16; ++r) run_s += __expf(l[r] - run_m);
            } else {
                // (taken after the tail masking: the padding codes of a row that holds an inf are NaN by 0 * inf and do not count)
                asm volatile("" ::: "memory");  // keep this a branch: rows without a finite logit are rare
#pragma unroll
                for (int r = 0; r < 16; ++r) saw_nan = saw_nan || l[r] != l[r];
            }
        }
    };
    // One 32-code sub-tile, software pipelined inside the wave like the search kernel's: two accumulators alternate, the
    // PREVIOUS sub-tile's epilogue (finished long ago: no MFMA drain, and its ~100 vector instructions sit inside the
    // current MFMA stream) runs between the first and the remaining MFMA groups.
    auto run_sub = [&](f32x16 &acc, f32x16 &prev, int u, int st, int cur, bool have_prev) {
        const f32x4 *tb = tile4 + cur * G::BUF_F4 + st * (kTileCodes * RS4);
        const f32x4 *ta = tb + c * RS4 + h;
        constexpr int G1 = NG >= 2 ? 1 : NG;
        f32x4 a[NG];
        acc = (f32x16){0};
        const float cnv = EUCLID ? ((const float *)tb)[c * RS + DP] : 0.0f;
        mfma_prefetch<DP>(a, ta);
        mfma_range<DP, 0, G1>(acc, a, ta, xf);
        if (have_prev) epilogue(prev, u - 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_range<DP, G1, NG>(acc, a, ta, xf);
        if (EUCLID) {
            const float a_aug = h ? cnv : 1.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
        }
    };

    stage(0, 0);
    __syncthreads();
    f32x16 acc0, acc1;
    int last_u = -1;   // the sub-tile whose result is still waiting for its epilogue (in acc0 if even count so far, else acc1)
    bool odd = false;  // which accumulator the NEXT sub-tile uses
    for (int t = 0; t < p.ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < p.ntiles) stage(t + 1, cur ^ 1);
#pragma unroll 1
        for (int st = 0; st < SUB; ++st) {
            const int u = t * SUB + st;
            if (u * kTileCodes >= p.K) break;  // wave-uniform: nothing but padding from here on
            if (!odd) run_sub(acc0, acc1, u, st, cur, last_u >= 0);
            else run_sub(acc1, acc0, u, st, cur, true);
            odd = !odd;
            last_u = u;
        }
        __syncthreads();  // next tile landed, everybody is done reading this one
    }
    if (last_u >= 0) {
        if (odd) epilogue(acc0, last_u);  // (the last sub-tile went into acc0)
        else epilogue(acc1, last_u);
    }

    if (MODE == kAuxSample) {
        const float ok = __shfl_xor(best_key, 32);
        const int oc = __shfl_xor(best_code, 32);
        const bool other_better = !(ok <= best_key) && best_key == best_key;
        const bool mine_better = !(best_key <= ok) && ok == ok;
        const bool take = other_better || (!mine_better && oc < best_code);  // equal keys, or both NaN: the lower code
        if (h == 0 && row_ok) p.idx[(long long)head * p.idx_hs + row * p.idx_rs] = take ? oc : best_code;
    }
    if (MODE == kAuxStats) {
        if (saw_nan) {  // travels to the other lane half in the sum: NaN * exp(0 - mm) stays NaN for every mm
            run_m = 0.0f;
            run_s = __builtin_nanf("");
        }
        const float om = __shfl_xor(run_m, 32), os = __shfl_xor(run_s, 32), ot = __shfl_xor(tgt_l, 32);
        const float mm = fmaxf(run_m, om);  // lane half 0 always saw code 0, so mm is finite
        const float s = (run_m > -INF ? run_s * __expf(run_m - mm) : 0.0f) + (om > -INF ? os * __expf(om - mm) : 0.0f);
        if (h == 0 && row_ok) {
            const long long o = (long long)head * p.M + row;
            p.lse[o] = mm + __logf(s);
            // the lane half that holds the target recorded its logit (fmaxf of the two would drop a NaN one); -2: stays -inf
            if (p.tgt_logit) p.tgt_logit[o] = (tgt == -1) ? 0.0f : ((tgt >= 0 && ((tgt >> 2) & 1)) ? ot : tgt_l);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// fused cross-entropy backward (SURVEY 8f rank 3):  d/dx of  coef * sum_rows (logsumexp_k sim - sim[target])
//   S sweep      t[code, row] exactly as in the search (codes on the MFMA i axis, rows on j)
//   epilogue     p = exp(sim - lse[row]);  gs = coef * (p - [code == target])            (d loss / d sim)
//                Euclid: ratio = gs / sim (0 where sim == 0)   -- ATen _euclidean_dist_backward with dist = -sim
//   G sweep      the 16 accumulator registers of the S sweep are, as they stand, valid B operands of
//                v_mfma_f32_32x32x2_f32 for the second contraction (register r of the two lane halves = one k-pair of
//                codes), so  G[pos, row] += Cimg[code, pos] * ratio[code, row]  needs no shuffles: Dp/2 more MFMAs per
//                sub-tile, A fragments read from the SAME LDS tile (one ds_read_b128 feeds 4 MFMAs, "virtual" d-chunks
//                of stride 4).
//   finalize     Euclid: gx = x * sum_k ratio + 0.5 * G   (the image holds -2c);   dot: gx = G.   G is staged through
//                LDS to undo the fragment / even-odd layout and written with coalesced stores.
// Register budget: Dp/2 (x fragments) + Dp/2 (G accumulators) + ~60 -> 4-wave workgroups; Dp = 256 runs one wave per
// SIMD (512 registers), Dp <= 128 two.  Dp = 512: two workgroups per row block (blockIdx.z), each repeats the S sweep
// and produces one 256-wide half of the dims (3 instead of 2 units of MFMA work).
// ------------------------------------------------------------------------------------------------
}  // namespace
namespace vqi {
struct CeBwdParams {
    const float *x;
    long long x_rs, x_hs;
    const float *packed;
    long long pk_hs;
    unsigned pk_bytes;
    long long M;
    int K, D, ntiles, vec_x;
    const float *lse;  // [H * M]
    const long long *target;
    long long tgt_rs, tgt_hs;
    const float *coef;  // one float on the device: upstream gradient / number of non-ignored rows
    const float *cb;    // natural codebook (the target's term is added in the finalize)
    long long cb_hs;
    const float *tgt_logit;  // [H * M] similarity of the target code (vq_softmax_stats_f32 output, scale 1)
    float *gx;
    long long gx_rs, gx_hs;
};
// live variant: `packed` = the codes the forward searched, `live_packed` the image of the codes at backward time (same K, D,
// metric and byte size); `cb` is then the natural LIVE codebook
struct CeBwdLiveParams : CeBwdParams {
    const float *live_packed;
    long long live_pk_hs;
};
}  // namespace vqi
namespace {
using vqi::CeBwdParams;
using vqi::CeBwdLiveParams;
#ifndef VQ_CE_LIVE_WAVES
#define VQ_CE_LIVE_WAVES 8  // waves per workgroup of the live kernel at Dp <= 128 (4: A/B builds)
#endif

template <int DP>
struct CeGeo {
    static constexpr int V = DP >= 128 ? 4 : DP / 32;  // floats per A-fragment read (positions 4i+e / 2i+e / i)
    static constexpr int NH = DP > 256 ? DP / 256 : 1; // the G accumulators of Dp = 512 do not fit beside the x fragments:
                                                       // blockIdx.z picks a 256-wide half of the packed positions
    static constexpr int WID = DP / NH;                // positions (= dims) one workgroup produces
    static constexpr int NJ = WID / (32 * V);          // 128-wide (V = 4) position blocks
    static constexpr int NACC = WID / 32;              // 32x32 accumulators of G
    static constexpr int GS = WID + 4;                 // staging row stride (floats): 16-B aligned rows, 2-way conflicts on the column writes
};

// finalize of the cross-entropy backward: rows [r_begin, r_end) of a 32-row block, positions [pos0, pos0 + WID) -- the staged
// G values (natural dim order, row stride GS) + the per-row terms -> gx.  `stg`, `srs`, `stg_t`, `stg_f`: the block's LDS staging.
template <int WID, bool EUCLID>
__device__ __forceinline__ void ce_finish_rows(const CeBwdParams &p, int head, long long row0, int r_begin, int r_end, int pos0,
                                               const float *stg, const float *srs, const int *stg_t, const float *stg_f, int lane) {
    constexpr int GS = WID + 4;
    const float *xh = p.x + (long long)head * p.x_hs;
    const int nrows = r_end;
    float *gxh = p.gx + (long long)head * p.gx_hs;
    const float *cbh = p.cb + (long long)head * p.cb_hs;
    const bool vec_g = p.vec_x && (p.gx_rs % 4 == 0) && (p.gx_hs % 4 == 0) && (((uintptr_t)p.gx & 15) == 0) &&
                       (p.cb_hs % 4 == 0) && (((uintptr_t)p.cb & 15) == 0);
    if (vec_g) {
        constexpr int RB = 8;                      // rows in flight: the x / codebook loads are latency-bound
        constexpr int NV = (WID + 255) / 256;      // float4 per lane and row
        for (int rr0 = r_begin; rr0 < nrows; rr0 += RB) {
            f32x4 xv[RB][NV], cv[RB][NV];
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const int rr = (rr0 + k < nrows) ? rr0 + k : nrows - 1;
                const float *xr = xh + (row0 + rr) * p.x_rs + pos0;
                const int t = stg_t[rr];
                const float *cr = cbh + (long long)(t < 0 ? 0 : t) * p.D + pos0;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int dl = 4 * (lane + 64 * j);
                    const bool in = dl < WID && pos0 + dl < p.D;
                    xv[k][j] = in ? *(const f32x4 *)(xr + dl) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                    cv[k][j] = in ? *(const f32x4 *)(cr + dl) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                }
            }
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                if (rr0 + k < nrows) {
                    const float sr = srs[rr0 + k], f = stg_f[rr0 + k];
                    float *gr = gxh + (row0 + rr0 + k) * p.gx_rs + pos0;
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        const int dl = 4 * (lane + 64 * j);
                        if (dl < WID && pos0 + dl < p.D) {
                            const f32x4 gv = *(const f32x4 *)(stg + (rr0 + k) * GS + dl);
                            const f32x4 x4 = xv[k][j], c4 = cv[k][j];
                            f32x4 o;
                            if (EUCLID) {
                                o.x = fmaf(f, c4.x - x4.x, fmaf(x4.x, sr, 0.5f * gv.x));
                                o.y = fmaf(f, c4.y - x4.y, fmaf(x4.y, sr, 0.5f * gv.y));
                                o.z = fmaf(f, c4.z - x4.z, fmaf(x4.z, sr, 0.5f * gv.z));
                                o.w = fmaf(f, c4.w - x4.w, fmaf(x4.w, sr, 0.5f * gv.w));
                            } else {
                                o.x = fmaf(f, c4.x, gv.x);
                                o.y = fmaf(f, c4.y, gv.y);
                                o.z = fmaf(f, c4.z, gv.z);
                                o.w = fmaf(f, c4.w, gv.w);
                            }
                            *(f32x4 *)(gr + dl) = o;
                        }
                    }
                }
            }
        }
    } else {
        for (int rr = r_begin; rr < nrows; ++rr) {
            const float sr = srs[rr], f = stg_f[rr];
            const int t = stg_t[rr];
            const float *xr = xh + (row0 + rr) * p.x_rs;
            const float *cr = cbh + (long long)(t < 0 ? 0 : t) * p.D;
            float *gr = gxh + (row0 + rr) * p.gx_rs;
            for (int dl = lane; dl < WID && pos0 + dl < p.D; dl += 64) {
                const int d = pos0 + dl;
                const float gv = stg[rr * GS + dl];
                gr[d] = EUCLID ? fmaf(f, cr[d] - xr[d], fmaf(xr[d], sr, 0.5f * gv)) : fmaf(f, cr[d], gv);
            }
        }
    }
}

// Live codes (vq_ce_backward_live_f32), Dp <= 256.  Four tile buffers: 133 120 B at Dp = 256 (the finalize staging, 134 656 B,
// still aliases them), 135 168 / 139 264 / 147 456 B at Dp = 128 / 64 / 32 -- one workgroup per CU.  Dp = 256 is the one-wave
// kernel as it stands (one wave per SIMD either way; the roles kernel's three buffers cannot be doubled).  Dp <= 128 has two
// 4-wave workgroups per CU without live codes; with them ONE 8-wave workgroup walks 256 rows and shares each pair of tiles,
// so the two waves per SIMD and their 256 registers stay.
template <int DP>
struct CeLiveGeo {
    static constexpr int WAVES = DP <= 128 ? VQ_CE_LIVE_WAVES : 4;
    static constexpr size_t TILES_B = (size_t)4 * Geo<DP, WAVES>::BUF_F4 * 16;
    static constexpr size_t PRO_B = (size_t)WAVES * 32 * Geo<DP, WAVES>::XS * 4;      // prologue staging (load_x_fragments)
    static constexpr size_t STG_B = (size_t)WAVES * (32 * CeGeo<DP>::GS + 96) * 4;    // finalize staging
    static constexpr size_t LDS_B = TILES_B > STG_B ? (TILES_B > PRO_B ? TILES_B : PRO_B) : (STG_B > PRO_B ? STG_B : PRO_B);
    static_assert(DP <= 256 && LDS_B <= 160 * 1024, "four tile buffers of Dp = 512 do not fit");
};

// The one-wave kernel.  LIVE: the weights come from the codes the forward searched (p.packed: S sweep, zero-distance fix-up,
// sum of the ratios; lse / tgt_logit belong to them too), what they are multiplied with from the codes as they are now
// (p.live_packed: the A operands of the G sweep; p.cb, the finalize's c_target, is the natural live codebook) -- the gradient
// autograd gives after an EMA step has rewritten the codebook through .data.  A second tile ring (buffers 2, 3: same geometry,
// tile index and parity) takes the live image, both tiles of a step are issued together; the MFMA chains and their order
// are the non-live kernel's, so with live == searched codes the result is its result bit for bit.
template <int DP, int METRIC, bool LIVE = false, int WAVES = 4>
__global__ void __launch_bounds__(WAVES * 64, (DP <= 128 && WAVES == 4 ? 2 : 1))
vq_ce_backward(const std::conditional_t<LIVE, CeBwdLiveParams, CeBwdParams> p) {
    using G = Geo<DP, WAVES>;
    using CG = CeGeo<DP>;
    constexpr int RS = G::RS, RS4 = G::RS4, SUB = G::SUB, NG = DP / 8, V = CG::V, NJ = CG::NJ, NACC = CG::NACC;
    constexpr int WID = CG::WID;
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    const int pos0 = (CG::NH > 1) ? (int)blockIdx.z * WID : 0;  // first packed position (= dim) of this workgroup
    constexpr float LOG2E = 1.4426950408889634f;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4 *tile4 = (f32x4 *)smem;
    lds_f32x4 *tile4_lds = (lds_f32x4 *)smem;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const long long row0 = ((long long)blockIdx.x * WAVES + wave) * 32;
    const float *xh = p.x + (long long)head * p.x_hs;

    STAMP(0);
    float xf[DP / 2];
    float xn0 = 0.0f;
    load_x_fragments<G::CH, G::XS, DP / G::CH, EUCLID>(xh, p.x_rs, p.M, p.D, p.vec_x, row0, true, smem, wave, lane, xf, xn0);
    __syncthreads();  // the staging region is about to be reused as codebook tile buffers
    STAMP(1);

    const long long row = row0 + c;
    const bool row_ok = row < p.M;
    const float *pk = p.packed + (long long)head * p.pk_hs;
    const float b_aug = h ? 1.0f : xn0;

    int tgt = -1;
    float lse2 = 0.0f;  // lse * log2(e)
    float tlog = 0.0f;  // similarity of the target code
    if (row_ok) {
        const long long tv = p.target[(long long)head * p.tgt_hs + row * p.tgt_rs];
        tgt = (tv >= 0 && tv < p.K) ? (int)tv : -1;
        lse2 = p.lse[(long long)head * p.M + row] * LOG2E;
        tlog = p.tgt_logit[(long long)head * p.M + row];
    }
    const float coef_row = (tgt >= 0) ? p.coef[0] : 0.0f;  // ignored / padding rows contribute nothing
    // The sweep below handles the softmax part  coef * p_k  of d loss / d sim_k for every code alike; the one-hot part
    // (-coef at k = target) is a rank-one term per row and is added in the finalize from the natural codebook.

    f32x16 gacc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j) gacc[j] = (f32x16){0};
    float sum_ratio = 0.0f;

    auto stage = [&](int tile, int buf) {
#pragma unroll
        for (int i = 0; i < (G::TILE_CHUNKS + WAVES - 1) / WAVES; ++i) {
            const int ck = i * WAVES + wave;
            if (ck < G::TILE_CHUNKS)
                lds_dma16(pk, p.pk_bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16,
                          tile4_lds + buf * G::BUF_F4 + ck * 64);
            if constexpr (LIVE) {
                if (ck < G::TILE_CHUNKS)
                    lds_dma16(p.live_packed + (long long)head * p.live_pk_hs, p.pk_bytes, lane * 16, (tile * G::TILE_F4 + ck * 64) * 16,
                              tile4_lds + (2 + buf) * G::BUF_F4 + ck * 64);
            }
        }
    };

    stage(0, 0);
    __syncthreads();
    for (int t = 0; t < p.ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < p.ntiles) stage(t + 1, cur ^ 1);
#pragma unroll 1
        for (int st = 0; st < SUB; ++st) {
            const int u = t * SUB + st;
            if (u * kTileCodes >= p.K) break;  // workgroup-uniform
            const f32x4 *tb = tile4 + cur * G::BUF_F4 + st * (kTileCodes * RS4);
            const f32x4 *tg = LIVE ? tb + 2 * G::BUF_F4 : tb;  // the tile the G sweep multiplies with
            // ---- S sweep
            f32x16 acc = {0};
            {
                const f32x4 *ta = tb + c * RS4 + h;
                f32x4 a[NG];
                const float cnv = EUCLID ? ((const float *)tb)[c * RS + DP] : 0.0f;
                mfma_prefetch<DP>(a, ta);
                mfma_range<DP, 0, NG>(acc, a, ta, xf);
                if (EUCLID) {
                    const float a_aug = h ? cnv : 1.0f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
                }
            }
            // ---- epilogue: acc[r] <- ratio (Euclid) / d loss / d sim (dot) of code u*32 + 4h + (r&3) + 8(r>>2)
            // (softmax part only; two values per step so that the multiplies / fma / add pack into v_pk_* instructions)
            const int cbase = u * kTileCodes + 4 * h;
            const bool tail = u * kTileCodes + kTileCodes > p.K;
            bool degenerate = false;  // some squared distance <= 0: ATen gives those codes the subgradient 0
            if (EUCLID) {
                float tm = vmin3(acc[0], acc[1], acc[2]);
                tm = vmin3(tm, acc[3], acc[4]);
                tm = vmin3(tm, acc[5], acc[6]);
                tm = vmin3(tm, acc[7], acc[8]);
                tm = vmin3(tm, acc[9], acc[10]);
                tm = vmin3(tm, acc[11], acc[12]);
                tm = vmin3(tm, acc[13], acc[14]);
                tm = fminf(tm, acc[15]);
                degenerate = __any(tm <= 0.0f);
            }
            const f32x2 ncoef = {-coef_row, -coef_row}, pcoef = {coef_row, coef_row};
            const f32x2 nl2e = {-LOG2E, -LOG2E}, pl2e = {LOG2E, LOG2E}, nlse = {-lse2, -lse2};
            f32x2 sum2 = {0.0f, 0.0f};
            // the weights of codes r, r + 1 of this lane, in place
            auto weights = [&](int r) {
                const f32x2 tv = {acc[r], acc[r + 1]};
                f32x2 v;
                if (EUCLID) {
                    const f32x2 tc = {vmax3(tv.x, 0.0f, 0.0f), vmax3(tv.y, 0.0f, 0.0f)};
                    const f32x2 rs = {__builtin_amdgcn_rsqf(tc.x), __builtin_amdgcn_rsqf(tc.y)};  // 1 / dist
                    const f32x2 ex = __builtin_elementwise_fma(tc * rs, nl2e, nlse);               // (-dist - lse) log2 e
                    const f32x2 pr = {__builtin_amdgcn_exp2f(ex.x), __builtin_amdgcn_exp2f(ex.y)};
                    v = (pr * rs) * ncoef;  // gs / sim with sim = -dist; inf / nan where dist == 0 (fixed below)
                } else {
                    const f32x2 ex = __builtin_elementwise_fma(tv, pl2e, nlse);
                    const f32x2 pr = {__builtin_amdgcn_exp2f(ex.x), __builtin_amdgcn_exp2f(ex.y)};
                    v = pr * pcoef;
                }
                acc[r] = v.x;
                acc[r + 1] = v.y;
                if (EUCLID) sum2 += v;
            };
            // ---- G sweep: gacc[J*V + e][pos-in-chunk i, row] += Cimg[code(r, half)][128J + 4i + e] * acc[r]
            const float *trow = (const float *)tg + (4 * h) * RS + V * c + pos0;
            // (wave-uniform; through readfirstlane so that it stays a run-time scalar: the dot variant otherwise gets one copy of
            // the sub-tile body per kind of tile and spills)
            const int plain_i = __builtin_amdgcn_readfirstlane((int)!(degenerate || tail));
            const bool plain_tile = plain_i != 0;
            if (!(V == 4 && plain_tile)) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) weights(r);
                float sum_u = sum2.x + sum2.y;
                // rare wave-uniform fix-ups, kept out of the straight-line path: zero distances and the codebook's tail
                if (degenerate || tail) {
                    asm volatile("" ::: "memory");  // keep this a branch (16 selects per lane otherwise)
                    sum_u = 0.0f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[r];
                        if (!(__builtin_fabsf(v) < __builtin_inff())) v = 0.0f;            // 1 / 0: subgradient 0
                        if (cbase + (r & 3) + 8 * (r >> 2) >= p.K) v = 0.0f;               // padding codes
                        acc[r] = v;
                        sum_u += v;
                    }
                }
                if (EUCLID) sum_ratio += sum_u;
            }
            if constexpr (V == 4) {
                // fragment reads run PF steps ahead of their MFMAs, order pinned (same scheme as mfma_range)
                constexpr int NSEQ = NJ * 16, PF = 4;
                auto frag = [&](int n) -> f32x4 {
                    const int J = n >> 4, r = n & 15;
                    return *(const f32x4 *)(trow + ((r & 3) + 8 * (r >> 2)) * RS + 128 * J);
                };
                f32x4 af[NSEQ];
#pragma unroll
                for (int n = 0; n < PF; ++n) af[n] = frag(n);
                auto gstep = [&](int n) {
                    if (n + PF < NSEQ) af[n + PF] = frag(n + PF);
                    const int J = n >> 4, r = n & 15;
                    gacc[J * 4 + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].x, acc[r], gacc[J * 4 + 0], 0, 0, 0);
                    gacc[J * 4 + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].y, acc[r], gacc[J * 4 + 1], 0, 0, 0);
                    gacc[J * 4 + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].z, acc[r], gacc[J * 4 + 2], 0, 0, 0);
                    gacc[J * 4 + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].w, acc[r], gacc[J * 4 + 3], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                };
                // Round 3: on a plain tile (no zero distance, no padding codes: all but a handful) the weights are computed two
                // codes at a time INSIDE the G sweep's MFMA stream -- its first 16 steps consume acc[0], acc[1], ... in order, so
                // only the first pair's sqrt / exp latency is exposed (at Dp >= 256 this kernel runs one wave per SIMD: nothing
                // else covers its vector work).  ONE copy of the MFMA stream serves both kinds of tile.
                if (plain_tile) weights(0);
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    if (plain_tile && r + 2 < 16) weights(r + 2);  // (ahead of the MFMAs that need the previous pair)
                    gstep(r);
                    gstep(r + 1);
                }
                if (EUCLID && plain_tile) sum_ratio += sum2.x + sum2.y;
#pragma unroll
                for (int n = 16; n < NSEQ; ++n) gstep(n);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float *ap = trow + ((r & 3) + 8 * (r >> 2)) * RS;
                    if (V == 2) {
                        const float a0 = ap[0], a1 = ap[1];
                        gacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, acc[r], gacc[0], 0, 0, 0);
                        gacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, acc[r], gacc[1], 0, 0, 0);
                    } else {
                        gacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[0], acc[r], gacc[0], 0, 0, 0);
                    }
                    if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound the fragment reads in flight
                }
            }
        }
        __syncthreads();  // next tile landed, everybody is done reading this one
    }

    STAMP(2);
    // ---------------- finalize: fragment layout -> natural rows through LDS ----------------
    // (the loop's last barrier guarantees nobody reads the tile buffers any more)
    constexpr int GS = CG::GS;
    float *stg = smem + wave * (32 * GS + 96);
    float *srs = stg + 32 * GS;
    // per row: sum of the ratios (Euclid) and the one-hot term's factor  f:  gx += f * (c_target - x)  (Euclid,
    // f = -coef / dist_t = coef / sim_t, 0 at dist_t == 0)   or   gx += f * c_target  (dot, f = -coef)
    int *stg_t = (int *)(srs + 32);
    float *stg_f = srs + 64;
    if (EUCLID) sum_ratio += __shfl_xor(sum_ratio, 32);
    if (h == 0) {
        srs[c] = sum_ratio;
        stg_t[c] = tgt;
        stg_f[c] = EUCLID ? ((tlog < 0.0f) ? coef_row / tlog : 0.0f) : -coef_row;
    }
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const int J = a / V, e = a % V;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 8 * (r >> 2) + 4 * h + (r & 3);       // MFMA i index held by this lane's register r
            const int pos = 32 * V * J + V * i + e;             // position in this workgroup's part of the packed row
            const int p8 = pos & 7;
            const int dim = (pos & ~7) + (p8 < 4 ? 2 * p8 : 2 * (p8 - 4) + 1);
            stg[c * GS + dim] = gacc[a][r];
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private region: in-order LDS, no barrier needed
    const int nrows = (p.M - row0 >= 32) ? 32 : (int)(p.M - row0);
    ce_finish_rows<WID, EUCLID>(p, head, row0, 0, nrows, pos0, stg, srs, stg_t, stg_f, lane);
    STAMP(3);
}

// ------------------------------------------------------------------------------------------------
// Dp = 256, round 3: the two contractions on two WAVES.  The one-wave kernel above needs Dp/2 x fragments + Dp/2 gradient
// accumulators + ~80 registers = one wave per SIMD, and nothing covers that wave's epilogue (sqrt / exp), LDS waits and
// barriers.  Here every 32-row block belongs to a pair: wave S (waves 0..3) keeps the x fragments, runs the S sweep of
// tile s and the softmax epilogue, and hands the 16 weights per lane to wave G (waves 4..7) through a 4-KiB LDS slot -- the
// accumulator registers of S are, as they stand, the B operands of G's MFMAs, so the slot is a plain register image (float4
// per lane, no layout change); G keeps the gradient accumulators and runs the G sweep of tile s - 1 out of the same staged
// tile.  128 (+1) MFMAs per wave and step on both sides, ~150 registers each -> two waves per SIMD (one S + one G: the
// vector work of S's epilogue sits beside G's pure MFMA stream).  Three tile buffers (tile s + 1 arriving, s for S, s - 1 for
// G), two slots per pair (written in step s, read in step s + 1; the step barrier orders both directions).
// Results are the one-wave kernel's bit for bit (same chains; the G accumulators see the tiles in the same order).
// ------------------------------------------------------------------------------------------------
struct CeRolesGeo {
    static constexpr int DP = 256, NB = 4;                         // row blocks (wave pairs) per workgroup
    using G = Geo<DP, 8>;
    static constexpr int NTB = 3;                                  // tile buffers
    static constexpr int SLOT_F = 64 * 16;                         // floats per slot
    static constexpr int TILES_F = NTB * G::BUF_F4 * 4;
    static constexpr int SWEEP_F = TILES_F + NB * 2 * SLOT_F;
    static constexpr int STG_F = 32 * CeGeo<DP>::GS + 96;          // finalize staging per row block
    static constexpr int LDS_F = SWEEP_F > NB * STG_F ? SWEEP_F : NB * STG_F;
};

template <int METRIC>
__global__ void __launch_bounds__(512, 1) vq_ce_backward_roles(const CeBwdParams p) {
    constexpr int DP = 256, WAVES = 8;
    using RG = CeRolesGeo;
    using G = RG::G;
    using CG = CeGeo<DP>;
    constexpr int RS = G::RS, RS4 = G::RS4, NG = DP / 8, NJ = CG::NJ, NACC = CG::NACC;
    static_assert(CG::V == 4 && CG::NH == 1 && G::SUB == 1, "roles kernel: one 32-code sub-tile per staged tile, 4 floats per A read");
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    constexpr float LOG2E = 1.4426950408889634f;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4 *tile4 = (f32x4 *)smem;
    lds_f32x4 *tile4_lds = (lds_f32x4 *)smem;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const bool role_g = wave >= RG::NB;       // (wave-uniform)
    const int blk = wave & (RG::NB - 1);
    const long long row0 = ((long long)blockIdx.x * RG::NB + blk) * 32;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float *pk = p.packed + (long long)head * p.pk_hs;
    const int T = p.ntiles;
    f32x4 *slot4 = (f32x4 *)(smem + RG::TILES_F + blk * 2 * RG::SLOT_F) + lane;  // this pair's two slots, this lane's float4 column

    auto stage = [&](int tile, int buf) { stage_tile<G, WAVES>(pk, p.pk_bytes, tile, tile4_lds + buf * G::BUF_F4, wave, lane); };
    // finalize staging of this pair's row block (aliases the tile buffers / slots once the sweep is over)
    float *stg = smem + blk * RG::STG_F;
    float *srs = stg + 32 * CG::GS;
    int *stg_t = (int *)(srs + 32);
    float *stg_f = srs + 64;

    stage(0, 0);  // (the rows are staged in the third tile buffer: tile 0 travels during the prologue)
    if (!role_g) {
        // ================= wave S: x fragments, S sweep, softmax weights =================
        float xf[DP / 2];
        float xn0 = 0.0f;
        load_x_fragments<G::CH, G::XS, DP / G::CH, EUCLID>(xh, p.x_rs, p.M, p.D, p.vec_x, row0, true, smem + 2 * G::BUF_F4 * 4, blk,
                                                           lane, xf, xn0);
        __syncthreads();
        const long long row = row0 + c;
        const bool row_ok = row < p.M;
        const float b_aug = h ? 1.0f : xn0;
        int tgt = -1;
        float lse2 = 0.0f, tlog = 0.0f;
        if (row_ok) {
            const long long tv = p.target[(long long)head * p.tgt_hs + row * p.tgt_rs];
            tgt = (tv >= 0 && tv < p.K) ? (int)tv : -1;
            lse2 = p.lse[(long long)head * p.M + row] * LOG2E;
            tlog = p.tgt_logit[(long long)head * p.M + row];
        }
        const float coef_row = (tgt >= 0) ? p.coef[0] : 0.0f;
        float sum_ratio = 0.0f;
        int buf = 0;
#ifndef VQ_EXP_CE_NO_PRIO
        // S shares its SIMD with a G wave: at equal priority the two MFMA streams interleave and S's sqrt / exp work starts only
        // when BOTH are through; with S ahead, its epilogue runs beside G's remaining MFMAs
        __builtin_amdgcn_s_setprio(2);
#endif
        for (int s = 0; s <= T; ++s) {
            const int nbuf = buf == RG::NTB - 1 ? 0 : buf + 1;
            if (s + 1 < T) stage(s + 1, nbuf);
            if (s < T) {
                const f32x4 *tb = tile4 + buf * G::BUF_F4;
                f32x16 acc = {0};
                {
                    const f32x4 *ta = tb + c * RS4 + h;
                    f32x4 a[NG];
                    const float cnv = EUCLID ? ((const float *)tb)[c * RS + DP] : 0.0f;
                    mfma_prefetch<DP>(a, ta);
                    mfma_range<DP, 0, NG>(acc, a, ta, xf);
                    if (EUCLID) {
                        const float a_aug = h ? cnv : 1.0f;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
                    }
                }
                const int cbase = s * kTileCodes + 4 * h;
                const bool tail = s * kTileCodes + kTileCodes > p.K;
                bool degenerate = false;
                if (EUCLID) {
                    float tm = vmin3(acc[0], acc[1], acc[2]);
                    tm = vmin3(tm, acc[3], acc[4]);
                    tm = vmin3(tm, acc[5], acc[6]);
                    tm = vmin3(tm, acc[7], acc[8]);
                    tm = vmin3(tm, acc[9], acc[10]);
                    tm = vmin3(tm, acc[11], acc[12]);
                    tm = vmin3(tm, acc[13], acc[14]);
                    tm = fminf(tm, acc[15]);
                    degenerate = __any(tm <= 0.0f);
                }
                const f32x2 ncoef = {-coef_row, -coef_row}, pcoef = {coef_row, coef_row};
                const f32x2 nl2e = {-LOG2E, -LOG2E}, pl2e = {LOG2E, LOG2E}, nlse = {-lse2, -lse2};
                f32x2 sum2 = {0.0f, 0.0f};
#pragma unroll
                for (int r = 0; r < 16; r += 2) {  // (the same arithmetic as vq_ce_backward's `weights`)
                    const f32x2 tv = {acc[r], acc[r + 1]};
                    f32x2 v;
                    if (EUCLID) {
                        const f32x2 tc = {vmax3(tv.x, 0.0f, 0.0f), vmax3(tv.y, 0.0f, 0.0f)};
                        const f32x2 rs = {__builtin_amdgcn_rsqf(tc.x), __builtin_amdgcn_rsqf(tc.y)};
                        const f32x2 ex = __builtin_elementwise_fma(tc * rs, nl2e, nlse);
                        const f32x2 pr = {__builtin_amdgcn_exp2f(ex.x), __builtin_amdgcn_exp2f(ex.y)};
                        v = (pr * rs) * ncoef;
                    } else {
                        const f32x2 ex = __builtin_elementwise_fma(tv, pl2e, nlse);
                        const f32x2 pr = {__builtin_amdgcn_exp2f(ex.x), __builtin_amdgcn_exp2f(ex.y)};
                        v = pr * pcoef;
                    }
                    acc[r] = v.x;
                    acc[r + 1] = v.y;
                    if (EUCLID) sum2 += v;
                }
                float sum_u = sum2.x + sum2.y;
                if (degenerate || tail) {
                    asm volatile("" ::: "memory");  // keep this a branch
                    sum_u = 0.0f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[r];
                        if (!(__builtin_fabsf(v) < __builtin_inff())) v = 0.0f;
                        if (cbase + (r & 3) + 8 * (r >> 2) >= p.K) v = 0.0f;
                        acc[r] = v;
                        sum_u += v;
                    }
                }
                if (EUCLID) sum_ratio += sum_u;
                f32x4 *sl = slot4 + (s & 1) * (RG::SLOT_F / 4);
#pragma unroll
                for (int g = 0; g < 4; ++g) sl[g * 64] = (f32x4){acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            }
            buf = nbuf;
            __syncthreads();  // tile s + 1 landed; the weights of tile s are visible; G is done with slot (s - 1) & 1 and tile s - 1
        }
        // (the loop's last barrier: nobody reads tiles or slots any more)
        if (EUCLID) sum_ratio += __shfl_xor(sum_ratio, 32);
        if (h == 0) {
            srs[c] = sum_ratio;
            stg_t[c] = tgt;
            stg_f[c] = EUCLID ? ((tlog < 0.0f) ? coef_row / tlog : 0.0f) : -coef_row;
        }
    } else {
        // ================= wave G: gradient accumulators, G sweep one tile behind =================
        __syncthreads();  // (S waves: end of the row prologue)
        f32x16 gacc[NACC];
#pragma unroll
        for (int j = 0; j < NACC; ++j) gacc[j] = (f32x16){0};
        int buf = 0, pbuf = 0;
        for (int s = 0; s <= T; ++s) {
            const int nbuf = buf == RG::NTB - 1 ? 0 : buf + 1;
            if (s + 1 < T) stage(s + 1, nbuf);
            if (s >= 1) {
                const f32x4 *tb = tile4 + pbuf * G::BUF_F4;
                const f32x4 *sl = slot4 + ((s - 1) & 1) * (RG::SLOT_F / 4);
                float w[16];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 t = sl[g * 64];
                    w[4 * g + 0] = t.x; w[4 * g + 1] = t.y; w[4 * g + 2] = t.z; w[4 * g + 3] = t.w;
                }
                const float *trow = (const float *)tb + (4 * h) * RS + 4 * c;
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
                    gacc[J * 4 + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].x, w[r], gacc[J * 4 + 0], 0, 0, 0);
                    gacc[J * 4 + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].y, w[r], gacc[J * 4 + 1], 0, 0, 0);
                    gacc[J * 4 + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].z, w[r], gacc[J * 4 + 2], 0, 0, 0);
                    gacc[J * 4 + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].w, w[r], gacc[J * 4 + 3], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            pbuf = buf;
            buf = nbuf;
            __syncthreads();
        }
        // fragment layout -> natural rows (same mapping as the one-wave kernel)
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const int J = a / 4, e = a % 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 8 * (r >> 2) + 4 * h + (r & 3);
                const int pos = 128 * J + 4 * i + e;
                const int p8 = pos & 7;
                const int dim = (pos & ~7) + (p8 < 4 ? 2 * p8 : 2 * (p8 - 4) + 1);
                stg[c * CG::GS + dim] = gacc[a][r];
            }
        }
    }
    __syncthreads();  // staged gradients and per-row terms of every pair are in LDS
    // each wave of a pair finishes 16 of the pair's 32 rows
    int nrows = (p.M - row0 >= 32) ? 32 : (int)(p.M - row0);
    const int r_begin = role_g ? 16 : 0;
    if (!role_g && nrows > 16) nrows = 16;
    ce_finish_rows<DP, EUCLID>(p, head, row0, r_begin, nrows, 0, stg, srs, stg_t, stg_f, lane);
}

// ------------------------------------------------------------------------------------------------
// Dp = 512, round 3: FOUR roles per 32-row block.  The S sweep is cut in two like the wave-pair search (S1: dims 0..255 from
// C = 0, hands the 32 x 32 accumulator to S2 through LDS; S2: dims 256..511, the augmented column, the softmax weights) and
// the gradient in two halves of the packed positions (G1: 0..255, G2: 256..511; both consume S2's weights).  128 MFMAs per
// role and tile, <= 200 registers each -> two waves per SIMD, and the S sweep runs ONCE per row block (the one-wave kernel
// repeats it in each of its two workgroups: 3 units of MFMA work instead of 2).
// Pipeline: step s -- S1 on tile s, S2 on tile s - 1, G1 / G2 on tile s - 2; one workgroup barrier per step.
// LDS: the S roles read their tiles as half rows through four half-tile buffers (the wave-pair kernel's scheme: lo(s + 1) and
// hi(s) arrive during step s); a CU has no room for the three further half tiles the G roles would need, so G1 / G2 read
// their A fragments straight from the packed image (L2): a lane's float4 = 4 consecutive positions of one code row, 32 lanes
// = 512 contiguous bytes, eight loads in flight.  S1 -> S2: one slot per quad + the wave-pair kernel's flag protocol;
// S2 -> G: two slots per quad (written in step s, read in step s + 1).
// Waves 0..3 are S1, S2, G1, G2 of quad 0 and waves 4..7 G1, G2, S1, S2 of quad 1: with round-robin wave placement every
// SIMD hosts one S and one G wave.
// ------------------------------------------------------------------------------------------------
// buffer_load_dwordx4 into registers: `base` + voffset (per lane, bytes) + soffset (scalar, bytes); out-of-range reads return 0
__device__ __forceinline__ f32x4 buffer_load16(const float *base, unsigned bytes, int voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)bytes, 0x00020000);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, soffset, 0);
    return __builtin_bit_cast(f32x4, v);
#else
    (void)base; (void)bytes; (void)voffset; (void)soffset;
    return (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#endif
}

struct CeRoles512Geo {
    static constexpr int HD = 256, NQ = 2;                       // dims per S wave / positions per G wave; quads per workgroup
    static constexpr int RSH = HD + 4, HT_F = 32 * RSH;          // half-tile buffers: 32 half rows, stride 260 floats
    static constexpr int TILES_F = 4 * HT_F;
    static constexpr int SLOT_F = 64 * 16;
    static constexpr int SLOTA_F = NQ * SLOT_F;                  // S1 -> S2: one slot per quad
    static constexpr int SLOTW_F = NQ * 2 * SLOT_F;              // S2 -> G: two slots per quad
    static constexpr int MISC_F = NQ * 32 + 8;                   // S1's part of |x|^2 + flags
    static constexpr int SWEEP_F = TILES_F + SLOTA_F + SLOTW_F + MISC_F;
    static constexpr int STG_F = 32 * (HD + 4);                  // finalize staging per G wave
    static constexpr int ROWT_F = 96;                            // per-row terms per quad
    static constexpr int FIN_F = 2 * NQ * STG_F + NQ * ROWT_F;
    static constexpr int LDS_F = SWEEP_F > FIN_F ? SWEEP_F : FIN_F;
    static_assert(LDS_F * 4 <= 160 * 1024, "one workgroup per CU");
};

template <int METRIC>
__global__ void __launch_bounds__(512, 1) vq_ce_backward_roles512(const CeBwdParams p) {
    using RG = CeRoles512Geo;
    constexpr int HD = RG::HD, NS = HD / 2, NG = HD / 8, RSH = RG::RSH, RSH4 = RSH / 4, HT_F = RG::HT_F;
    constexpr int RSP = 512 + 4;  // packed row stride, floats
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    constexpr float LOG2E = 1.4426950408889634f;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *slot_a_all = smem + RG::TILES_F;
    float *slot_w_all = slot_a_all + RG::SLOTA_F;
    float *xn_a = slot_w_all + RG::SLOTW_F;                   // [2 quads][32]
    volatile int *flags = (volatile int *)(xn_a + RG::NQ * 32);  // [2 quads] (+ pad)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const int quad = wave >> 2;
    const int role = (wave + 2 * quad) & 3;  // 0 S1, 1 S2, 2 G1, 3 G2
    const int sw = quad * 2 + (role & 1);    // index among the 4 S waves (DMA shares) / the 4 G waves (staging regions)
    const long long row0 = ((long long)blockIdx.x * RG::NQ + quad) * 32;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float *pk = p.packed + (long long)head * p.pk_hs;
    const int T = p.ntiles;
    f32x4 *slot_a = (f32x4 *)(slot_a_all + quad * RG::SLOT_F) + lane;
    f32x4 *slot_w = (f32x4 *)(slot_w_all + quad * 2 * RG::SLOT_F) + lane;

    // one half tile: 32 half rows of 1 KiB by LDS-DMA, eight per S wave
    auto dma_half = [&](int tile, int half, int buf) {
        float *dst = smem + (half * 2 + buf) * HT_F;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = sw + 4 * i;
            lds_dma16(pk, p.pk_bytes, lane * 16, ((tile * 32 + r) * RSP + half * HD) * 4, (lds_f32x4 *)(dst + r * RSH));
        }
    };
    // finalize staging (aliases the tile buffers once the sweep is over)
    float *rowt = smem + 2 * RG::NQ * RG::STG_F + quad * RG::ROWT_F;  // this quad's per-row terms
    float *srs = rowt;
    int *stg_t = (int *)(rowt + 32);
    float *stg_f = rowt + 64;

    if (role < 2) {
        // ================= S1 / S2: this wave's half of the rows -> fragments =================
        const int dbase = role * HD;
        float xf[NS];
        float xn0 = 0.0f;
        {
            // S1 walks its part of the d-ordered |x|^2 chain, S2 continues it below (row chunks of 32 dims, as in vq_search_pair512)
            constexpr int CH = 32, XS = 64 + 4;
            load_x_fragments<CH, XS, HD / CH, EUCLID>(xh + dbase, p.x_rs, p.M, p.D - dbase, p.vec_x, row0, role == 0, smem, sw, lane, xf, xn0);
            if (EUCLID && role == 0 && h == 0) xn_a[quad * 32 + c] = xn0;
        }
        if (tid < 8) flags[tid] = 0;  // (wave 0 is quad 0's S1; before the barrier)
        __syncthreads();  // (1) the staging region becomes tile buffers; S1's chain values are visible to S2
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) asm volatile("" : "+v"(xf[s2]));  // (cut the register pairing of the swaps)
        dma_half(0, 0, 0);
        __syncthreads();  // (2) lo(0) landed

        if (role == 0) {
            // ---------------- S1: dims 0..255, one tile ahead of S2 ----------------
            for (int s = 0; s <= T + 1; ++s) {
                if (s < T) {
                    const f32x4 *ta = (const f32x4 *)(smem + (s & 1) * HT_F) + c * RSH4 + h;
                    f32x4 a[NG];
                    f32x16 acc = {0};
                    mfma_prefetch<HD>(a, ta);
                    mfma_range<HD, 0, 1>(acc, a, ta, xf);
                    if (s + 1 < T) dma_half(s + 1, 0, (s + 1) & 1);
                    dma_half(s, 1, s & 1);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_range<HD, 1, NG>(acc, a, ta, xf);
                    while (flags[quad] < s) __builtin_amdgcn_s_sleep(1);  // S2 has taken accumulator s - 1 out of the slot
#pragma unroll
                    for (int j = 0; j < 4; ++j) slot_a[j * 64] = (f32x4){acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
                }
                __syncthreads();
            }
        } else {
            // ---------------- S2: dims 256..511, the augmented column, the softmax weights; one tile behind S1 ----------------
            const long long row = row0 + c;
            const bool row_ok = row < p.M;
            int tgt = -1;
            float lse2 = 0.0f, tlog = 0.0f;
            if (row_ok) {
                const long long tv = p.target[(long long)head * p.tgt_hs + row * p.tgt_rs];
                tgt = (tv >= 0 && tv < p.K) ? (int)tv : -1;
                lse2 = p.lse[(long long)head * p.M + row] * LOG2E;
                tlog = p.tgt_logit[(long long)head * p.M + row];
            }
            const float coef_row = (tgt >= 0) ? p.coef[0] : 0.0f;
            float b_aug = 1.0f;
            if (EUCLID) {  // continue the |x|^2 chain over this wave's registers (the other k-parity comes from the partner lane)
                float xn = xn_a[quad * 32 + c];
                const int partner = (lane ^ 32) * 4;
#pragma unroll
                for (int s0 = 0; s0 < NS; s0 += 4) {
                    float t1[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) t1[k] = __uint_as_float(__builtin_amdgcn_ds_bpermute(partner, __float_as_uint(xf[s0 + k])));
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        xn = __builtin_fmaf(xf[s0 + k], xf[s0 + k], xn);
                        xn = __builtin_fmaf(t1[k], t1[k], xn);
                    }
                    asm volatile("" : "+v"(xn));
                }
                b_aug = h ? 1.0f : xn;
            }
            float sum_ratio = 0.0f;
#ifndef VQ_EXP_CE_NO_PRIO
            __builtin_amdgcn_s_setprio(2);  // (ahead of the G wave on its SIMD: the softmax work then runs beside G's MFMAs)
#endif
            // step 0: nothing to consume yet -- this wave's share of the copies
            if (T > 1) dma_half(1, 0, 1);
            dma_half(0, 1, 0);
            __syncthreads();
            for (int s = 1; s <= T + 1; ++s) {
                if (s <= T) {
                    const int tile = s - 1;
                    const float cnv = EUCLID ? pk[(long long)(tile * 32 + c) * RSP + 512] : 0.0f;
                    const f32x4 *ta = (const f32x4 *)(smem + (2 + (tile & 1)) * HT_F) + c * RSH4 + h;
                    f32x4 a[NG];
                    f32x16 acc;
                    mfma_prefetch<HD>(a, ta);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 t = slot_a[j * 64];
                        acc[4 * j] = t.x; acc[4 * j + 1] = t.y; acc[4 * j + 2] = t.z; acc[4 * j + 3] = t.w;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane == 0) flags[quad] = s;  // the slot may be overwritten
                    mfma_range<HD, 0, 2>(acc, a, ta, xf);
                    if (s < T) {
                        if (s + 1 < T) dma_half(s + 1, 0, (s + 1) & 1);
                        dma_half(s, 1, s & 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_range<HD, 2, NG>(acc, a, ta, xf);
                    if (EUCLID) {
                        const float a_aug = h ? cnv : 1.0f;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
                    }
                    // ---- softmax weights of tile `tile`, in place (the same arithmetic as vq_ce_backward's `weights`)
                    const int cbase = tile * kTileCodes + 4 * h;
                    const bool tail = tile * kTileCodes + kTileCodes > p.K;
                    bool degenerate = false;
                    if (EUCLID) {
                        float tm = vmin3(acc[0], acc[1], acc[2]);
                        tm = vmin3(tm, acc[3], acc[4]);
                        tm = vmin3(tm, acc[5], acc[6]);
                        tm = vmin3(tm, acc[7], acc[8]);
                        tm = vmin3(tm, acc[9], acc[10]);
                        tm = vmin3(tm, acc[11], acc[12]);
                        tm = vmin3(tm, acc[13], acc[14]);
                        tm = fminf(tm, acc[15]);
                        degenerate = __any(tm <= 0.0f);
                    }
                    const f32x2 ncoef = {-coef_row, -coef_row}, pcoef = {coef_row, coef_row};
                    const f32x2 nl2e = {-LOG2E, -LOG2E}, pl2e = {LOG2E, LOG2E}, nlse = {-lse2, -lse2};
                    f32x2 sum2 = {0.0f, 0.0f};
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const f32x2 tv = {acc[r], acc[r + 1]};
                        f32x2 v;
                        if (EUCLID) {
                            const f32x2 tc = {vmax3(tv.x, 0.0f, 0.0f), vmax3(tv.y, 0.0f, 0.0f)};
                            const f32x2 rs = {__builtin_amdgcn_rsqf(tc.x), __builtin_amdgcn_rsqf(tc.y)};
                            const f32x2 ex = __builtin_elementwise_fma(tc * rs, nl2e, nlse);
                            const f32x2 pr = {__builtin_amdgcn_exp2f(ex.x), __builtin_amdgcn_exp2f(ex.y)};
                            v = (pr * rs) * ncoef;
                        } else {
                            const f32x2 ex = __builtin_elementwise_fma(tv, pl2e, nlse);
                            const f32x2 pr = {__builtin_amdgcn_exp2f(ex.x), __builtin_amdgcn_exp2f(ex.y)};
                            v = pr * pcoef;
                        }
                        acc[r] = v.x;
                        acc[r + 1] = v.y;
                        if (EUCLID) sum2 += v;
                    }
                    float sum_u = sum2.x + sum2.y;
                    if (degenerate || tail) {
                        asm volatile("" ::: "memory");  // keep this a branch
                        sum_u = 0.0f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float v = acc[r];
                            if (!(__builtin_fabsf(v) < __builtin_inff())) v = 0.0f;
                            if (cbase + (r & 3) + 8 * (r >> 2) >= p.K) v = 0.0f;
                            acc[r] = v;
                            sum_u += v;
                        }
                    }
                    if (EUCLID) sum_ratio += sum_u;
                    f32x4 *sl = slot_w + (tile & 1) * (RG::SLOT_F / 4);
#pragma unroll
                    for (int g = 0; g < 4; ++g) sl[g * 64] = (f32x4){acc[4 * g + 0], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                }
                __syncthreads();
            }
            // (past the sweep's last barrier: tiles and slots are dead)
            if (EUCLID) sum_ratio += __shfl_xor(sum_ratio, 32);
            if (h == 0) {
                srs[c] = sum_ratio;
                stg_t[c] = tgt;
                stg_f[c] = EUCLID ? ((tlog < 0.0f) ? coef_row / tlog : 0.0f) : -coef_row;
            }
        }
    } else {
        // ================= G1 / G2: positions pos0 .. pos0 + 255 of the gradient, two tiles behind S1 =================
        const int pos0 = (role & 1) * HD;
        __syncthreads();  // (1)
        __syncthreads();  // (2)
        f32x16 gacc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) gacc[j] = (f32x16){0};
        // this lane's float4 of fragment n of a tile: code row 4h + (r & 3) + 8 (r >> 2), positions pos0 + 128 J + 4c .. + 3
        const int voff = ((4 * h) * RSP + pos0 + 4 * c) * 4;  // bytes
        __syncthreads();  // (step 0)
        __syncthreads();  // (step 1)
        for (int s = 2; s <= T + 1; ++s) {
            const int tile = s - 2;
            const f32x4 *sl = slot_w + (tile & 1) * (RG::SLOT_F / 4);
            float w[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 t = sl[g * 64];
                w[4 * g + 0] = t.x; w[4 * g + 1] = t.y; w[4 * g + 2] = t.z; w[4 * g + 3] = t.w;
            }
            constexpr int NSEQ = 32, PF = 8;
            const int tbase = tile * 32 * RSP * 4;  // bytes (scalar)
            auto frag = [&](int n) -> f32x4 {
                const int J = n >> 4, r = n & 15;
                return buffer_load16(pk, p.pk_bytes, voff, tbase + (((r & 3) + 8 * (r >> 2)) * RSP + 128 * J) * 4);
            };
            f32x4 af[NSEQ];
#pragma unroll
            for (int n = 0; n < PF; ++n) af[n] = frag(n);
#pragma unroll
            for (int n = 0; n < NSEQ; ++n) {
                if (n + PF < NSEQ) af[n + PF] = frag(n + PF);
                const int J = n >> 4, r = n & 15;
                gacc[J * 4 + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].x, w[r], gacc[J * 4 + 0], 0, 0, 0);
                gacc[J * 4 + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].y, w[r], gacc[J * 4 + 1], 0, 0, 0);
                gacc[J * 4 + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].z, w[r], gacc[J * 4 + 2], 0, 0, 0);
                gacc[J * 4 + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[n].w, w[r], gacc[J * 4 + 3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        }
        // fragment layout -> natural rows (same mapping as the one-wave kernel), into this wave's staging region
        float *stg = smem + sw * RG::STG_F;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int J = a / 4, e = a % 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 8 * (r >> 2) + 4 * h + (r & 3);
                const int pos = 128 * J + 4 * i + e;
                const int p8 = pos & 7;
                const int dim = (pos & ~7) + (p8 < 4 ? 2 * p8 : 2 * (p8 - 4) + 1);
                stg[c * (HD + 4) + dim] = gacc[a][r];
            }
        }
    }
    __syncthreads();  // staged gradients and per-row terms are in LDS
    // S1 + G1 finish the rows of positions 0..255 (16 rows each), S2 + G2 those of 256..511
    {
        const int half = role & 1;
        const float *stg = smem + (quad * 2 + half) * RG::STG_F;
        int nrows = (p.M - row0 >= 32) ? 32 : (int)(p.M - row0);
        const int r_begin = role >= 2 ? 16 : 0;
        if (role < 2 && nrows > 16) nrows = 16;
        ce_finish_rows<HD, EUCLID>(p, head, row0, r_begin, nrows, half * HD, stg, srs, stg_t, stg_f, lane);
    }
}

// scalar fallback for the similarity matrix (D > 512, cross-check): one thread per (row, code)
template <int METRIC>
__global__ void __launch_bounds__(256) vq_sims_simple(const float *__restrict__ x, long long x_rs, long long x_hs,
                                                      const float *__restrict__ cb, long long cb_hs, long long M, int K,
                                                      int D, float *__restrict__ sims, long long sims_rs, long long sims_hs) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= M * K) return;
    const long long row = gid / K;
    const int k = (int)(gid % K);
    const int head = blockIdx.y;
    const float *xr = x + (long long)head * x_hs + row * x_rs;
    const float *cr = cb + (long long)head * cb_hs + (long long)k * D;
    float acc = 0.0f;
    if (METRIC == VQ_METRIC_EUCLID) {
        float xn = 0.0f, cn = 0.0f;
        for (int d = 0; d < D; ++d) {
            xn = fmaf(xr[d], xr[d], xn);
            cn = fmaf(cr[d], cr[d], cn);
            acc = fmaf(xr[d], -2.0f * cr[d], acc);
        }
        acc = fmaf(1.0f, xn, acc);
        acc = fmaf(cn, 1.0f, acc);
        acc = -sqrtf(acc < 0.0f ? 0.0f : acc);  // clamp_min_(0) keeps NaN
    } else {
        for (int d = 0; d < D; ++d) acc = fmaf(xr[d], cr[d], acc);
    }
    sims[(long long)head * sims_hs + row * sims_rs + k] = acc;
}

