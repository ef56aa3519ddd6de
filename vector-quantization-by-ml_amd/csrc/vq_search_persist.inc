// vq_search_persist.inc -- inference search with the gather of block b hidden inside the sweep of block b + 1.
// Included by vq_kernels.hip after vq_search.inc (same SearchParams, fragment pipeline, epilogue, tie rule).
//
// Why: at K = 1024 a row block's life is 26 k cycles of prologue, 551 k of sweep and 21 k of fused finalize (gather
// codebook[idx], store 256 KiB of quantized rows): the finalize is 3.5 % of the kernel, it is an HBM write burst (every CU
// stores at the same time), and nothing runs on the matrix pipe meanwhile.  For the plain inference call (one stage, no
// straight-through, no loss) the finalize is a pure copy -- out[row] = codebook[idx[row]] -- that needs no vector arithmetic:
// a scalar row address, one global load and one store per row.  So the workgroup becomes PERSISTENT over its row blocks
// (block id, + grid size, ...) and copies the rows of the block it has just searched one row per sub-tile during the NEXT
// block's sweep: a load at sub-tile n, the matching store at sub-tile n + 1 (the data has long arrived), the winner index
// read from LDS one sub-tile ahead.  Two VMEM instructions, one v_readfirstlane and a few scalar instructions per sub-tile
// beside 129 MFMAs; only the last block of a workgroup pays the finalize in the open.
// Everything that decides results (prologue chain, sweep, tie rule) is the code of vq_search_mfma<.., MULTI = 0>.
// TRAIN (round 3): the training-mode call -- straight-through output x + (c - x) and / or the squared error sum -- copies the
// same way: the deferred step of a row loads the code row AND the x row (read again: the fragment registers of that block are
// gone), does the finalize's arithmetic on the float4 and stores; the wave's squared-error partial is written once at the end.
// ------------------------------------------------------------------------------------------------
// SCREEN (Dp = 256, Euclid, plain inference call): an fp16 screen with a proven error bound, exact rule for the rest
// ------------------------------------------------------------------------------------------------
// The fp32 sweep runs v_mfma_f32_32x32x2_f32 (4 096 FLOP in 64 cycles); v_mfma_f32_32x32x16_f16 does 32 768 FLOP in 32.
// The screened sweep holds every code as ONE fp16 value ct = fp16(s_c c') (c' = -2c as packed, s_c a power of two per head that
// puts max |c'| s_c in [2^13, 2^14)) and every row as an fp16 pair of X = s_x x (s_x a second power of two per head, max |c_i|
// s_x in [2^7, 2^8)): xh = fp16(X), xl = fp16(X - xh).  It accumulates ct * xh + ct * xl (2 fp16 MFMAs per 16 dims: 32 per
// 32 x 32 sub-tile instead of 129 fp32 ones), starting from |c|^2 s_c s_x (the fp32 chain of the packed image times an exact
// power of two) in the accumulator, and divides the values it keeps by sg = s_c s_x once, after the sweep.  The rounding of
// the codes is the one first-order error left; it is a property of the codebook, which the pack kernel measures (E_c below)
// instead of bounding it.  Each lane keeps the three lowest screened values of its codes -- as KEYS: the value with the
// accumulator register's number in its 4 low mantissa bits, item (6) below -- and the sub-tiles of the two lowest, from which
// their codes are decoded after the sweep (vq_scr_keys.h).  A row whose two lowest screened values
// are further apart than the bound below can only have the screened winner as its exact winner.  The other rows are decided
// by a second kernel on the same stream (vq_resolve_rows_kernel), none of them inside the sweep kernel, where one wave's
// exact chains would hold the other seven at the next tile barrier.  The sweep puts them on one of two lists, which share one
// array of H M uint32 entries head * M + row in the workspace (counts: scr_count[0], scr_count[1], zeroed by
// vq_pack_scr_kernel):
//  * rescore list, filled from the BACK of the array: the row's candidates are among the <= 4 codes its two lane halves
//    track.  Between the two kernels the row's idx element (an int64 the second pass overwrites) holds them as four 16-bit
//    codes, 0xFFFF for an empty slot (the persistent kernel is chosen for K <= 3072); the second pass runs the exact chain for
//    each (rescore_batch);
//  * full-search list, filled from the FRONT: a lane half holds more candidates than it tracks, or the row is not eligible;
//    the second pass searches all K codes again (exact_row_euclid).  idx holds the screened argmin meanwhile.
// A row is on one list at most, so the two ends never meet and the array needs no more room than one list did.  Results
// are those of the fp32 kernel bit for bit.
//
// The bound.  u = 2^-24; for a row x (fp32 chain xn = d-ordered sum of squares) and code c (fp32 chain cn), c' = -2c as
// packed (exact), Q = sum_k x_k c'_k in real arithmetic, nx = sqrt(xn), nc = sqrt(max cn) over the codebook, L = 2 nx nc.
// The chains xn, cn are sums of non-negative terms, relative error <= gamma_256 = 256u / (1 - 256u) < 1.6e-5, so
// |x| <= nx (1 + 8e-6) and Cauchy-Schwarz gives sum_k |x_k c'_k| <= 2 |x| |c| <= L * 1.0001.  Scaling by s_c, s_x, sg = s_c s_x
// is exact (powers of two; the pack kernel flags a head whose exponents leave +-62, where a scaled value could leave the
// normal range).  Per head, from the pack kernel: E_c = max_k |s_c c'_k - ct_k|_2 and l1 = max_k sum_i |ct_ki|, both over
// the value ct the MFMA sees (an fp16 below 2^-14 counted as 0), both rounded up.
//  S = screened value (accumulator / sg), E = exact fp32 value minus xn (the kernels' D = fl(fl(P + xn) + cn), P the
//  k-ordered fmaf chain).
//  (1) codes: |sum_k (s_c c'_k - ct_k) X_k| <= E_c |X|_2 (Cauchy-Schwarz); over sg: <= (E_c / s_c) |x| <= (E_c / s_c) nx
//      (1 + 8e-6).  ct_k = fp16(s_c c'_k) by round to nearest, |ct_k| < 2^14 + 8: finite.
//  (2) row split: X = xh + xl + r.  |X| >= 2^-14: |X - xh| <= 2^-11 |X| (round to nearest, 11-bit significand), X - xh exact
//      in fp32, and, where that is >= 2^-14 too, |r| <= 2^-11 |X - xh| <= 2^-22 |X|.  Eligible rows have |X_k| <= 2^15
//      (below), so xh is finite.  sum_k |ct_k| 2^-22 |X_k| <= 2^-22 |ct|_2 |X|_2 with |ct|_2 <= s_c |c'| + E_c: over sg
//      <= 2^-22 (1.0001 L + (E_c / s_c) nx (1 + 8e-6)).
//  (3) fp16 subnormals: the ISA does not promise that the MFMA keeps fp16 operands below 2^-14, nor that the conversion
//      does; assume either may give 0.  A part of X (xh, or xl) below 2^-14 then costs < 2^-14, whatever was done to it (kept:
//      <= 2^-25 of rounding): per element <= 2 * 2^-14 in all, sum_k |ct_k| 2^-13 <= 2^-13 l1; over sg: 2^-13 l1 / sg.
//      On the code side the pack kernel stores the flushed ct and measures E_c against it: inside (1).
//  (4) fp16 x fp16 products are exact in fp32 (22 significant bits, >= 2^-28); the MFMAs add the 2 D = 512 products and the
//      initial cn sg in an undocumented order: any order of 512 additions is within gamma_512 < 3.052e-5 of the sum of the
//      absolute values, here <= cn sg + |ct|_2 |X|_2 (1 + 2^-10): over sg <= 3.052e-5 (1.002 L + 1.002 (E_c / s_c) nx + nc^2).
//      fp32 partial sums below 2^-126 may be flushed: < 513 * 2^-126 < 2^-116, over sg; the division by sg rounds only a
//      result below 2^-126: <= 2^-149.
//  (5) the exact side: |P - Q| <= gamma_256 sum |x_k c'_k| <= 1.53e-5 L * 1.0001 (k-ordered fmaf chain), the two
//      additions of xn and cn add <= u (|P + xn| + |D|) <= 1.2e-7 (L + xn + nc^2) * 1.0001; fp32 denormals in the chain
//      < 258 * 2^-149.
//  (6) the key: what the kernel keeps, compares and thresholds is not the accumulator A but its KEY, A with the 4 low mantissa
//      bits replaced by the accumulator register's number (vq_scr_keys.h), so S = key / sg.  |key - A| <= 15 ulp(A): for a
//      normal A <= 15 * 2^-23 |A| < 1.789e-6 |A|, and |A| is within gamma_512 of the sum of the absolute values of (4):
//      |A| / sg <= (1 + 3.1e-5) (nc^2 + 1.002 L + 1.002 (E_c / s_c) nx), so the key costs <= 1.789e-6 nc^2 + 1.793e-6 L +
//      1.793e-6 (E_c / s_c) nx.  A subnormal A (|A| < 2^-126, the exact 0 of a zero code that wins included) moves by
//      <= 15 * 2^-149 < 2^-145, over sg: inside the 2^-116 / sg of (4), which was claimed for 513 * 2^-126 = 2^-116.997
//      (the rest, 511 * 2^-126, is 2^19 times the key's share).  The padding codes' start value (finite instead of +inf,
//      last sub-tile) is no code's screened value and stays above every threshold (vq_scr_keys.h).
//  => |S - E| <= 1.0001 (E_c / s_c) nx + 4.81e-5 L + 3.25e-5 nc^2 + 1.21e-7 xn + (2^-13 l1 + 2^-116) / sg + 2^-140 =: delta_0
//     ((1): 1 + 8e-6, (2): 2.4e-7, (4): 3.06e-5, (6): 1.8e-6 on the first term, 1.0000406 in all; (2): 2.4e-7, (4): 3.058e-5,
//     (5): 1.542e-5, (6): 1.793e-6 on L, 4.804e-5 in all; (4): 3.052e-5, (5): 1.2e-7, (6): 1.789e-6 on nc^2, 3.243e-5 in all).
//     The kernel uses delta = 1.1 delta_0: the factor covers the rounding of delta's own evaluation (a dozen fp32
//     operations on non-negative terms, < 2e-6) and of the two fp32 sqrt.
// A row is CERTAIN when (b1, b2 = lowest and second lowest keys / sg over distinct codes of the row)
//  * b2 - b1 > 2 delta + w, w = 2^-20 (|b1| + xn + delta): every other code j has E_j >= b2 - delta > b1 + delta + w >=
//    E_win + w, so D_j - D_win > w >= 2^-21 D_win * 2: the two squared distances cannot share a correctly rounded sqrt (two
//    values more than 2^-21 apart relative never do -- the fp32 sweep's tie rule), the screened argmin is the unique winner;
//  * b1 + xn > 2 delta: the winner's D is positive, so no code clamps to 0 (several clamped codes would tie at 0 and the
//    lowest index, not the screened argmin, would win);
//  * eligibility: xn s_x^2 <= 2^30 (no element of X reaches fp16's largest value; NaN / inf rows fail this test and take the
//    exact path, which follows the non-finite rule) and max cn <= 2^100, the codebook is not flagged non-finite, and the
//    pack kernel has not flagged the head (an exponent outside +-62, or a real code whose cn sg is not 0 or a normal fp32).
// The winning distance is then known only through the screen, so calls that request it (`best`) keep the fp32 sweep.
constexpr int kScrRowBytes = 528;                              // one code: 16 groups of 16 dims x 2 x 16 B of fp16, + 16 B pad
constexpr int kScrTileBytes = kTileCodes * kScrRowBytes + 128;  // 32 codes + their 32 fp32 |c|^2 s_c s_x
constexpr int kScrCnOffset = kTileCodes * kScrRowBytes;
constexpr int kScrChunks = (kScrTileBytes + 1023) / 1024;      // 1-KiB wave copies per tile (over-copy into the next tile)
// Behind the ntiles tiles of a head, 32-bit words, ntiles of each: max |c|^2 of the tile's real codes (unscaled), E_c and l1
// of the tile (scaled units, rounded up), the tile's flag, max |c'_i| of the tile (written by vq_scr_absmax_kernel, from which
// every workgroup of the pack kernel derives the head's exponents); then the two exponents e_c, e_x (s_c = 2^e_c, s_x = 2^e_x).
constexpr int kScrTailMcn = 0, kScrTailEc = 1, kScrTailL1 = 2, kScrTailFlag = 3, kScrTailAbs = 4, kScrTailExp = 5;
constexpr int kScrMaxExp = 62;
// The room of an image (kScrTileRoom per tile and 4 bytes behind, scr_image_bytes: vq_search_plan.h) is still that of the
// bf16-pair image this one replaced.  The image uses the front of the room; the rest is unused and never read.
static_assert(kScrChunks * 1024 + 4 * kScrTailExp + 8 <= kScrTileRoom + 4, "tiles, over-copy and tail fit the room of one tile");
// the MFMA group (of 16 per sub-tile) after which waves 4..7 run the sweep's epilogue; waves 0..3 run it after group 0
// (8 = half a sub-tile; profiles/cfg2_stagger.md has the figures of 5, 6, 8, 10, 12 and 14, profiles/cfg2_tagged_keys.md
// those of 4, 5, 6, 8 and 10 with the shorter epilogue of the tagged keys)
#ifndef VQ_SCR_LATE_GROUP
#define VQ_SCR_LATE_GROUP 8
#endif
constexpr int kScrLateGroup = VQ_SCR_LATE_GROUP;
// groups of 16 dims whose A fragments are read ahead of their MFMAs (3 or 4: profiles/cfg2_fp16_screen.md)
#ifndef VQ_SCR_PF
#define VQ_SCR_PF 3
#endif
#include "vq_resolve_plan.h"
#include "vq_scr_keys.h"
// The control block behind the images (SearchParams::scr_count points at it), 32-bit words: [0] rows on the full-search list,
// [1] rows on the rescore list, [2] exit ticket of the second pass, [4] and [5] the two counts of the previous call (no kernel
// reads them: tests and diagnostics do); from word kScrRowTicketWord on one ticket per split full-search row, and from
// kScrSlotWord on kResolveMaxSplit 8-byte result slots for each (vq_resolve_plan.h).  vq_pack_scr_kernel zeroes the block; the
// second pass leaves words 0..2 and every ticket zero again (vq_resolve_rows_kernel), so an image that outlives the call needs
// no per-call zeroing.  (kScrCtrlBytes: vq_search_plan.h)
constexpr int kScrTicketWord = 2, kScrLastCountsWord = 4, kScrRowTicketWord = 8;
constexpr int kScrSlotWord = kScrRowTicketWord + (int)kResolveMaxSplitRows;
static_assert(kScrSlotWord % 2 == 0 && (kScrSlotWord + 2 * (int)(kResolveMaxSplitRows * kResolveMaxSplit)) * 4 <= kScrCtrlBytes,
              "8-byte slots, inside the block");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

// hi = fp16(v), lo = fp16(v - hi) of 8 floats (plain casts: v_cvt_f16_f32 under the default round-to-nearest mode, never
// v_cvt_pkrtz_f16_f32)
__device__ __forceinline__ void split_f16x2(const f32x8 &v, f16x8 &hi, f16x8 &lo) {
    hi = __builtin_convertvector(v, f16x8);
    const f32x8 r = v - __builtin_convertvector(hi, f32x8);
    lo = __builtin_convertvector(r, f16x8);
}
// 2^e as a float, -126 <= e <= 127
__device__ __forceinline__ float scr_pow2(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

// max |c'_i| of every 32-code tile of the fp32 packed image (padding rows hold zeros), NaN ignored: word kScrTailAbs of the
// image's tail.  Grid (tiles, heads), 256 threads, ahead of vq_pack_scr_kernel on the stream.
template <int DP>
__global__ void __launch_bounds__(256) vq_scr_absmax_kernel(const float *__restrict__ packed, long long pk_hs, int ntiles,
                                                            char *__restrict__ img, long long img_hs) {
    constexpr int RS = DP + 4;
    static_assert(DP == 256, "8 threads per code, 32 floats each");
    const int t = blockIdx.x, c = threadIdx.x >> 3, part = threadIdx.x & 7;
    const float *prow = packed + (long long)blockIdx.y * pk_hs + (long long)(t * kTileCodes + c) * RS + 32 * part;
    float m = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x4 v = *(const f32x4 *)(prow + 4 * i);
        m = fmaxf(m, fmaxf(fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), fmaxf(__builtin_fabsf(v.z), __builtin_fabsf(v.w))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        ((float *)(img + (long long)blockIdx.y * img_hs + (long long)ntiles * kScrTileBytes))[kScrTailAbs * ntiles + t] =
            fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The fp16 image of a Dp = 256 Euclid codebook, built from its fp32 packed image (values c' = -2c, |c|^2 at float Dp, +inf for
// the padding rows).  Per 32-code tile: row c at c * 528 bytes, for each group s of 16 dims ct[16s .. 16s+7], ct[16s+8 ..
// 16s+15] (16 B each: one ds_read_b128 is one MFMA's A fragment), ct = fp16(s_c c') with values below 2^-14 stored as 0; then
// the 32 |c|^2 s_c s_x of the tile; behind the tiles the words described at kScrTailMcn.  Every workgroup derives the head's
// exponents from the tiles' max |c'_i| (vq_scr_absmax_kernel): e_c = 13 - floor(log2 max |c'|), e_x = e_c - 5 (max |c_i| =
// max |c'| / 2 in [2^7, 2^8)); both 0 for an all-zero codebook, both 0 and the head flagged when one leaves +-kScrMaxExp
// (non-finite or subnormal maxima included).  Grid (tiles, heads), 256 threads: 8 per code.
// One workgroup also zeroes the control block `ctrl` (kScrCtrlBytes): the counts of the two lists of rows for the second pass
// (vq_resolve_rows_kernel) and its exit ticket.
template <int DP>
__global__ void __launch_bounds__(256) vq_pack_scr_kernel(const float *__restrict__ packed, long long pk_hs, int K, int ntiles,
                                                          char *__restrict__ img, long long img_hs, unsigned *__restrict__ ctrl) {
    static_assert(DP == 256, "the screened sweep is built for Dp = 256");
    static_assert(kScrCtrlBytes % (256 * 16) == 0, "whole rounds of 16 B per thread");
    // ahead of the sweep on the stream: both lists of rows for the second pass start empty
    if (blockIdx.x == 0 && blockIdx.y == 0) {
#pragma unroll
        for (int i = 0; i < kScrCtrlBytes / (256 * 16); ++i) ((uint4 *)ctrl)[i * 256 + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    }
    constexpr int RS = DP + 4;
    const int t = blockIdx.x, c = threadIdx.x >> 3, part = threadIdx.x & 7;
    const int k = t * kTileCodes + c;
    const float *prow = packed + (long long)blockIdx.y * pk_hs + (long long)k * RS;
    char *himg = img + (long long)blockIdx.y * img_hs;
    char *tile = himg + (long long)t * kScrTileBytes;
    float *tail = (float *)(himg + (long long)ntiles * kScrTileBytes);
    char *dst = tile + c * kScrRowBytes;
    // the head's exponents (the same in every workgroup of the head)
    float hmax = 0.0f;
    for (int i = 0; i < ntiles; ++i) hmax = fmaxf(hmax, tail[kScrTailAbs * ntiles + i]);
    int e_c = 0, e_x = 0;
    unsigned flag = 0u;
    if (hmax != 0.0f) {
        const int lg = (int)((__float_as_uint(hmax) >> 23) & 0xFFu) - 127;  // floor(log2 hmax) of a normal value
        e_c = 13 - lg;
        e_x = e_c - 5;
        if (e_c > kScrMaxExp || e_c < -kScrMaxExp || e_x > kScrMaxExp || e_x < -kScrMaxExp) {
            e_c = e_x = 0;
            flag = 1u;
        }
    }
    const float s_c = scr_pow2(e_c), sg = scr_pow2(e_c + e_x);
    float d2 = 0.0f, l1 = 0.0f;  // this thread's part of |s_c c' - ct|^2 and of sum |ct|
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
        const int s = 2 * part + ss;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int g = 2 * s + h;  // 8-dim group of the fp32 image: evens first, then odds
            const f32x4 ev = *(const f32x4 *)(prow + 8 * g), od = *(const f32x4 *)(prow + 8 * g + 4);
            const f32x8 v = (f32x8){ev.x, od.x, ev.y, od.y, ev.z, od.z, ev.w, od.w} * s_c;
            f16x8 ct = __builtin_convertvector(v, f16x8);
            f32x8 cf = __builtin_convertvector(ct, f32x8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (__builtin_fabsf(cf[e]) < 0x1p-14f) {  // what the MFMA may see as 0 is stored as 0
                    ct[e] = (_Float16)0.0f;
                    cf[e] = 0.0f;
                }
                const float d = v[e] - cf[e];  // exact in fp32
                d2 = fmaf(d, d, d2);
                l1 += __builtin_fabsf(cf[e]);
            }
            *(f16x8 *)(dst + 32 * s + 16 * h) = ct;
        }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        d2 += __shfl_xor(d2, o);
        l1 += __shfl_xor(l1, o);
    }
    // (threads 8c of the first 4 waves hold the values: maxima over the workgroup through LDS)
    __shared__ float red_cn[kTileCodes], red_ec[kTileCodes], red_l1[kTileCodes];
    __shared__ unsigned red_fl[kTileCodes];
    if (part == 0) {
        *(f32x4 *)(dst + 512) = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        const float cn = prow[DP];  // the packed |c|^2 (+inf for padding rows)
        const float cs = cn * sg;
        *(float *)(tile + kScrCnOffset + 4 * c) = cs;
        const bool real = k < K;
        // rounded up: the chains and the sqrt are within 2e-5 of the real values
        red_cn[c] = real ? prow[DP + 2] : 0.0f;
        red_ec[c] = real ? sqrtf(d2) * (1.0f + 0x1p-10f) : 0.0f;
        red_l1[c] = real ? l1 * (1.0f + 0x1p-10f) : 0.0f;
        red_fl[c] = (real && cn < __builtin_inff() && !(cs == 0.0f ? cn == 0.0f : (cs >= 0x1p-126f && cs < __builtin_inff()))) ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = 0.0f, ec = 0.0f, ml1 = 0.0f;
        for (int i = 0; i < kTileCodes; ++i) {
            m = (red_cn[i] > m || red_cn[i] != red_cn[i]) ? red_cn[i] : m;
            ec = (red_ec[i] > ec || red_ec[i] != red_ec[i]) ? red_ec[i] : ec;
            ml1 = (red_l1[i] > ml1 || red_l1[i] != red_l1[i]) ? red_l1[i] : ml1;
            flag |= red_fl[i];
        }
        tail[kScrTailMcn * ntiles + t] = m;
        tail[kScrTailEc * ntiles + t] = ec;
        tail[kScrTailL1 * ntiles + t] = ml1;
        ((unsigned *)tail)[kScrTailFlag * ntiles + t] = flag;
        if (t == 0) {
            ((int *)tail)[kScrTailExp * ntiles] = e_c;
            ((int *)tail)[kScrTailExp * ntiles + 1] = e_x;
        }
    }
}

// The exact rule (oracle/vq_oracle.c; repair_nonfinite_rows) for ONE row and the codes kbeg <= k < kend, Euclid, by one wave,
// 64 codes at a time, one per lane: the k-ordered fmaf chain over the dims, + |x|^2, + |c|^2, clamp_min(0), correctly rounded
// sqrt; first NaN, else first minimum, then the 6-step butterfly (NaN first, value, index): every lane returns the wave's
// (bn = a NaN was met, bv, bi).  better_euclid is the order of that rule.  `rowbuf` = the row in LDS (Dp floats, zeros behind
// D); its |x|^2 chain in the prologue's order (d-ordered fmaf from 0) runs beside the distance chain of every pass, as in
// rescore_batch: a second, independent chain in the same loop costs no time, a loop of its own ahead of the first load did.
// A lane walking its own code row of the packed image reads 16 B of a different cache line than every other lane: 64 tag
// look-ups per load instruction, 66 k per row at K = 1024, which is what such a search costs (30 us on one CU, measured).
// So the codes come through `stage` (wave-private LDS, 64 rows of kExStageRow floats), 32 dims at a time: 8 lanes load the
// 128 B of one code, 8 codes per instruction, one chunk ahead of the arithmetic, and each lane reads its own code's 32 dims
// back (20 us per row, measured; two codes per lane and 128 codes per pass were no faster).  LDS operations of one wave
// execute in order, so the wave needs no barrier between its stores and loads.
constexpr int kExChunk = 32;                // dims per staged chunk
constexpr int kExStageRow = kExChunk + 4;   // floats per staged code (144 B: 16 lanes' ds_read_b128 cover the 64 banks once)
constexpr int kExCodes = 64;                // codes per wave and pass
// 8 dims of the k-ordered fmaf chain: `xa`, `xb` = dims 8 q .. 8 q + 7 of the row, `ce`, `co` = the even and the odd dims of
// that group of the packed image (values -2c)
__device__ __forceinline__ float exact_chain8(float acc, const f32x4 &xa, const f32x4 &xb, const f32x4 &ce, const f32x4 &co) {
    acc = fmaf(xa.x, ce.x, acc);
    acc = fmaf(xa.y, co.x, acc);
    acc = fmaf(xa.z, ce.y, acc);
    acc = fmaf(xa.w, co.y, acc);
    acc = fmaf(xb.x, ce.z, acc);
    acc = fmaf(xb.y, co.z, acc);
    acc = fmaf(xb.z, ce.w, acc);
    acc = fmaf(xb.w, co.w, acc);
    return acc;
}
// the chain's end: + |x|^2, + |c|^2, clamp_min_(0) (keeps NaN), correctly rounded sqrt
__device__ __forceinline__ float exact_dist(float acc, float xn, float cn) {
    float tt = fmaf(1.0f, xn, acc);
    tt = fmaf(cn, 1.0f, tt);
    tt = (tt < 0.0f) ? 0.0f : tt;
    return sqrtf(tt);
}
__device__ __forceinline__ bool better_euclid(bool on, float ov, int oi, bool bn, float bv, int bi) {
    if (on != bn) return on;
    if (bn) return oi < bi;
    return (ov < bv) || (ov == bv && oi < bi);
}
template <int DP>
__device__ __forceinline__ void exact_row_euclid(const float *rowbuf, float *stage, const float *pk, int kbeg, int kend, int lane,
                                                 bool &bn, float &bv, int &bi) {
    constexpr int RS = DP + 4, CD = kExChunk, SR = kExStageRow, NCH = DP / CD, NL = kExCodes / 8;
    static_assert(DP % CD == 0, "whole chunks");
    bv = __builtin_inff();
    bi = (kbeg + lane < kend) ? kbeg + lane : 0x7FFFFFFF;
    bn = false;
    const int piece = lane & 7, sub = lane >> 3;  // this lane loads float4 `piece` of the chunk of codes kb + sub + 8 i
    const float *cr = stage + lane * SR;
#pragma clang loop unroll(disable)
    for (int kb = kbeg; kb < kend; kb += kExCodes) {  // (wave-uniform)
        const int k = kb + lane;
        const bool ok = k < kend;
        const float *src[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int kk = kb + sub + 8 * i;
            src[i] = pk + (long long)(kk < kend ? kk : kend - 1) * RS + 4 * piece;
        }
        f32x4 g[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) g[i] = *(const f32x4 *)(src[i]);
        const float cn = pk[(long long)(ok ? k : kend - 1) * RS + DP];
        float acc = 0.0f, xn = 0.0f;
#pragma clang loop unroll(disable)
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int i = 0; i < NL; ++i) *(f32x4 *)(stage + (sub + 8 * i) * SR + 4 * piece) = g[i];
            if (ch + 1 < NCH) {
#pragma unroll
                for (int i = 0; i < NL; ++i) g[i] = *(const f32x4 *)(src[i] + (ch + 1) * CD);
            }
#pragma unroll
            for (int q = 0; q < CD / 8; ++q) {
                const f32x4 ce = *(const f32x4 *)(cr + 8 * q), co = *(const f32x4 *)(cr + 8 * q + 4);
                const f32x4 xa = *(const f32x4 *)(rowbuf + ch * CD + 8 * q), xb = *(const f32x4 *)(rowbuf + ch * CD + 8 * q + 4);
                xn = fmaf(xa.x, xa.x, xn);
                xn = fmaf(xa.y, xa.y, xn);
                xn = fmaf(xa.z, xa.z, xn);
                xn = fmaf(xa.w, xa.w, xn);
                xn = fmaf(xb.x, xb.x, xn);
                xn = fmaf(xb.y, xb.y, xn);
                xn = fmaf(xb.z, xb.z, xn);
                xn = fmaf(xb.w, xb.w, xn);
                acc = exact_chain8(acc, xa, xb, ce, co);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the chunk has been read: the next one may overwrite it
        }
        const float s = exact_dist(acc, xn, cn);
        if (ok && !bn) {
            if (s != s) {
                bn = true;
                bv = s;
                bi = k;
            } else if (s < bv) {
                bv = s;
                bi = k;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const bool on = __shfl_xor((int)bn, o) != 0;
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (better_euclid(on, ov, oi, bn, bv, bi)) {
            bn = on;
            bv = ov;
            bi = oi;
        }
    }
}

// Rescore list of the screened sweep, one wave and kRsEntries entries `first` .. of it (entry i is scr_list[cap - 1 - i]): a
// lane per (entry, candidate) pair.  The entry's <= 4 candidate codes are the 16-bit fields of its idx element (0xFFFF: none;
// written by vq_search_persist<.., SCREEN>).  Each lane runs the oracle's chain for its pair -- what exact_row_euclid does for
// a code -- and, in the same pass over the row, the d-ordered |x|^2 chain of the prologue; the four lanes of an entry then
// take the lowest distance, then the lowest code, and idx and the quantized row are stored over the provisional ones.
// As in exact_row_euclid nothing walks a row of its own: 8 lanes load the 128 B of one code (of one row) per chunk of 32 dims,
// one chunk ahead, into `cstage` (64 pairs) and `xstage` (16 rows), kExStageRow floats each, both private to the wave.
constexpr int kRsEntries = 16;
template <int DP>
__device__ __forceinline__ void rescore_batch(const SearchParams &p, unsigned cap, unsigned first, unsigned n1, float *cstage, float *xstage,
                                              int lane) {
    constexpr int RS = DP + 4, CD = kExChunk, SR = kExStageRow, NCH = DP / CD, NLC = 64 / 8, NLX = kRsEntries / 8;
    const int e = lane >> 2, j = lane & 3;
    const bool in_list = first + (unsigned)e < n1;
    unsigned ent = p.scr_list[cap - 1u - (in_list ? first + (unsigned)e : first)];
    const bool ok = in_list && ent < cap;  // (ent < cap: always, for a list the sweep wrote)
    if (!ok) ent = 0u;
    const int head = (int)(ent / (unsigned long long)p.M);
    const int row = (int)((long long)ent - (long long)head * p.M);  // (H M < 2^31)
    const long long io = (long long)head * p.idx_hs + (long long)row * p.idx_rs;
    const unsigned code = (unsigned)((unsigned long long)p.idx[io] >> (16 * j)) & 0xFFFFu;
    const bool valid = ok && code < (unsigned)p.K;
    const int kc = valid ? (int)code : 0;
    const int piece = lane & 7, sub = lane >> 3;  // this lane loads float4 `piece` of the chunk of pairs (rows) sub + 8 i
    const float *csrc[NLC], *xsrc[NLX];
#pragma unroll
    for (int i = 0; i < NLC; ++i) {
        const int q = sub + 8 * i;
        csrc[i] = p.packed + (long long)__shfl(head, q) * p.pk_hs + (long long)__shfl(kc, q) * RS + 4 * piece;
    }
#pragma unroll
    for (int i = 0; i < NLX; ++i) {
        const int q = 4 * (sub + 8 * i);
        xsrc[i] = p.x + (long long)__shfl(head, q) * p.x_hs + (long long)__shfl(row, q) * p.x_rs + 4 * piece;
    }
    f32x4 g[NLC], gx[NLX];
    auto load = [&](int ch) {
#pragma unroll
        for (int i = 0; i < NLC; ++i) g[i] = *(const f32x4 *)(csrc[i] + ch * CD);
#pragma unroll
        for (int i = 0; i < NLX; ++i)  // (natural rows: zeros behind D; D % 4 == 0)
            gx[i] = (ch * CD + 4 * piece < p.D) ? *(const f32x4 *)(xsrc[i] + ch * CD) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    };
    load(0);
    const float cn = p.packed[(long long)head * p.pk_hs + (long long)kc * RS + DP];
    const float *cr = cstage + lane * SR, *xr = xstage + e * SR;
    float acc = 0.0f, xn = 0.0f;
#pragma clang loop unroll(disable)
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int i = 0; i < NLC; ++i) *(f32x4 *)(cstage + (sub + 8 * i) * SR + 4 * piece) = g[i];
#pragma unroll
        for (int i = 0; i < NLX; ++i) *(f32x4 *)(xstage + (sub + 8 * i) * SR + 4 * piece) = gx[i];
        if (ch + 1 < NCH) load(ch + 1);
#pragma unroll
        for (int q = 0; q < CD / 8; ++q) {
            const f32x4 ce = *(const f32x4 *)(cr + 8 * q), co = *(const f32x4 *)(cr + 8 * q + 4);
            const f32x4 xa = *(const f32x4 *)(xr + 8 * q), xb = *(const f32x4 *)(xr + 8 * q + 4);
            xn = fmaf(xa.x, xa.x, xn);
            xn = fmaf(xa.y, xa.y, xn);
            xn = fmaf(xa.z, xa.z, xn);
            xn = fmaf(xa.w, xa.w, xn);
            xn = fmaf(xb.x, xb.x, xn);
            xn = fmaf(xb.y, xb.y, xn);
            xn = fmaf(xb.z, xb.z, xn);
            xn = fmaf(xb.w, xb.w, xn);
            acc = exact_chain8(acc, xa, xb, ce, co);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the chunk has been read: the next one may overwrite it
    }
    const float s = exact_dist(acc, xn, cn);
    float bv = valid ? s : __builtin_inff();
    int bk = valid ? kc : 0x7FFFFFFF;
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bk, o);
        if (ov < bv || (ov == bv && oi < bk)) {
            bv = ov;
            bk = oi;
        }
    }
    const bool store = ok && bk < p.K;  // (an entry always holds the screened argmin, a valid code)
    if (j == 0 && store) p.idx[io] = bk;
    if (p.out) {
        const int dl = 4 * lane;
#pragma unroll 4
        for (int r = 0; r < kRsEntries; ++r) {  // one row per step: 64 lanes x float4
            const int q = 4 * r;
            const int wk = __shfl(bk, q), hq = __shfl(head, q), rq = __shfl(row, q);
            if (__shfl((int)store, q) != 0 && dl < p.D)
                *(f32x4 *)(p.out + (long long)hq * p.out_hs + (long long)rq * p.out_rs + dl) =
                    *(const f32x4 *)(p.cb + (long long)hq * p.cb_hs + (long long)wk * p.D + dl);
        }
    }
}

// Second pass of the screened sweep: the rows it could not decide, on two lists that share one array of H M entries
// head * M + row (written by vq_search_persist<.., SCREEN> earlier on the stream; counts p.scr_count[0] and [1]).
//  * From the front, rows to search again in full by the exact rule.  Grid-stride over the entries, one 8-wave workgroup
//    per entry at a time: the row staged in LDS once, its |x|^2 chain recomputed in the prologue's order (d-ordered fmaf from
//    0), the waves split the K codes in runs of 64 (exact_row_euclid), the winner reduced over the waves through LDS in the
//    order of the rule; then idx and the quantized row are stored over the provisional ones.
//  * From the back, rows whose <= 4 candidates are known (their idx element holds the codes): rescore_batch, kRsEntries
//    entries per wave.  A full search keeps a workgroup busy for ~20 us, a batch a wave for a few, so the batches are dealt
//    to the workgroups that have no full-search entry: from the last workgroup downwards, one batch for every such workgroup
//    before a second wave of any of them gets one.  When every workgroup has a full search to do, all of them share.
// Few full searches (at most half the grid): the K codes of each row are split over S workgroups, workgroup e * S + s takes
// slice s of row e (resolve_plan in vq_resolve_plan.h: the one rule for S, the slices' codes and the dealing of the batches).
// A slice's workgroup publishes its (NaN met, value, index) as ONE 8-byte word in its slot of the control block (agent-scope
// atomic store), waits for that store (s_waitcnt vmcnt(0)) and adds to the row's ticket (agent-scope); the workgroup whose
// add returned S - 1 reads the S slots (agent-scope atomic loads), reduces them in slice order by the rule, stores idx and
// the quantized row and sets the ticket back to 0.  8-byte agent atomics on both sides need no fence.  More rows than that:
// S = 1, the rows are dealt grid-stride, a workgroup finishes its rows alone, no tickets.
// The kernel is the last reader of the two counts and leaves them zero for the next call on the image (which may be a cached
// one that no pack kernel touches again): every workgroup, also one with nothing to do, reads the counts, joins one barrier
// and then adds to the exit ticket (agent scope).  The workgroup whose add returned gridDim.x - 1 knows that all others have
// read the counts: when it has finished its own work it copies them to words kScrLastCountsWord, + 1 and zeroes the counts
// and the ticket.
// No workgroup ever waits for another (no spin loop, no polling: "the last arriver does the work" is the only step across
// workgroups), so a defect in these protocols could give a wrong result but never a hang.
// `flags` (A/B measurements and tests, from the environment per call): kResolveNoSplit = S is 1 whatever the counts
// (VQ_RESOLVE_NO_SPLIT).
// Dynamic LDS only (the launcher raises the kernel's dynamic limit to the CU's 160 KiB, which leaves no room for static
// arrays): [row, Dp floats][8 waves x 64 x kExStageRow floats of code staging][8 waves x kRsEntries x kExStageRow floats of
// row staging][the waves' winners: 3 x 8 words].
constexpr int kResolveWaves = 8;
constexpr int kResolveNoSplit = 1;
static_assert(kResolveWaves == (int)kResolvePlanWaves && kExCodes == (int)kResolvePassCodes && kRsEntries == (int)kResolveBatchRows,
              "vq_resolve_plan.h describes this kernel");
template <int DP>
constexpr size_t resolve_lds_bytes() {
    return ((size_t)DP + kResolveWaves * (kExCodes + kRsEntries) * kExStageRow + 3 * kResolveWaves) * 4;
}
// a slice's result as one word: value bits high, NaN flag and index (< 2^31) low
__device__ __forceinline__ unsigned long long resolve_slot_pack(bool bn, float bv, int bi) {
    return ((unsigned long long)__float_as_uint(bv) << 32) | (bn ? 0x80000000u : 0u) | ((unsigned)bi & 0x7FFFFFFFu);
}
template <int DP>
__global__ void __launch_bounds__(kResolveWaves * 64) vq_resolve_rows_kernel(const SearchParams p, int H, int flags) {
    constexpr int WAVES = kResolveWaves;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const unsigned cap = (unsigned)((long long)H * p.M);  // (choose_search: H M < 2^31, the array holds them all)
    unsigned *ctrl = p.scr_count;
    // (atomic loads: the values stay in registers, nothing reads the words again after the exit ticket below)
    const unsigned listed0 = __hip_atomic_load(ctrl + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned listed1 = __hip_atomic_load(ctrl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // The exit ticket is drawn HERE, once every wave of the workgroup holds the counts (the wait, then the barrier), and its
    // answer is looked at when the workgroup has finished: all that the cleaning workgroup has to know is that nobody will
    // read the counts any more, and this way the atomic's round trip runs beside the work instead of behind the last wave.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned exit_ticket = 0u;
    if (threadIdx.x == 0) exit_ticket = __hip_atomic_fetch_add(ctrl + kScrTicketWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned count = listed0, n1 = listed1;
    if (count > cap) count = cap;
    if (n1 > cap - count) n1 = cap - count;
    const unsigned grid = gridDim.x, wg = blockIdx.x;
    const ResolvePlan pl = resolve_plan(count, n1, grid, (unsigned)p.K, !(flags & kResolveNoSplit));  // (workgroup-uniform, the same in all)
    float *rowbuf = smem;
    float *red_v = smem + DP + WAVES * (kExCodes + kRsEntries) * kExStageRow;
    int *red_i = (int *)(red_v + WAVES), *red_n = red_i + WAVES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *stage = smem + DP + wave * (kExCodes * kExStageRow);
    float *xstage = smem + DP + WAVES * (kExCodes * kExStageRow) + wave * (kRsEntries * kExStageRow);
    // rows of this workgroup: slice `s` of row wg / S, or (S == 1) rows wg, wg + grid, ...
    unsigned e_first, e_step, s;
    resolve_wg_rows(pl, count, grid, wg, e_first, e_step, s);
    unsigned kb, ke;
    resolve_wave_codes((unsigned)p.K, pl.S, s, (unsigned)wave, kb, ke);
    const int kbeg = (int)kb, kend = (int)ke;
    for (unsigned e = e_first; e < count; e += e_step) {
        const unsigned ent = p.scr_list[e];
        if (ent >= cap) continue;  // (workgroup-uniform, and the same in every slice of the row; never true for a list the sweep wrote)
        const int head = (int)(ent / (unsigned long long)p.M);
        const long long row = (long long)ent - (long long)head * p.M;
        const float *xr = p.x + (long long)head * p.x_hs + row * p.x_rs;
        if (tid < DP) rowbuf[tid] = (tid < p.D) ? xr[tid] : 0.0f;
        __syncthreads();
        bool bn;
        float bv;
        int bi;
        exact_row_euclid<DP>(rowbuf, stage, p.packed + (long long)head * p.pk_hs, kbeg, kend, lane, bn, bv, bi);
        if (lane == 0) {
            red_n[wave] = (int)bn;
            red_v[wave] = bv;
            red_i[wave] = bi;
        }
        __syncthreads();
        if (wave == 0) {
            bn = red_n[0] != 0;
            bv = red_v[0];
            bi = red_i[0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {
                const bool on = red_n[w] != 0;
                const float ov = red_v[w];
                const int oi = red_i[w];
                if (better_euclid(on, ov, oi, bn, bv, bi)) {
                    bn = on;
                    bv = ov;
                    bi = oi;
                }
            }
            bool finish = true;
            if (pl.S > 1) {  // (e < kResolveMaxSplitRows, s < S <= kResolveMaxSplit: resolve_plan)
                unsigned long long *slots = (unsigned long long *)(ctrl + kScrSlotWord) + (size_t)e * kResolveMaxSplit;
                unsigned *ticket = ctrl + kScrRowTicketWord + e;
                int last = 0;
                if (lane == 0) {
                    __hip_atomic_store(slots + s, resolve_slot_pack(bn, bv, bi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slot has left before the ticket is drawn
                    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pl.S - 1u ? 1 : 0;
                }
                finish = __shfl(last, 0) != 0;
                if (finish) {  // every slice of the row has published: lane i reads slot i, the reduction runs in slice order
                    const unsigned long long mine =
                        (unsigned)lane < pl.S ? __hip_atomic_load(slots + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                    const unsigned lo = (unsigned)mine, hi = (unsigned)(mine >> 32);
                    bn = (__shfl(lo, 0) & 0x80000000u) != 0u;
                    bv = __uint_as_float(__shfl(hi, 0));
                    bi = (int)(__shfl(lo, 0) & 0x7FFFFFFFu);
                    for (unsigned i = 1; i < pl.S; ++i) {
                        const unsigned olo = __shfl(lo, (int)i), ohi = __shfl(hi, (int)i);
                        const bool on = (olo & 0x80000000u) != 0u;
                        const float ov = __uint_as_float(ohi);
                        const int oi = (int)(olo & 0x7FFFFFFFu);
                        if (better_euclid(on, ov, oi, bn, bv, bi)) {
                            bn = on;
                            bv = ov;
                            bi = oi;
                        }
                    }
                    if (lane == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (all S adds are in)
                }
            }
            if (finish) {
                if (lane == 0) p.idx[(long long)head * p.idx_hs + row * p.idx_rs] = bi;
                const int dl = 4 * lane;
                if (p.out && dl < p.D)  // (the persistent kernel's deferred copy: float4 of natural rows)
                    *(f32x4 *)(p.out + (long long)head * p.out_hs + row * p.out_rs + dl) =
                        *(const f32x4 *)(p.cb + (long long)head * p.cb_hs + (long long)bi * p.D + dl);
            }
        }
    }
    // the rescore batches of this wave (no barrier from here to the end of the work: the staging regions are the wave's own)
    unsigned bfirst, bstride;
    resolve_wave_batches(pl, grid, wg, (unsigned)wave, bfirst, bstride);
    for (unsigned b = bfirst; b < pl.nbatch; b += bstride) rescore_batch<DP>(p, cap, b * kRsEntries, n1, stage, xstage, lane);
    // leave the control block clean: the workgroup that drew the last exit ticket does it (see above)
    if (tid == 0) {
        if (exit_ticket == grid - 1u) {
            __hip_atomic_store(ctrl + kScrLastCountsWord, listed0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctrl + kScrLastCountsWord + 1, listed1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctrl + 0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctrl + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctrl + kScrTicketWord, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#ifdef VQ_EXP_SCREEN_COUNT
__device__ unsigned long long g_scr_rows[3];  // [0] rows listed for the second pass, [1] rows screened, [2] rows rescored
#endif

// SCREEN: the screened sweep described above (Dp = 256, Euclid, no TRAIN); p.scr holds the fp16 images.
template <int DP, int WAVES, int METRIC, bool TRAIN = false, bool SCREEN = false>
__global__ void __launch_bounds__(WAVES * 64, 2) vq_search_persist(const SearchParams p) {
    static_assert(!SCREEN || (DP == 256 && METRIC == VQ_METRIC_EUCLID && !TRAIN), "screened sweep: Dp = 256, Euclid, inference");
    using G = Geo<DP, WAVES>;
    constexpr int RS = G::RS, RS4 = G::RS4, CH = G::CH, XS = G::XS, NS = G::NS, SUB = G::SUB;
    constexpr bool EUCLID = (METRIC == VQ_METRIC_EUCLID);
    static_assert(G::NCH4 == 1 || DP == 512, "one float4 per lane covers a row");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4 *tile4 = (f32x4 *)smem;
    lds_f32x4 *tile4_lds = (lds_f32x4 *)smem;
    static_assert(G::SEP_STAGE, "rows are staged behind the tile buffers (one 8-wave workgroup per CU)");
    int *sidx = (int *)(smem + G::MAIN_FLOATS_S);  // [2][WAVES][32]: winners of the current and of the previous block

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float *pk = p.packed + (long long)head * p.pk_hs;
    const float *cbh = p.cb + (long long)head * p.cb_hs;
    const float *scrh = SCREEN ? (const float *)((const char *)p.scr + head * p.scr_hs) : nullptr;
    // SCREEN, per head from the words behind the tiles (all wave-uniform: scalar registers): max |c|^2 of the codebook (the
    // bound's nc^2), E_c / s_c, the bound's absolute term, the pack kernel's flag and the scales
    float scr_mcn = 0.0f, scr_ecs = 0.0f, scr_abs = 0.0f, scr_sx = 1.0f, scr_isg = 1.0f;
    unsigned scr_flag = 0u;
    if constexpr (SCREEN) {
        const float *tail = (const float *)((const char *)scrh + (long long)p.ntiles * kScrTileBytes);
        float ec = 0.0f, l1 = 0.0f;
        auto nanmax = [](float a, float v) { return (v > a || v != v) ? v : a; };
        for (int i = lane; i < p.ntiles; i += 64) {
            scr_mcn = nanmax(scr_mcn, tail[kScrTailMcn * p.ntiles + i]);
            ec = nanmax(ec, tail[kScrTailEc * p.ntiles + i]);
            l1 = nanmax(l1, tail[kScrTailL1 * p.ntiles + i]);
            scr_flag |= ((const unsigned *)tail)[kScrTailFlag * p.ntiles + i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            scr_mcn = nanmax(scr_mcn, __shfl_xor(scr_mcn, o));
            ec = nanmax(ec, __shfl_xor(ec, o));
            l1 = nanmax(l1, __shfl_xor(l1, o));
            scr_flag |= (unsigned)__shfl_xor((int)scr_flag, o);
        }
        int e_c = ((const int *)tail)[kScrTailExp * p.ntiles], e_x = ((const int *)tail)[kScrTailExp * p.ntiles + 1];
        if (e_c > kScrMaxExp || e_c < -kScrMaxExp || e_x > kScrMaxExp || e_x < -kScrMaxExp) {  // (never, for an image the pack kernel wrote)
            e_c = e_x = 0;
            scr_flag = 1u;
        }
        scr_sx = scr_pow2(e_x);
        scr_isg = scr_pow2(-(e_c + e_x));
        scr_ecs = ec * scr_pow2(-e_c);
        scr_abs = (0x1p-13f * l1 + 0x1p-116f) * scr_isg + 0x1p-140f;
        scr_mcn = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(scr_mcn)));
        scr_ecs = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(scr_ecs)));
        scr_abs = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(scr_abs)));
        scr_sx = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(scr_sx)));
        scr_isg = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(scr_isg)));
        scr_flag = __builtin_amdgcn_readfirstlane(scr_flag);
    }
    float *outh = p.out ? p.out + (long long)head * p.out_hs : nullptr;
    const float INF = __builtin_inff();
    const int nblk = (int)((p.M + 32 * WAVES - 1) / (32 * WAVES));
    const int dl = 4 * lane;            // this lane's float4 of a natural row
    const bool dok = dl < p.D;
    // SCREEN: waves w and w + 4 share a SIMD and run the same program between the same barriers.  With the epilogue at one
    // place both would leave the matrix pipe idle at once and then compete for it; waves 4..7 (a scalar branch) run theirs
    // after group kScrLateGroup instead, beside their partners' MFMAs.  When a wave folds a sub-tile into its three lowest
    // values changes none of them (order statistics), so p.scr_stagger = 0 gives the same bits.
    const bool scr_late = SCREEN && p.scr_stagger != 0 && wave >= 4;

    // deferred copy of the previous block's rows (all wave-uniform except the data registers)
    int cp_rows = 0, cp_next = 0;       // rows of the previous block / next row to load
    long long cp_row0 = 0;
    const int *cp_idx = sidx;           // the previous block's winners (this wave's 32)
    int cp_pend = -1;                   // row whose data sits in cp_v, waiting to be stored
    f32x4 cp_v = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 cp_x = {0.0f, 0.0f, 0.0f, 0.0f};  // TRAIN: the row itself
    float cp_e = 0.0f;                  // TRAIN: this lane's part of the squared error sum (all blocks of the workgroup)
    int cp_iv = 0;                      // winner index of row cp_next, read from LDS one step ahead
    // the finalize's arithmetic on one float4 of a row (vector_quantize_pytorch.py:273,362)
    auto train_quant = [&](const f32x4 &cv, const f32x4 &xv) -> f32x4 {
        const f32x4 diff = cv - xv;
        cp_e = fmaf(diff.x, diff.x, cp_e);
        cp_e = fmaf(diff.y, diff.y, cp_e);
        cp_e = fmaf(diff.z, diff.z, cp_e);
        cp_e = fmaf(diff.w, diff.w, cp_e);
        return p.ste ? xv + diff : cv;
    };
    auto copy_step = [&]() {
        if (cp_pend >= 0) {
            if (dok) {
                f32x4 o = cp_v;
                if constexpr (TRAIN) o = train_quant(cp_v, cp_x);
                if (p.out) __builtin_nontemporal_store(o, (f32x4 *)(outh + (cp_row0 + cp_pend) * p.out_rs + dl));
            }
            cp_pend = -1;
        }
        if (cp_next < cp_rows) {
            const int i = __builtin_amdgcn_readfirstlane(cp_iv);
            if (dok) {
                cp_v = *(const f32x4 *)(cbh + (long long)i * p.D + dl);
                if constexpr (TRAIN) cp_x = *(const f32x4 *)(xh + (cp_row0 + cp_next) * p.x_rs + dl);
            }
            cp_pend = cp_next;
            ++cp_next;
            if (cp_next < cp_rows) cp_iv = cp_idx[cp_next];
        }
    };

    auto stage = [&](int tile, int buf) {
        if constexpr (SCREEN) {  // an fp16 tile: its own length, whole KiB
            static_assert(kScrChunks * 1024 <= G::BUF_F4 * 16, "an fp16 tile fits the fp32 tile's buffer");
#pragma unroll
            for (int i2 = 0; i2 < (kScrChunks + WAVES - 1) / WAVES; ++i2) {
                const int ck = i2 * WAVES + wave;
                if (ck < kScrChunks)
                    lds_dma16(scrh, p.scr_bytes, lane * 16, tile * kScrTileBytes + ck * 1024, tile4_lds + buf * G::BUF_F4 + ck * 64);
            }
        } else {
            stage_tile<G, WAVES>(pk, p.pk_bytes, tile, tile4_lds + buf * G::BUF_F4, wave, lane);
        }
    };
    // Diagnostic build (-DVQ_EXP_STAMPS; tools/stamps_persist.py): per wave and row block `it` < 8 the shader-clock time of
    // block start, prologue end, sweep end and resolve end in slots 4 it .. 4 it + 3, the end of the open finalize in slot 56,
    // the wave's block count in slot 57, the real-time pair in slots 60 / 61.  SCREEN, sub-tiles 12 .. 17 of block it == 2:
    // barrier release, start and end of the epilogue (of the sub-tile before), barrier arrival in slots 32 + 4 (u - 12) .. + 3.
#define PSTAMP(j) do { if (it < 8) STAMP(4 * it + (j)); } while (0)
#define SSTAMP(j) do { if (it == 2 && u >= 12 && u < 18) STAMP(32 + 4 * (u - 12) + (j)); } while (0)
    int it = 0;
    long long row0 = 0;
    STAMP_RT(60);
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x, ++it) {
        row0 = ((long long)blk * WAVES + wave) * 32;
        PSTAMP(0);
        // the sweep's first tile goes out before the rows are loaded: the tile buffers are free (the previous sweep ended with a
        // barrier) and the rows are staged behind them
        stage(0, 0);
        // ---------------- prologue: this wave's 32 rows -> MFMA fragments in registers ----------------
        // (load_x_fragments of vq_search.inc written out in place: vector loads only, and SCREEN pairs the groups of 8 dims
        //  into fp16 fragments instead of swapping them -- see there)
        __builtin_amdgcn_s_setprio(2);
        float xf[NS];  // (unused by SCREEN)
        f16x8 xhf[SCREEN ? DP / 16 : 1], xlf[SCREEN ? DP / 16 : 1];  // SCREEN: B fragments of group s = 16 dims (hi, lo) of s_x x
        float xn0 = 0.0f;
        {
            float *xs = smem + G::NBUF * G::BUF_F4 * 4 + wave * (32 * XS);
            constexpr int NCHUNK = DP / CH;
            constexpr int LPL = CH / 8;
            f32x4 v[2][LPL];
            auto load_chunk = [&](int ch, f32x4 (&dst)[LPL]) {
#pragma unroll
                for (int i2 = 0; i2 < LPL; ++i2) {
                    const int f = i2 * 64 + lane;
                    const int r = f / (CH / 4), c4 = f % (CH / 4);
                    long long grow = row0 + r;
                    if (grow >= p.M) grow = p.M - 1;
                    const int d0 = ch * CH + c4 * 4;
                    f32x4 t = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (d0 < p.D) t = __builtin_nontemporal_load((const f32x4 *)(xh + grow * p.x_rs + d0));
                    dst[i2] = t;
                }
            };
            load_chunk(0, v[0]);
#pragma unroll
            for (int ch = 0; ch < NCHUNK; ++ch) {
                if (ch + 1 < NCHUNK) load_chunk(ch + 1, v[(ch + 1) & 1]);
#pragma unroll
                for (int i2 = 0; i2 < LPL; ++i2) {
                    const int f = i2 * 64 + lane;
                    const int r = f / (CH / 4), c4 = f % (CH / 4);
                    *(f32x4 *)(xs + r * XS + c4 * 4) = v[ch & 1][i2];
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                const float *rp = xs + c * XS;
                f32x4 plo, phi;  // SCREEN: the previous (even) group of 8 dims
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
                        asm volatile("" : "+v"(xn0));
                    }
                    if constexpr (SCREEN) {
                        // B operand of v_mfma_f32_32x32x16_f16: lane (c, h) holds dims 16 s + 8 h .. + 7 of row c
                        if (j & 1) {
                            const f32x8 v8 = h ? (f32x8){lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}
                                               : (f32x8){plo.x, plo.y, plo.z, plo.w, phi.x, phi.y, phi.z, phi.w};
                            const int sg = ch * (CH / 16) + (j >> 1);
                            split_f16x2(v8 * scr_sx, xhf[sg], xlf[sg]);
                        } else {
                            plo = lo;
                            phi = hi;
                        }
                        continue;
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
        }
        __builtin_amdgcn_s_setprio(0);
        const long long row = row0 + c;
        const bool row_ok = row < p.M;
        const float b_aug = EUCLID ? (h ? 1.0f : xn0) : 1.0f;

        const unsigned cb_flag = codebook_flag(pk, p.pk_bytes);
        // (SCREEN starts from +inf: a flagged codebook makes every row uncertain instead, below)
        LaneBest lb = lane_best_start<METRIC>(SCREEN ? INF : sweep_start_value<METRIC>(cb_flag));
        // SCREEN, per lane over its codes: the three lowest KEYS (the screened value with the accumulator register's number in
        // its 4 low mantissa bits) and the sub-tiles in which the two lowest arrived (vq_scr_keys.h: tag, three-lowest block and
        // sub-tile update, no branch and no search of the registers; the codes are decoded once, after the sweep).  The keys
        // overwrite the accumulators, which are dead after their epilogue.
        ScrTrack scr_t = scr_track_start();
        auto epilogue = [&](f32x16 &v, int u) {
            if constexpr (SCREEN) {
                scr_track_update(scr_t, v, u);
            } else {
                tile_epilogue<METRIC, DP, false>(v, u, h, p.K, lb);
            }
        };

        const int t1 = p.ntiles;
        // SCREEN sub-tile: 16 groups of 16 dims, 2 fp16 MFMAs each (ct.xh, ct.xl), |c|^2 s_c s_x as the accumulator's start;
        // fragments read PF groups ahead, one ds_read_b128 per 2 MFMAs
        auto run_sub_scr = [&](f32x16 &acc, f32x16 &prev, int u, bool have_prev) {
            constexpr int NGS = DP / 16, PF = VQ_SCR_PF;
            static_assert(kScrLateGroup > 3 && kScrLateGroup < NGS, "the late epilogue sits inside the last range of groups");
            SSTAMP(0);
            const int cur = u & 1;
            const char *tb = (const char *)(tile4 + cur * G::BUF_F4);
            const char *ta = tb + c * kScrRowBytes + 16 * h;
            f16x8 ah[NGS];
            {
                const f32x4 *cn4 = (const f32x4 *)(tb + kScrCnOffset);  // acc[r] <-> code 4 h + (r & 3) + 8 (r >> 2)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 cv = cn4[2 * q + h];
                    acc[4 * q + 0] = cv.x; acc[4 * q + 1] = cv.y; acc[4 * q + 2] = cv.z; acc[4 * q + 3] = cv.w;
                }
                // the last sub-tile may hold padding codes, whose +inf would become a NaN key: they start from a large finite
                // value instead, which no real code's |c|^2 s_c s_x (< 2^29) reaches (vq_scr_keys.h; a wave-uniform branch)
                if (u + 1 == t1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = scr_start_clamp(acc[r]);
                }
            }
#pragma unroll
            for (int g = 0; g < PF; ++g) ah[g] = *(const f16x8 *)(ta + 32 * g);
            copy_step();
            auto groups = [&](auto g0c, auto g1c) {
                constexpr int G0 = decltype(g0c)::value, G1 = decltype(g1c)::value;
#pragma unroll
                for (int g = G0; g < G1; ++g) {
                    if (g + PF < NGS) ah[g + PF] = *(const f16x8 *)(ta + 32 * (g + PF));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[g], xhf[g], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[g], xlf[g], acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            groups(IntC<0>{}, IntC<1>{});
            if (have_prev && !scr_late) {
                SSTAMP(1);
                epilogue(prev, u - 1);
                SSTAMP(2);
            }
            __builtin_amdgcn_sched_barrier(0);
            groups(IntC<1>{}, IntC<3>{});
            if (u + 1 < t1) stage(u + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            groups(IntC<3>{}, IntC<kScrLateGroup>{});
            // waves 4..7: the same call, while their SIMD partners 0..3 are in their MFMA tails (`prev` is not written before
            // the next sub-tile; the fences keep the block where it is)
            if (have_prev && scr_late) {
                SSTAMP(1);
                epilogue(prev, u - 1);
                SSTAMP(2);
            }
            __builtin_amdgcn_sched_barrier(0);
            groups(IntC<kScrLateGroup>{}, IntC<NGS>{});
            SSTAMP(3);
            __syncthreads();
        };
        auto run_sub = [&](f32x16 &acc, f32x16 &prev, int u, bool have_prev) {
            if constexpr (SCREEN) {
                run_sub_scr(acc, prev, u, have_prev);
                return;
            }
            const int t = u / SUB, st = u % SUB;
            const int cur = t & 1;
            const f32x4 *tb = tile4 + cur * G::BUF_F4 + st * (kTileCodes * RS4);
            constexpr int NG = DP / 8;
            constexpr int G1 = NG >= 2 ? 1 : NG, G2 = NG >= 4 ? 3 : NG;
            const f32x4 *ta = tb + c * RS4 + h;
            f32x4 a[NG];
            acc = (f32x16){0};
            const float a_aug = EUCLID ? ((const float *)tb)[c * RS + DP + 1 - h] : 0.0f;
            mfma_prefetch<DP>(a, ta);
            copy_step();  // one row of the PREVIOUS block: store the row loaded a sub-tile ago, load the next one (right after
                          // the barrier: the whole sub-tile lies between these accesses and the next barrier's vmcnt(0))
            mfma_range<DP, 0, G1>(acc, a, ta, xf);
            if (have_prev) epilogue(prev, u - 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_range<DP, G1, G2>(acc, a, ta, xf);
            if (st == 0 && t + 1 < t1) stage(t + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_range<DP, G2, NG>(acc, a, ta, xf);
            if (EUCLID) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
            }
            if (st == SUB - 1) __syncthreads();
        };

        PSTAMP(1);
        __syncthreads();  // the first tile (issued before the prologue) has landed for every wave
        {
            f32x16 acc0, acc1;
            int u = 0;
            const int u1 = t1 * SUB;
            bool have_prev = false;
            for (; u + 1 < u1; u += 2) {
                run_sub(acc0, acc1, u, have_prev);
                run_sub(acc1, acc0, u + 1, true);
                have_prev = true;
            }
            if (u < u1) {
                run_sub(acc0, acc1, u, have_prev);
                epilogue(acc0, u);
            } else if (have_prev) {
                epilogue(acc1, u - 1);
            }
        }
        // rows of the previous block the sweep did not get to (short sweeps), and the last store
        while (cp_next < cp_rows || cp_pend >= 0) copy_step();
        PSTAMP(2);

        float best_s;
        int best_i;
        long long cand = 0;     // SCREEN: the candidate codes of a row on the rescore list (lane h == 0), stored as its idx
        bool has_cand = false;
        if constexpr (SCREEN) {
            // the screened argmin of this lane (lowest code holding the lowest value), then both lane halves of the row
            // (the accumulators are in units of s_c s_x: one exact division by that power of two for the values kept)
            // this lane's two lowest keys and their codes, decoded from the keys' low bits BEFORE the scaling (which keeps the
            // order and, for normal results, the bits; the codes are right where it matters: (I1), (I2) of vq_scr_keys.h)
            const int li1 = scr_key_code(scr_t.b1, scr_t.u1, h), li2 = scr_key_code(scr_t.b2, scr_t.u2, h);
            const float l1 = scr_t.b1 * scr_isg, l2 = scr_t.b2 * scr_isg;
            const float scr_b3 = scr_t.b3 * scr_isg;
            best_i = li1 < p.K ? li1 : p.K - 1;  // (a NaN / inf row's keys decode to anything in [0, 32 ntiles))
            float b1 = l1;
            const float ob1 = __shfl_xor(l1, 32), ob2 = __shfl_xor(l2, 32), ob3 = __shfl_xor(scr_b3, 32);
            const int oi = __shfl_xor(best_i, 32);
            const float b2 = fminf(fmaxf(l1, ob1), fminf(l2, ob2));  // second lowest of the row over distinct codes
            if (ob1 < b1 || (ob1 == b1 && oi < best_i)) {
                b1 = ob1;
                best_i = oi;
            }
            // certainty test (the bound: top of this file)
            const float nx = sqrtf(xn0), nc = sqrtf(scr_mcn);
            const float delta = 1.1f * (1.0001f * scr_ecs * nx + 4.81e-5f * (2.0f * nx * nc) + 3.25e-5f * scr_mcn + 1.21e-7f * xn0 + scr_abs);
            const float w = 0x1p-20f * (__builtin_fabsf(b1) + xn0 + delta);
            const bool eligible = cb_flag == 0u && scr_flag == 0u && xn0 * scr_sx * scr_sx <= 0x1p30f && scr_mcn <= 0x1p100f &&
                                  (b1 + xn0 > 2.0f * delta);
            const bool certain = eligible && (b2 - b1 > 2.0f * delta + w);
            best_s = 0.0f;  // (the screened calls do not return distances)
            // Uncertain rows.  Only a code with S <= thr = b1 + 2 delta + w can beat or tie the exact winner (its D would
            // otherwise exceed the winner's by more than the sqrt rounding window, and `eligible` excludes clamping).  When
            // the third lowest value of BOTH lane halves is above thr, the row's candidates are among the <= 4 codes the
            // halves hold: the second pass rescores those by the exact chain (rescore); every other row goes onto the list of
            // rows that it searches again in full (candidate overflow, NaN / inf rows, ineligible magnitudes, flagged codebooks).
            const float thr = b1 + 2.0f * delta + w;
            const bool complete = eligible && scr_b3 > thr && ob3 > thr;
            const unsigned rescore = (unsigned)__ballot(row_ok && !certain && complete);
            const unsigned todo = (unsigned)__ballot(row_ok && !certain && !complete);
#ifdef VQ_EXP_SCREEN_COUNT
            const unsigned rows_here = (unsigned)__ballot(row_ok);  // (outside the branch: a ballot sees the active lanes only)
            if (lane == 0) {
                atomicAdd(&g_scr_rows[0], (unsigned long long)__builtin_popcount(todo));
                atomicAdd(&g_scr_rows[1], (unsigned long long)__builtin_popcount(rows_here));
                atomicAdd(&g_scr_rows[2], (unsigned long long)__builtin_popcount(rescore));
            }
#endif
            // Both kinds of uncertain row are decided by vq_resolve_rows_kernel after this kernel, which stores their idx and
            // quantized rows; until then they keep the screened argmin in sidx (best_i < K: the deferred copy gathers a valid
            // code row).  One array of H M entries head * M + row holds both lists: rows to search in full from the front,
            // rows to rescore from the back (a row is on one list at most, so the ends never meet).
            if (rescore != 0u) {
                // the row's candidates = the codes of both lane halves with S <= thr, as four 16-bit codes (0xFFFF: none;
                // K <= 3072 here) in the row's own idx element, which the second pass reads and overwrites
                const unsigned my = ((l1 <= thr) ? (unsigned)li1 : 0xFFFFu) | (((l2 <= thr) ? (unsigned)li2 : 0xFFFFu) << 16);
                const unsigned other = (unsigned)__shfl_xor((int)my, 32);
                unsigned at = 0u;
                if (lane == 0) at = atomicAdd(p.scr_count + 1, (unsigned)__builtin_popcount(rescore));
                at = __builtin_amdgcn_readfirstlane(at);
                if (h == 0 && ((rescore >> c) & 1u)) {
                    const unsigned cap = (unsigned)((long long)gridDim.y * p.M);
                    p.scr_list[cap - 1u - (at + __builtin_popcount(rescore & ((1u << c) - 1u)))] = (unsigned)((long long)head * p.M + row);
                    cand = (long long)(((unsigned long long)other << 32) | my);
                    has_cand = true;
                }
            }
            if (todo != 0u) {
                unsigned at = 0u;
                if (lane == 0) at = atomicAdd(p.scr_count, (unsigned)__builtin_popcount(todo));
                at = __builtin_amdgcn_readfirstlane(at);
                if (h == 0 && ((todo >> c) & 1u))
                    p.scr_list[at + __builtin_popcount(todo & ((1u << c) - 1u))] = (unsigned)((long long)head * p.M + row);
            }
        } else {
        row_winner<METRIC>(lb, h, p.K, best_s, best_i);
        // non-finite inputs (rare, out of line; see repair_nonfinite_rows)
        if (const unsigned todo = nonfinite_rows(best_s, row_ok); __builtin_expect(todo != 0u, 0)) {
            float *rowbuf = smem + G::NBUF * G::BUF_F4 * 4 + wave * (32 * XS);  // this wave's row staging region
            auto fill_row = [&](int rr) -> float { return fill_row_from_memory<METRIC, DP, 0, 0>(p, head, row0 + rr, rowbuf, lane); };
            auto acc_init = [&](int, int) -> float { return 0.0f; };
            repair_nonfinite_rows<METRIC, DP>(todo, rowbuf, pk, 0, p.K, lane, fill_row, acc_init, best_s, best_i);
        }
        }
        PSTAMP(3);
        if (h == 0 && row_ok) store_winner(p, head, row, 0, best_s, has_cand ? cand : (long long)best_i);
        int *mine = sidx + ((it & 1) * WAVES + wave) * 32;
        mine[c] = best_i;
        // this block becomes the one to copy during the next sweep (wave-private LDS: in order, no barrier needed)
        cp_rows = (p.M - row0 >= 32) ? 32 : (p.M - row0 > 0 ? (int)(p.M - row0) : 0);
        cp_row0 = row0;
        cp_idx = mine;
        cp_next = 0;
        cp_pend = -1;
        if (cp_rows > 0) cp_iv = mine[0];
    }

    // ---------------- the last block of this workgroup: gather + store in the open, four rows in flight ----------------
    __builtin_amdgcn_s_setprio(2);
    constexpr int RB = 4;
    for (int rr0 = 0; rr0 < cp_rows; rr0 += RB) {
        f32x4 o[RB], xv[RB];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int rr = (rr0 + k < cp_rows) ? rr0 + k : cp_rows - 1;
            const int i = cp_idx[rr];
            o[k] = dok ? *(const f32x4 *)(cbh + (long long)i * p.D + dl) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (TRAIN) xv[k] = dok ? *(const f32x4 *)(xh + (cp_row0 + rr) * p.x_rs + dl) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            if (rr0 + k < cp_rows && dok) {
                if constexpr (TRAIN) o[k] = train_quant(o[k], xv[k]);
                if (p.out) __builtin_nontemporal_store(o[k], (f32x4 *)(outh + (cp_row0 + rr0 + k) * p.out_rs + dl));
            }
        }
    }
    if constexpr (TRAIN) {
        if (p.loss_part) {  // one partial per wave: [head][workgroup][wave]
#pragma unroll
            for (int o2 = 32; o2 > 0; o2 >>= 1) cp_e += __shfl_xor(cp_e, o2);
            if (lane == 0) p.loss_part[((long long)head * gridDim.x + blockIdx.x) * WAVES + wave] = cp_e;
        }
    }
    STAMP(56);
    STAMP_RT(61);
#ifdef VQ_EXP_STAMPS
    if (lane == 0) g_stamps[(((long long)blockIdx.x * WAVES + wave) & 8191) * VQ_NSTAMP + 57] = (unsigned long long)it;
#endif
#undef PSTAMP
#undef SSTAMP
}
