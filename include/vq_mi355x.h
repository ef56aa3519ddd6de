/*
 * vq_mi355x.h -- C ABI of the MI355X (gfx950) nearest-codebook library  (libvq_mi355x.so).
 *
 * The reference (MisterBourbaki/vector-quantization-by-ml) has NO native layer: its hot path is a
 * sequence of ATen calls issued from Python.  Each entry point below therefore replaces a run of
 * reference Python lines (cited per function, paths relative to the reference root) rather than an
 * existing FFI symbol, and is what a maintainer would bind (ctypes stub in INTEGRATION.md).
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM) unless stated; the library never allocates or frees
 *     persistent memory and never synchronises the host: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = default stream);
 *   - all floating point is fp32, indices are int64 (reference: codebooks.py:354, general.py:128);
 *   - strides are in ELEMENTS; rows of x / out may be strided (head-split views need no copy);
 *   - return value: 0 on success, a negative VQ_E* code for argument errors, or a positive
 *     hipError_t.  vq_last_error() returns a human-readable string for the calling thread.
 *   - re-entrant across streams; no global mutable state besides the per-thread error string.
 *   - buffers: the contents of a workspace are unspecified on entry and on exit -- every call writes what it later reads,
 *     so a caller may hand over uninitialised memory and reuse one buffer across calls (the one exception is stated where
 *     it applies: vq_gumbel_reinmax_backward_codes_f32 reuses what vq_gumbel_reinmax_columns_f32 left).  No call writes
 *     outside the workspace_bytes it was given or outside the documented extent of an output; an output is written in
 *     full unless its description names the elements that are left as they were.
 */
#ifndef VQ_MI355X_H
#define VQ_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQ_METRIC_EUCLID 0 /* similarity = -cdist(x, c)      codebooks.py:128-129 */
#define VQ_METRIC_DOT 1    /* similarity = einsum(x, c)      codebooks.py:122-123 */

#define VQ_E_BADARG (-1)
#define VQ_E_UNSUPPORTED (-2)
#define VQ_E_NODEVICE (-3)

/* flags */
#define VQ_F_STE 1u          /* out = x + (q - x)  (train-mode straight-through, vector_quantize_pytorch.py:273) */
#define VQ_F_FORCE_SIMPLE 2u /* use the scalar-FMA fallback kernel instead of the MFMA kernel (cross-check)        */
#define VQ_F_FORCE_SPLIT 4u  /* force the split-K + packed-key path even when the fused path would be chosen        */
#define VQ_F_X_F16 16u        /* a->x points to fp16 rows (strides in elements); inference only: no STE / sq_err          */
#define VQ_F_X_BF16 32u       /* a->x points to bf16 rows; both are widened in the prologue = the reference's x.float() */
#define VQ_F_SQERR_PER_HEAD 8u /* sq_err (and grad_sq_err of the backward) are [H][Q]: one sum per head and stage     */

/*
 * Packed codebook image (the layout the search kernel streams through LDS).  For one codebook of
 * K codes x D dims:  Kp rows of (Dp + 4) floats, Dp = padded dim chosen by the library (32/64/128/256/512) and Kp = K
 * rounded up to the staged LDS tile (32 codes at Dp >= 256, else 256 / Dp * 32: 64 / 128 / 256 codes at Dp = 128 / 64 / 32);
 * inside each group of 8 dims the even dims come first, then the odd ones, values pre-scaled by -2 (Euclid) or 1 (dot);
 * float Dp of each row holds |c|^2 (d-ordered fmaf chain; +inf for the padding rows), float Dp + 1 holds 1.0, float
 * Dp + 2 the same chain under either metric; the last 16 bytes of the image hold a "some code is non-finite" word.
 * D > 512: ceil(D / 512) such images back to back, one per 512-dim slice of the rows (the last one as wide as it needs).
 * Returns the number of floats ONE packed codebook occupies (including over-copy slack), 0 on bad args.
 */
int64_t vq_packed_floats(int K, int D);

/*
 * Pack `n_codebooks` natural row-major [K, D] codebooks (consecutive ones `cb_stride` floats apart)
 * into `packed` (consecutive images vq_packed_floats(K, D) floats apart).
 * Replaces: the per-call operand preparation inside ATen cdist (cat([-2x,|x|^2,1]) / cat([c,1,|c|^2])),
 * reached from codebooks.py:386.
 */
int vq_pack_codebooks_f32(const float *cb, int n_codebooks, int64_t cb_stride, int K, int D, int metric,
                          float *packed, void *stream);

typedef struct vq_args {
    /* problem */
    int32_t H;      /* independent codebooks searched side by side (heads)  -- grid.y              */
    int32_t Q;      /* residual stages (1 = plain VectorQuantize)                                  */
    int64_t M;      /* rows per head                                                               */
    int32_t K;      /* codes per codebook                                                          */
    int32_t D;      /* dims                                                                        */
    int32_t metric; /* VQ_METRIC_*                                                                 */
    uint32_t flags; /* VQ_F_*                                                                      */
    /* inputs */
    const float *x;        /* [H][M][D], element (h, m, d) at x[h*x_hs + m*x_rs + d]               */
    int64_t x_rs, x_hs;
    const float *cb;       /* natural codebooks: (h, q, k, d) at cb[h*cb_hs + q*cb_qs + k*D + d]    */
    int64_t cb_hs, cb_qs;  /* (cb_qs = 0: all stages share one codebook)                           */
    const float *packed;   /* packed images: codebook (h, q) at packed[h*pk_hs + q*pk_qs]           */
    int64_t pk_hs, pk_qs;
    /* outputs (any of out / best / sq_err may be NULL) */
    float *out;            /* quantized (or straight-through) rows, (h, m, d) at out[h*out_hs + m*out_rs + d];
                              for Q > 1: ((0 + q_1) + q_2) + ...   residual_vq.py:233                */
    int64_t out_rs, out_hs;
    int64_t *idx;          /* (h, m, q) at idx[h*idx_hs + m*idx_rs + q*idx_qs]                      */
    int64_t idx_rs, idx_hs, idx_qs;
    float *best;           /* winning sqrt-distance (Euclid) / similarity (dot); same indexing as idx */
    double *sq_err;        /* [Q] : sum over all heads/rows/dims of (q - x)^2 per stage (overwritten;
                              fixed summation order -> run-to-run reproducible);
                              commitment loss = weight * sq_err / (H*M*D)   vector_quantize_pytorch.py:362 */
    /* scratch */
    void *workspace;       /* >= vq_workspace_bytes() bytes, 16-byte aligned                        */
    int64_t workspace_bytes;
    /* optional, vq_quantize_f32 only: the caller-cached screen image of `packed` (vq_pack_screen_image_f32) and its
       vq_screen_image_bytes(); NULL and 0: the call builds its own in the workspace.  Ignored by calls that take
       another kernel; a byte count that does not match is VQ_E_BADARG.                               */
    void *screen;
    int64_t screen_bytes;
} vq_args;

/*
 * The screen image: what the fp16 screened sweep reads instead of the fp32 packed image (plain Euclid inference calls of
 * 128 < D <= 256 with 1 024 <= Kp <= 3 072 codes and enough rows to fill the chip), followed by a small control block that
 * the call's kernels share.  It is a pure function of the packed image, so a caller whose codebook stays put between calls
 * builds it once and hands it over in vq_args.screen: the call then launches no pack kernel.
 *   vq_screen_image_bytes: bytes of the H images plus the control block; 0 where no screened sweep exists for the shape
 *     (host arithmetic only).  The room per image is that of the earlier bf16-pair image, so buffers sized by it stay
 *     valid and the control block stays where it was; the fp16 image fills about half of it and the rest is unused
 *     (never written, never read).
 *   vq_pack_screen_image_f32: builds the images of `packed` (head stride pk_hs floats) into `screen` (16-byte aligned,
 *     screen_bytes == vq_screen_image_bytes(...)) and zeroes the control block.  Per head: every code as one fp16 value
 *     fp16(s_c * -2c), 32-code tiles of 528-byte rows with the tile's |c|^2 s_c s_x behind them; behind the tiles, per
 *     tile, max |c|^2, the codes' largest rounding error |s_c c' - fp16|_2 and largest sum |fp16|, a flag and max |-2c_i|,
 *     then the exponents of the two power-of-two scales s_c, s_x (csrc/vq_search_persist.inc has the layout and the
 *     error bound that reads it).  Two kernels on `stream`.
 * One image serves one call at a time: calls that share it must be ordered on one stream (the control block holds the
 * call's counts and tickets; every call leaves those zeroed for the next).
 */
int64_t vq_screen_image_bytes(int H, int K, int D, int metric);
int vq_pack_screen_image_f32(const float *packed, int H, int64_t pk_hs, int K, int D, int metric, void *screen,
                             int64_t screen_bytes, void *stream);

/* Bytes of scratch vq_quantize_f32 / vq_search_keys_f32 may need for (H, M, Q): packed keys (+ 8 MiB of key planes for K
 * splits), squared-error partials and -- residual stacks (Q > 1) of more than 32 768 rows -- 64 MiB for the residual rows of a
 * partly filled last round of workgroups, which is searched stage by stage (residual_vq.py:212-243 on the remainder). */
int64_t vq_workspace_bytes(int H, int64_t M, int Q);

/*
 * The same for rows WIDER than 512 dims (Q == 1).  The reference has no limit on the row width (cdist / einsum over any
 * D, codebooks.py:122-129,386); here a distance is one k-ordered fmaf chain over all dims, so such rows are swept in
 * 512-dim slices and the chains of one (row chunk) x (code chunk) wait in the workspace between two slices
 * (at most 512 MiB beyond vq_workspace_bytes(H, M, 1)).  For D <= 512 this is vq_workspace_bytes(H, M, 1).
 */
int64_t vq_workspace_bytes_wide(int H, int64_t M, int K, int D);

/*
 * The hot path: search (+ residual loop) + gather + straight-through + squared-error sums.
 * Replaces Codebook.forward's search core  codebooks.py:386-397  (similarity -> first argmax -> gather),
 * VectorQuantize.forward's quantize step   vector_quantize_pytorch.py:261-279,337,361-364  and, for Q > 1,
 * the ResidualVQ loop                      residual_vq.py:154-155,212-243.
 * Bit-exact twin: oracle/vq_oracle.c (k-ordered fmaf chains).
 */
int vq_quantize_f32(const vq_args *a, void *stream);

/*
 * vq_quantize_f32 for Q == 1 that ALSO emits lse[h*M + m] = log sum_k exp(similarity[h, m, k]) from the same sweep
 * (online softmax in the search epilogue).  With a->best (the winner's distance / similarity) this is everything the
 * cross-entropy commitment loss needs -- vector_quantize_pytorch.py:338-346 -- so that loss costs no second sweep:
 * logit[argmax] = -best (Euclid) / best (dot).  D <= 512, fused path only (no VQ_F_FORCE_* flags).
 */
int vq_quantize_lse_f32(const vq_args *a, float *lse, void *stream);

/* Thin named wrappers: Q must be 1 for vq_nearest_f32. */
int vq_nearest_f32(const vq_args *a, void *stream);
int vq_residual_f32(const vq_args *a, void *stream);

/* Largest number of residual stages ONE fused launch can hold for rows of dimension D (the winners' indices and, with
 * want_sq_err, the loss partials of every stage live in the CU's 160 KiB of LDS).  0 for D > 512 (such rows are searched one stage per call, in 512-dim slices).
 * A caller with more stages (the reference's ResidualVQ has no limit, residual_vq.py:212-243) runs its layers one
 * launch each instead.  Host-side arithmetic only: no device call. */
int vq_max_fused_stages(int D, int want_sq_err);

/*
 * Codebook-sharded search, step 1: search only the local shard and emit one packed SIGNED 64-bit key
 * per row:  hi = order image of the value ("smaller wins", top bit flipped), lo = code index + idx_offset.
 * `keys[h*M + m]` is combined with atomic MIN, so the caller initialises it (vq_keys_init) and may then
 * reduce keys across GPUs with ncclMin on int64 (RCCL).  Uses a->x, a->packed, H, M, K, D, metric; Q == 1.
 */
int vq_keys_init(int64_t *keys, int64_t n, void *stream);
int vq_search_keys_f32(const vq_args *a, int64_t idx_offset, int64_t *keys, void *stream);

/*
 * The same search without the init launch and without atomics: when the library splits K over workgroups (few rows: the
 * chip would not be full otherwise), split z STORES its winners into plane z of `keys` [vq_key_planes(a)][H][M]; the
 * winner of a row is the MIN over the planes -- and over the planes of the other shards, which is what the exchange of
 * the sharded path transports and vq_finalize_key_planes_f32 reduces.  vq_key_planes is host arithmetic (same arguments
 * as the search call, current device's CU count).  Rows wider than 512 dims / VQ_F_FORCE_SIMPLE: one plane, initialised
 * and combined inside the call.
 */
int vq_key_planes(const vq_args *a);
int vq_search_key_planes_f32(const vq_args *a, int64_t idx_offset, int64_t *keys, void *stream);

/*
 * Step 2: decode the (reduced) keys and finish: idx/best, gather from the natural codebook `a->cb`
 * (indexed by the GLOBAL code index), straight-through, sq_err.  Q == 1.
 * vq_finalize_key_planes_f32: `keys` holds n_planes candidate planes [n_planes][H][M] (K splits x shards, e.g. the
 * all-gathered planes of every rank); the MIN over the planes is taken on the fly.
 */
int vq_finalize_keys_f32(const vq_args *a, const int64_t *keys, void *stream);
int vq_finalize_key_planes_f32(const vq_args *a, const int64_t *keys, int n_planes, void *stream);

/*
 * Backward of vq_quantize_f32 with respect to x (the autograd of the quantize step, vector_quantize_pytorch.py:261-279,
 * 361-364, and of the residual loop, residual_vq.py:212-243), one pass:
 *   grad_x = (VQ_F_STE ? Q * grad_out : 0) + sum_q 2 * grad_sq_err[q] * (r_q - c_q[idx_q])
 * Uses a->x, a->cb (cb_qs = 0: shared codebook), a->idx as written by the forward, H, M, D, Q, flags.  grad_out (same
 * layout conventions as out) and grad_sq_err ([Q] doubles on the device) may each be NULL.  The codebook receives no
 * gradient here (learnable codebooks take the PyTorch path).
 */
int vq_quantize_backward_f32(const vq_args *a, const float *grad_out, int64_t go_rs, int64_t go_hs, const double *grad_sq_err,
                             float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream);

/*
 * The rotation trick (Fifty et al., "Restructuring Vector Quantization with the Rotation Trick", arXiv 2410.06424, section
 * 4.2): backward of the quantize step with respect to x when the straight-through estimator is replaced by the rotation
 * and rescaling that carries each row onto its code.  The forward is vq_quantize_f32 with VQ_F_STE, unchanged.  For one
 * stage with input row r (the residual that stage quantized), selected code c = cb[idx] and eps = 1e-6:
 *   a = max(|r|, eps)   b = max(|c|, eps)   u = r / a   qh = c / b   s = u + qh   w = s / max(|s|, eps)
 *   lam = |c| / a                                        (numerator unclamped)
 *   rot(r) = lam * (r - 2 (r.w) w + 2 (r.u) qh)          (u, qh, w, lam constants of autograd; the value is c)
 *   d/dr :  g  ->  lam * (g - 2 (g.w) w + 2 (g.qh) u)
 * and every residual of a stack is x minus detached terms, so one pass computes
 *   grad_x = sum_q lam_q (g - 2 (g.w_q) w_q + 2 (g.qh_q) u_q) + sum_q 2 * grad_sq_err[q] * (r_q - c_q[idx_q]),  g = grad_out.
 * Degenerate rows follow the formula and stay finite: c = 0 gives a zero rotation term, c = -r gives s = 0 and w = 0,
 * r = 0 gives u = 0 and lam = |c| * 1e6.  The codes receive no gradient through the output.
 * Arguments as vq_quantize_backward_f32: a->x (strided rows and heads), a->cb (cb_qs = 0: shared codebook), a->idx as
 * written by the forward (any strides), H, M, D, Q, flags (VQ_F_STE: the residual chain is recomputed with the forward's
 * rule quant = r + (c - r); VQ_F_SQERR_PER_HEAD: grad_sq_err is [H][Q]); grad_out and grad_sq_err may each be NULL.
 * D <= 1024 (the row is held in registers; wider rows: VQ_E_UNSUPPORTED).  M == 0 returns 0 without a launch.
 */
int vq_rotate_backward_f32(const vq_args *a, const float *grad_out, int64_t go_rs, int64_t go_hs, const double *grad_sq_err,
                           float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream);

/*
 * Training-state step that FOLLOWS the hot path -- exponential-moving-average codebook update.
 * vq_ema_accumulate_f32: counts[h*K + k] += 1 and sums[(h*K + k)*D + d] += x[h, m, d] for every row m assigned to
 *   code k = idx[h*idx_hs + m*idx_rs] (rows with mask[h*M + m] == 0 are skipped; mask may be NULL).  Rows whose index is
 *   outside [0, K) -- negative, K or larger, compared as 64-bit values -- are skipped as well: not counted, their x rows not read.
 *   Both this entry and vq_ema_accumulate_det_f32 ADD INTO the existing contents of counts / sums (a second call on the
 *   same buffers doubles the contribution); the caller zeroes them for a fresh result (and all-reduces them across
 *   replicas when codebooks are synchronised).  x, idx and mask are only read.  M == 0 returns 0 without a launch.
 *   Replaces embed_onehot.sum(1) and einsum("h n d, h n c -> h c d") -- codebooks.py:405-415 -- without the one-hot.
 * vq_ema_update_f32: cluster_size.lerp_(counts, 1-decay); embed_avg.lerp_(sums, 1-decay); embeddings =
 *   [l2norm](embed_avg / laplace_smoothing(cluster_size) * total) -- codebooks.py:411,417-425.  total_scratch: H floats.
 *   decay is a double because the reference forms 1 - decay in double and rounds the WEIGHT to fp32 once: rounding decay
 *   first moves the weight by up to u * decay / (1 - decay) (16 ulp of the weight at decay = 0.99).
 * The sums are exact up to fp32 summation order (float atomics / per-wave partial sums: run-to-run differences at the
 * 1e-7 relative level).
 */
int vq_ema_accumulate_f32(const float *x, int64_t x_rs, int64_t x_hs, const int64_t *idx, int64_t idx_rs, int64_t idx_hs,
                          const uint8_t *mask, int H, int64_t M, int K, int D, float *counts, float *sums, void *stream);
/* Run-to-run REPRODUCIBLE variant of vq_ema_accumulate_f32 (same arguments, same meaning): no float atomics -- every
 * (row range, code owner) pair stores its partial sums to `workspace` and a second kernel adds the row ranges in a fixed
 * order, so two runs on the same device give bit-identical counts / sums.  workspace: >= vq_ema_det_workspace_bytes()
 * bytes, 16-byte aligned (0 = unsupported: D > 2048).  Meant for the common "many rows per code" regime; with very many
 * codes and few rows it is slower than the atomic path (every owner scans all indices). */
int64_t vq_ema_det_workspace_bytes(int H, int64_t M, int K, int D);
int vq_ema_accumulate_det_f32(const float *x, int64_t x_rs, int64_t x_hs, const int64_t *idx, int64_t idx_rs, int64_t idx_hs,
                              const uint8_t *mask, int H, int64_t M, int K, int D, float *counts, float *sums, void *workspace,
                              int64_t workspace_bytes, void *stream);
/* The same statistics for every stage of a residual stack in one pass (residual_vq.py:212-233: stage q's Codebook sees the
 * residual r_q): uses a->x, a->cb (stages cb_qs apart; 0 = shared), a->idx (as written by vq_quantize_f32), H, M, K, D, Q
 * and VQ_F_STE (train-mode residual rule).  counts [H][Q][K], sums [H][Q][K][D], zeroed by the caller. */
int vq_ema_accumulate_residual_f32(const vq_args *a, float *counts, float *sums, void *stream);
int vq_ema_update_f32(float *cluster_size, float *embed_avg, float *embeddings, const float *counts, const float *sums,
                      float *total_scratch, int H, int K, int D, double decay, float eps, int l2norm, void *stream);

/*
 * Dead-code expiry decided and carried out on the device (codebooks.py:216-262, expire_codes_ / replace): no host
 * synchronisation, capturable in a hipGraph.  Two launches on `stream`, issued whatever the cluster sizes hold.
 * Per head h of cluster_size [H][K], embed_avg [H][K][D], embeddings [H][K][D] (contiguous):
 *   code k is dead iff cluster_size[h][k] < threshold, an fp32 comparison (a NaN is not dead); its rank r is the number of
 *   dead codes below k, n_dead the number of dead codes of the head.  The three entries of a live code are not written.
 *   A dead code gets embeddings[h][k][:] = row, cluster_size[h][k] = reset_cluster_size, embed_avg[h][k][:] =
 *   fl(row * reset_cluster_size), where row is pool row sel(h, r) -- element (h, n, d) of the pool at
 *   pool[h*pool_hs + n*pool_rs + d], N rows per head, pool_hs may be 0 (one pool for all heads) -- copied bit for bit when
 *   l2norm == 0, and divided by max(||row||, 1e-12) when l2norm == 1 (F.normalize of the picked row: fp32 sum of squares, one
 *   square root, one division per element; an all-zero row stays zero).
 * Row selection: sel(h, r) is a function of (seed, h, r, n_dead <= N, N) only, never of the launch geometry.  P(c0, c1) names
 * the four words of Philox4x32-10 (the generator of vq_gumbel_sample_f32) with
 *   key      k0 = seed[0] bits 31..0, k1 = seed[0] bits 63..32
 *   counter  (c0, c1) as given, (c3 : c2) = (h << 32) + seed[1]  (mod 2^64, c2 the low word).
 *   n_dead > N (with replacement, the reference's randint): w = P(r, 0xFFFFFFFF); sel = ((w[1] << 32) | w[0]) mod N.
 *   n_dead <= N (without replacement, the reference's randperm(N)[:n_dead]): b = the bit length of N - 1 (0 for N == 1), so
 *     that 2^b < 2N.  One application of the bijection F of [0, 2^b) is six Feistel rounds on uneven halves: with widths
 *     wl = b / 2 (rounded down) and wr = b - wl, round i = 0 .. 5 splits y into hi = y >> wr and lo = y mod 2^wr and sets
 *     y = (lo << wl) | ((hi xor P(lo, i)[0]) mod 2^wl), then swaps wl and wr.  Cycle walk: y = r; repeat y = F(y) until
 *     y < N, at most 64 applications; sel = y.  F is a bijection, so sel(h, .) is injective on [0, N).  A walk from a point
 *     below N leaves [0, N) for at most 2^b - N applications in a row, so the bound cannot be reached at all while
 *     2^b - N < 64; beyond that every application lands below N with probability above 1/2 (N / 2^b), and a walk reaches the bound
 *     with probability below 2^-64 per dead code (F taken as a random permutation).  At the bound sel = y - N: inside [0, N),
 *     as y < 2^b < 2N, but the head's selection may then hold that row twice.
 * picked (may be NULL): picked[h][k] = sel for a dead code, -1 for a live one (written in full).  n_expired (may be NULL):
 *   n_expired[h] = n_dead.  seed: TWO 64-bit words on the DEVICE.
 * Residual chain: with chain != NULL the pool is not read (pool may be NULL; N = chain->M).  Row n of the pool is the
 *   stage-`stage` residual of row n of chain->x, rebuilt for the picked rows only with the fp32 operations of the
 *   straight-through chain in its order: r = x; for j < stage: c = cb_j[idx[n][j]]; quant = r + (c - r); r = r - quant (an
 *   index outside [0, K) ends the row's chain, as in vq_ema_accumulate_residual_f32).  Reads chain->x (x_rs), chain->cb
 *   (stages cb_qs apart; 0 = shared), chain->idx (idx_rs, idx_qs), M, K, D, Q; H and chain->H must be 1, K and D the
 *   codebook's, 0 <= stage < Q.  chain->cb must not overlap `embeddings` (the stage codes of the forward are a copy).
 * workspace: >= vq_expire_workspace_bytes(H, K) bytes, 16-byte aligned ([n_dead: H int32][dead codes in ascending order:
 *   H * K int32]).  N == 0, H == 0 or K == 0: returns 0 without a launch (nothing is written).  VQ_E_BADARG: D < 1, a
 *   negative size, H > 65535, a null required pointer, a chain that does not fit.
 * Rows of any D and alignment: 16-byte accesses when D % 4 == 0 and the picked row, the code's two rows and the chain's
 *   codebooks lie on the 16-byte grid (decided per picked row), else one float at a time.
 */
int64_t vq_expire_workspace_bytes(int H, int K);
int vq_expire_codes_f32(float *cluster_size, float *embed_avg, float *embeddings, const float *pool, int64_t pool_rs, int64_t pool_hs,
                        int64_t N, const vq_args *chain, int stage, int H, int K, int D, float threshold, float reset_cluster_size,
                        int l2norm, const int64_t *seed /* 2 words, device */, int64_t *picked /* [H][K] or NULL */,
                        int32_t *n_expired /* [H] or NULL */, void *workspace, void *stream);

/*
 * Affine re-parameterisation of a codebook (codebooks.py:275-348, 379-384, 400-403).
 *
 * vq_affine_stats_f32: per-column statistics of the rows (h, m, :) at x[h*x_hs + m*x_rs + d] in ONE read of x:
 *   count[h] = rows kept by the mask (all M without one), mean[h][d] their mean, m2[h][d] = sum (x - mean)^2 (the biased
 *   variance is m2 / count; both 0 when count is 0).  mask: NULL or uint8 (h, m) at mask[h*mask_hs + m*mask_rs], non-zero =
 *   keep.  The same entry point serves the codebook's own statistics (x = the codes, M = K).
 *   No atomics and a fixed summation order (bit-identical from run to run); the raw sum of squares is never formed.
 *   Geometry: VEC = 4 columns per thread (float4 loads) when x, x_rs, x_hs are 16-byte aligned and D % 4 == 0, else VEC = 1;
 *   TC = min(64, next power of two >= ceil(D / VEC)) threads across the columns, TR = 256 / TC row lanes, CG = ceil(D / (TC VEC))
 *   column groups, nblk = clamp(ceil(M / (16 TR)), 1, max(1, 1024 / (H CG))) row blocks.  Row lane r of block b folds the rows
 *   b TR + r + i nblk TR, i = 0, 1, ..., in that order (Welford in fp32 on x minus the lane's first kept row); the TR lanes are
 *   merged pairwise (lane r takes lane r + s, s = TR / 2 .. 1); then 64 lanes per column fold the nblk partials (lane j:
 *   b = j, j + 64, ... in that order) and are merged pairwise (lane j takes lane j + s, s = 32 .. 1).  Every merge is Chan's
 *   formula in fp64.
 *   workspace: >= vq_affine_stats_workspace_bytes(H, M, D) bytes, 16-byte aligned.  VQ_E_UNSUPPORTED: M / nblk >= 2^24.
 *
 * vq_affine_apply_f32: elementwise over in / out [H][K][D] contiguous (in == out allowed), the four statistics [H][D],
 *   std = sqrt(clamp(variance, min = 1e-5)) computed in the kernel:
 *   mode 0 (codes -> batch space)             out = (in - codebook_mean) * (batch_std / codebook_std) + batch_mean
 *   mode 1 (accumulated sums -> codebook space) out = in * r + hits[h][k] * (codebook_mean - batch_mean * r), r = codebook_std / batch_std
 *          = the per-code sums of (x - batch_mean) * r + codebook_mean from the sums of the raw rows (vq_ema_accumulate_f32).
 */
int64_t vq_affine_stats_workspace_bytes(int H, int64_t M, int D);
int vq_affine_stats_f32(const float *x, int64_t x_rs, int64_t x_hs, const uint8_t *mask, int64_t mask_rs, int64_t mask_hs, int H,
                        int64_t M, int D, int64_t *count, float *mean, float *m2, void *workspace, int64_t workspace_bytes,
                        void *stream);
int vq_affine_apply_f32(const float *in, float *out, const float *hits /* mode 1 */, const float *codebook_mean,
                        const float *codebook_variance, const float *batch_mean, const float *batch_variance, int H, int K, int D,
                        int mode, void *stream);

/*
 * Consumers of the similarity matrix.  Both use a->x, a->packed (a->cb for D > 512 / VQ_F_FORCE_SIMPLE),
 * H, M, K, D, metric; Q is ignored.
 * vq_similarities_f32: sims[h*sims_hs + m*sims_rs + k] = -cdist(x, c) (Euclid) or x.c (dot): the third return value of
 *   Codebook.forward -- codebooks.py:386,435 -- bit-identical to the values the search compares.  The caller chooses
 *   how many rows to materialise at once (row chunks via the x / sims pointers).  Rows wider than 512 dims run the sliced
 *   MFMA sweep when a->workspace holds vq_workspace_bytes_wide(H, M, K, D) bytes, else one thread per entry.
 * vq_softmax_stats_f32: logits = scale * similarity; lse[h*M + m] = log sum_k exp(logit), target_logit[h*M + m] = logit
 *   of code target[h*tgt_hs + m*tgt_rs] (0 for a negative = ignored target; -inf for one >= K).  This is
 *   F.cross_entropy(distances, codes, ignore_index=-1) -- vector_quantize_pytorch.py:287-297 -- as an online-softmax
 *   epilogue of the sweep: [M, K] never exists.  target may be NULL (lse only).  Accuracy: native sqrt/exp/log (1e-6 rel).
 *   A target is compared with 0 and K as the 64-bit value it is, before any narrowing (2^32 + 3 is out of range, not code 3);
 *   vq_ce_backward_f32 and vq_ce_backward_live_f32 ignore a row whose target is negative OR >= K (its grad_x is exactly 0).
 *   A row with a NaN or a +inf logit has lse = NaN (ATen's log_softmax), a NaN target logit stays NaN.
 */
int vq_similarities_f32(const vq_args *a, float *sims, int64_t sims_rs, int64_t sims_hs, void *stream);
int vq_softmax_stats_f32(const vq_args *a, float scale, const int64_t *target, int64_t tgt_rs, int64_t tgt_hs, float *lse,
                         float *target_logit, void *stream);

/*
 * Backward of that cross entropy with respect to x, fused (flash-attention style, nothing of [M, K] in memory):
 *   grad_x[h, m, :] = coef * d/dx (lse - logit[target])   for rows with target >= 0, 0 for ignored rows
 * = the autograd of F.cross_entropy o (-cdist | einsum) the reference runs -- vector_quantize_pytorch.py:292-294 with
 * ATen's _euclidean_dist_backward.  lse / target_logit: the vq_softmax_stats_f32 outputs (scale 1; the softmax part of
 * the gradient runs through the MFMA sweep, the one-hot part is a rank-one term per row added from a->cb, the natural
 * codebook, with 1 / dist_target taken from target_logit); coef: ONE float on the device
 * (upstream gradient / number of non-ignored rows).  D <= 512 (VQ_E_UNSUPPORTED beyond: use row chunks of
 * vq_similarities_f32).  The gradient with respect to a learnable codebook is vq_ce_backward_codes_f32 below.
 */
int vq_ce_backward_f32(const vq_args *a, const float *lse, const float *target_logit, const int64_t *target, int64_t tgt_rs,
                       int64_t tgt_hs, const float *coef, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream);

/*
 * The same backward when the codebook has been rewritten between forward and backward.  In the reference the EMA step
 * overwrites the codes through .data right after the similarities were computed (codebooks.py:418-425), which autograd does
 * not see: the backward of the cross entropy (vector_quantize_pytorch.py:284-299,338-346) then multiplies the ratio matrix,
 * computed from the OLD similarities, with the UPDATED codebook.  Per head, with x [M, D], c [K, D] the codes the forward
 * searched (a->packed), l [K, D] the live codes at backward time (live_cb natural, live_packed its packed image: same K, D
 * and metric as c), s = similarities(x, c) and
 *   gs_mk = coef * [t_m >= 0] * (softmax_k(s_m)_k - [k == t_m]):
 *   dot     grad_x_m = sum_k gs_mk l_k
 *   Euclid  r_mk = gs_mk / s_mk (0 where s_mk == 0, ATen's mask);  grad_x_m = x_m sum_k r_mk - sum_k r_mk l_k
 * Everything that decides the weights comes from c (the similarity sweep, lse, target_logit, the zero-distance mask, the
 * sum of the ratios, the factor of the one-hot term); everything they are multiplied with from l.  a->cb is not read.
 * live_cb == a->cb with live_packed == a->packed is legal; with l bit-equal to c the result is vq_ce_backward_f32's
 * (its one-wave kernel, VQ_CE_NO_ROLES=1) bit for bit.  D <= 256: VQ_E_UNSUPPORTED beyond (two tile rings of wider rows do
 * not fit in LDS; use row chunks of vq_similarities_f32).  The other arguments are vq_ce_backward_f32's.
 */
int vq_ce_backward_live_f32(const vq_args *a, const float *live_cb, int64_t live_cb_hs, const float *live_packed, int64_t live_pk_hs,
                            const float *lse, const float *target_logit, const int64_t *target, int64_t tgt_rs, int64_t tgt_hs,
                            const float *coef, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream);

/*
 * Backward of the same cross entropy with respect to a learnable codebook (the codes the forward searched, unchanged since),
 * nothing of [M, K] in memory.  Per head, with s = similarities(x, c), t the targets and lse / coef as for vq_ce_backward_f32:
 *   w_mk = coef * (exp(s_mk - lse_m) - [k == t_m])   for rows with 0 <= t_m < K, 0 for every other (= ignored) row
 *   dot     grad_codes_k = sum_m w_mk x_m
 *   Euclid  r_mk = w_mk / s_mk (0 where s_mk == 0, ATen's mask);   grad_codes_k = c_k sum_m r_mk - sum_m r_mk x_m
 * Reads a->x (strided rows), a->cb (the natural codebook), H, M, K, D, metric; lse [H][M] contiguous (scale 1, natural log);
 * target (h, m) at target[h*tgt_hs + m*tgt_rs], compared with 0 and K as the 64-bit value it is; coef: ONE float on the
 * device.  grad_codes [H][K][D] contiguous.  The x, the lse and the logits of an ignored row are never multiplied with
 * anything (they may be NaN / inf): its weight is selected to 0 and its row is packed as padding.  A wave owns 32 codes,
 * the packed rows are streamed; the one-hot term is a comparison inside the sweep.  The rows are split over workgroups by the
 * plan of vq_gumbel_backward_codes_f32 and the splits' partial sums are added in split order: no float atomics,
 * bit-identical results from run to run on one device.  M == 0: grad_codes is cleared, nothing else is touched.
 * VQ_E_UNSUPPORTED: D > 256, more than 2^31 - 1 rows, a packed row image of 2 GiB or more (use row chunks of
 * vq_similarities_f32).  VQ_E_BADARG: a->cb, grad_codes, lse, target or coef null; a workspace that is too small or misaligned.
 * Workspace (>= vq_ce_codes_workspace_bytes bytes, 16-byte aligned; 0 = unsupported shape), in 4-byte units, with
 * img = vq_packed_floats(M, D), rsM = vq_gumbel_row_stride(M) and splits as in the reinmax entry below:
 *   [x image: H*img][target int32: H*rsM (-1 = ignored or past M)][lse: H*rsM]
 *   [grad_codes partials: splits*H*K*D, only when splits > 1]
 */
int64_t vq_ce_codes_workspace_bytes(int H, int64_t M, int K, int D);
int vq_ce_backward_codes_f32(const vq_args *a, const float *lse, const int64_t *target, int64_t tgt_rs, int64_t tgt_hs,
                             const float *coef, float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Backward of the straight-through Gumbel softmax over the similarities (utils/general.py:147-149 with
 * codebooks.py:386-395), nothing of [M, K] in memory.  With s = similarities, g = dL/dquantize, a = g c^T, tau = 1 / temperature:
 *   p = softmax_k(tau s), delta_m = sum_k p_mk a_mk, w = tau p (a - delta) = dL/ds, and through the similarities
 *   dot: gx = w c, gc = w^T x;   Euclid: r = w / s (0 at s == 0), gx = x rowsum(r) - r c, gc = c colsum(r) - r^T x.
 * All three use a->x, H, M, K, D (<= 256: VQ_E_UNSUPPORTED beyond), metric and the rows g (h, m, d) at g[h*g_hs + m*g_rs + d].
 * lse2 / delta: [H][vq_gumbel_row_stride(M)] floats, 16-byte aligned; columns past M are not written and reach no result.
 * vq_gumbel_stats_f32 (a->packed): writes lse2[h][m] = log2 sum_k exp2(tau s log2 e) and delta[h][m].
 * vq_gumbel_backward_x_f32 (a->packed): grad_x (h, m, d) at grad_x[h*gx_hs + m*gx_rs + d].
 * vq_gumbel_backward_codes_f32 (a->cb, the natural codebook): grad_codes [H][K][D] contiguous -- the part through the
 *   similarities only; the gradient of the gather itself is vq_ema_accumulate_f32 of g.  The rows are packed into the
 *   workspace (>= vq_gumbel_workspace_bytes bytes, 16-byte aligned; 0 = unsupported shape), split over workgroups, and the
 *   splits' partial sums are added in a fixed order: no float atomics, bit-identical results from run to run on one device.
 */
int64_t vq_gumbel_row_stride(int64_t M);
int64_t vq_gumbel_workspace_bytes(int H, int64_t M, int K, int D);
int vq_gumbel_stats_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, float *lse2, float *delta,
                        void *stream);
int vq_gumbel_backward_x_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2,
                             const float *delta, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream);
int vq_gumbel_backward_codes_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2,
                                 const float *delta, float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Backward of the reinmax Gumbel softmax over the similarities (utils/general.py:131-146 with codebooks.py:386-395), nothing
 * of [M, K] in memory.  With s, g, a, tau as above and ind the selected code of every row:
 *   p0 = softmax_k(s)                      delta0_m = sum_k p0_mk a_mk
 *   ptau = softmax_k(tau s)                p1_mk = max((onehot(ind_m)_k + ptau_mk) / 2, 1e-5)
 *   col_k = sum_m p1_mk                    e_k = (sum_m p1_mk a_mk) / col_k        (sums over the rows of the head)
 *   w_mk = 2 (p1_mk / col_k)(a_mk - e_k) - 0.5 p0_mk (a_mk - delta0_m) = dL/ds, and through the similarities as above.
 * All four use a->x, H, M, K, D (<= 256: VQ_E_UNSUPPORTED beyond), metric and the rows g; tau must be positive and finite
 * (VQ_E_BADARG).  M == 0: nothing is launched (backward_codes zeroes grad_codes).
 * Per-row arrays lse2_tau / lse2_one / delta0: [H][vq_gumbel_row_stride(M)] floats (columns past M are not written and
 * reach no result); per-code arrays col / e: [H][vq_gumbel_row_stride(K)] floats (entries past K are written as col = 1, e = 0); all 16-byte aligned.
 * ind: int64, element (h, m) at ind[h*ind_hs + m*ind_rs].  It is only ever COMPARED with a code index: a value outside
 * [0, K) selects nothing.  It need not be the argmax of the similarities.
 * vq_gumbel_reinmax_stats_f32 (a->packed): lse2_tau[h][m] = log2 sum_k exp2(tau s log2 e), lse2_one the same at tau = 1, delta0.
 * vq_gumbel_reinmax_columns_f32 (a->cb): writes col and e.  It packs the x rows and the g rows into the workspace, converts
 *   ind to int32 there, sweeps the rows in splits and adds the splits' partial sums in split order.
 * vq_gumbel_reinmax_backward_x_f32 (a->packed): grad_x (h, m, d) at grad_x[h*gx_hs + m*gx_rs + d].
 * vq_gumbel_reinmax_backward_codes_f32 (a->cb): grad_codes [H][K][D] contiguous, the part through the similarities only.
 *   CONTRACT: it must be given the workspace that vq_gumbel_reinmax_columns_f32 filled for the same a->x, g, ind and shape
 *   on the same stream order -- it reuses the packed row images and the int32 ind found there and does not pack again.
 * No float atomics anywhere: results are bit-identical from run to run on one device.
 * Workspace (>= vq_gumbel_reinmax_workspace_bytes bytes, 16-byte aligned; 0 = unsupported shape), in 4-byte units, with
 * img = vq_packed_floats(M, D), rsM = vq_gumbel_row_stride(M), rsK = vq_gumbel_row_stride(K), splits = the row splits of
 * the plan vq_gumbel_backward_codes_f32 uses:
 *   [x image: H*img][g image: H*img][ind int32: H*rsM (-1 past M)][col partials: splits*H*rsK][e partials: splits*H*rsK]
 *   [grad_codes partials: splits*H*K*D, only when splits > 1]
 * More than 2^31 - 1 rows or a packed row image of 2 GiB or more: VQ_E_UNSUPPORTED (use row chunks).
 */
int64_t vq_gumbel_reinmax_workspace_bytes(int H, int64_t M, int K, int D);
int vq_gumbel_reinmax_stats_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, float *lse2_tau,
                                float *lse2_one, float *delta0, void *stream);
int vq_gumbel_reinmax_columns_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2_tau,
                                  const int64_t *ind, int64_t ind_rs, int64_t ind_hs, float *col, float *e, void *workspace,
                                  int64_t workspace_bytes, void *stream);
int vq_gumbel_reinmax_backward_x_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2_tau,
                                     const float *lse2_one, const float *delta0, const int64_t *ind, int64_t ind_rs, int64_t ind_hs,
                                     const float *col, const float *e, float *grad_x, int64_t gx_rs, int64_t gx_hs, void *stream);
int vq_gumbel_reinmax_backward_codes_f32(const vq_args *a, const float *g, int64_t g_rs, int64_t g_hs, float tau, const float *lse2_tau,
                                         const float *lse2_one, const float *delta0, const float *col, const float *e,
                                         float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Codebook diversity loss (vector_quantize_pytorch.py:324-334 with utils/general.py:25-30) and its gradients with respect to
 * the rows and to a learnable codebook, nothing of [M, K] in memory.  With s the similarities [H][M][K] as above, T the diversity temperature, N the
 * number of sequence positions and n(m) = (m / pos_div) % N the position of row m of every head (pos_div = 1, or the number
 * of heads when the heads of one shared codebook are interleaved in the rows); C = H * M / N rows per position:
 *   p_hmk = softmax_k(-T s_hmk)                     (the sign is the reference's: under Euclid the FAR codes get the mass)
 *   A_nk  = (1 / C) sum over h and the rows m with n(m) = n of p_hmk          (over the heads too, in head order)
 *   loss  = (1 / N) sum_nk A_nk log(max(A_nk, 1e-5))
 *   U_nk  = g / (N C) * (log(max(A_nk, 1e-5)) + [A_nk >= 1e-5])               (g = dL/dloss; ATen's clamp backward)
 *   delta_hm = sum_k p_hmk U[n(m)][k]               w_hmk = dL/ds_hmk = -T p_hmk (U[n(m)][k] - delta_hm)
 *   dot:    grad_x = w l             Euclid:  r = w / s (0 where s == 0),  grad_x = x rowsum(r) - r l
 *   dot:    grad_codes_k = sum_m w_mk x_m            Euclid:  grad_codes_k = c_k sum_m r_mk - sum_m r_mk x_m      (all rows of the head)
 * where l = the live codes when live_packed is given, else the codes of a->packed: everything that decides the weights (s,
 * lse2, the zero mask, rowsum(r)) comes from a->packed, what they are multiplied with from live_packed (the convention of
 * vq_ce_backward_live_f32).  loss and U are [N][K] element-wise work on A and are left to the caller.
 * All five use a->x (strided rows), H, M, K, D (<= 256: VQ_E_UNSUPPORTED beyond) and metric; Q is ignored.  Checked before
 * any launch (VQ_E_BADARG): T finite; N > 0, pos_div > 0 and M a multiple of N * pos_div; every array argument non-null
 * and 16-byte aligned.  M == 0: nothing is launched and nothing is written (backward_codes zeroes grad_codes).
 * lse2, delta: [H][vq_gumbel_row_stride(M)] floats (columns past M are not written and reach no result).
 * A, U: [N][vq_gumbel_row_stride(K)] floats; the entries of A past K are written as 0, those of U must be finite (they are
 * read and discarded).
 * vq_diversity_stats_f32 (a->packed): lse2[h][m] = log2 sum_k exp2(-T s log2 e).
 * vq_diversity_accumulate_f32 (a->cb, the natural codes): writes A.  The rows are packed into the workspace in position-major
 *   order -- image row n*Cp + j holds row ((j / pos_div) N + n) pos_div + j % pos_div for j < M / N, with
 *   Cp = ceil(M / N / 32) * 32: every position is padded to whole 32-row sub-tiles, the padding contributes exactly 0 -- and
 *   lse2 beside them in the same order.  A wave owns 32 codes and sums p over the rows of one position at a time; the
 *   positions (never the rows of one position) are split over workgroups, the heads' partial tables are added in head order.
 *   No float atomics: bit-identical results from run to run on one device.  The sweep's work grows with Cp / (M / N): up
 *   to 32x for one row per position.
 *   Workspace (>= vq_diversity_workspace_bytes bytes, 16-byte aligned; 0 = unsupported shape), in 4-byte units, with
 *   Mp = N*Cp rounded up to the staged tile (32 * max(1, 256 / Dp) rows, Dp = D rounded up to 32 / 64 / 128 / 256) and
 *   rsK = vq_gumbel_row_stride(K):
 *     [x image: H * (Mp*(Dp + 4) + 2048)][lse2 in image order: H*Mp][partials of A: H*N*rsK]
 *   More than 2^31 - 1 rows or an image of 2 GiB or more: VQ_E_UNSUPPORTED (use row chunks).
 * vq_diversity_delta_f32 (a->packed): delta from lse2 and U, as sum_k p U / sum_k p with the p it summed (1 within rounding).
 *   w, and with it grad_x, does not change when a constant is added to a row of U (delta moves with it): a caller who
 *   subtracts a per-position constant near the row's values first shrinks every rounding error of delta and of U - delta by
 *   |U - constant| / |U|.
 * vq_diversity_backward_x_f32 (a->packed): grad_x (h, m, d) at grad_x[h*gx_hs + m*gx_rs + d].  live_packed: NULL, or the
 *   packed images of the live codes (vq_pack_codebooks_f32 of [H][K][D] with the same metric, head stride live_pk_hs floats);
 *   an image bit-equal to a->packed gives bit for bit the result of NULL.
 * vq_diversity_backward_codes_f32 (a->cb, the natural codes; lse2, delta and U as for backward_x, in the caller's row order):
 *   grad_codes [H][K][D] contiguous.  It packs the position-major image of vq_diversity_accumulate_f32 again (the forward's
 *   workspace need not outlive the forward), lse2 and delta beside it in image order.  A wave owns 32 codes and recomputes p
 *   with the expression the other sweeps rounded it with; w / r of a position's padding rows is selected to 0.  The staged
 *   tiles are split over workgroups by the plan of vq_gumbel_backward_codes_f32 (splits = min(64, tiles, ceil(CUs / (H *
 *   ceil(K / 128)))) regrouped into equal runs of tiles), every split stores its partial and the partials are added in
 *   split order: no float atomics, bit-identical results from run to run on one device.  Also VQ_E_BADARG: a->cb or
 *   grad_codes null, a workspace that is too small or misaligned.
 *   Workspace (>= vq_diversity_codes_workspace_bytes bytes, 16-byte aligned; 0 for exactly the shapes
 *   vq_diversity_workspace_bytes gives 0 for), in 4-byte units, Mp and Dp as above:
 *     [x image: H * (Mp*(Dp + 4) + 2048)][lse2 in image order: H*Mp][delta in image order: H*Mp]
 *     [grad_codes partials: splits*H*K*D, only when splits > 1]
 */
int64_t vq_diversity_workspace_bytes(int H, int64_t M, int K, int D, int N);
int vq_diversity_stats_f32(const vq_args *a, float T, float *lse2, void *stream);
int vq_diversity_accumulate_f32(const vq_args *a, float T, int N, int pos_div, const float *lse2, float *A, void *workspace,
                                int64_t workspace_bytes, void *stream);
int vq_diversity_delta_f32(const vq_args *a, float T, int N, int pos_div, const float *lse2, const float *U, float *delta,
                           void *stream);
int vq_diversity_backward_x_f32(const vq_args *a, const float *live_packed, int64_t live_pk_hs, float T, int N, int pos_div,
                                const float *lse2, const float *delta, const float *U, float *grad_x, int64_t gx_rs, int64_t gx_hs,
                                void *stream);
int64_t vq_diversity_codes_workspace_bytes(int H, int64_t M, int K, int D, int N);
int vq_diversity_backward_codes_f32(const vq_args *a, float T, int N, int pos_div, const float *lse2, const float *delta,
                                    const float *U, float *grad_codes, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Orthogonal regularisation loss (utils/losses.py:23-28) without the [n, n] cosine matrix: one sweep with the same rows on
 * both sides.  With x the n rows of a head AS GIVEN -- the entry does not normalise; the caller hands in F.normalize(codes)
 * and differentiates through the normalisation itself; it is defined for any finite rows --
 *   cos_ij  = x_i . x_j
 *   rowsq_i = sum_j cos_ij^2                          (row sums of squares)
 *   G_i     = sum_j cos_ij x_j                        (the gram matrix times the rows, [n][D])
 *   loss    = sum_{h,i} rowsq_i / (H n^2) - 1 / n     d loss / d x_i = 4 G_i / (H n^2)   (cos is symmetric)
 * Reads a->H, a->K (= n, the number of rows), a->D (<= 256: VQ_E_UNSUPPORTED beyond), a->metric (must be VQ_METRIC_DOT),
 * a->x with x_rs / x_hs (the resident rows [H][n][D]; D and strides need not be multiples of 4) and a->packed with pk_hs
 * (vq_pack_codebooks_f32 of the SAME rows with VQ_METRIC_DOT, K = n).  M, Q, cb and everything else are ignored.
 * rowsq: [H][vq_gumbel_row_stride(n)] floats, 16-byte aligned; entries past n are not written.  gram: NULL (only rowsq is
 * produced, the contraction is skipped) or G with (h, i, d) at gram[h*g_hs + i*g_rs + d], 16-byte aligned base, any strides.
 * Checked before any launch (VQ_E_BADARG, vq_last_error names the argument): non-positive H, K or D, a metric other than dot,
 * null x or packed, a null or misaligned rowsq, a misaligned gram.
 * fp32 MFMA throughout.  The image's padding codes and a workgroup's rows past n contribute exactly nothing (selected to 0
 * by index); a NaN / inf in a real row reaches rowsq and G of every row.  Every rowsq entry and G row is accumulated by one
 * lane set in tile order: no float atomics, bit-identical results from run to run on one device.
 */
int vq_orthogonal_gram_f32(const vq_args *a, float *rowsq, float *gram, int64_t g_rs, int64_t g_hs, void *stream);

/*
 * Gumbel-max sampling of the code, utils/general.py:112-129 (ind = argmax(similarities / temperature + gumbel_noise)) with
 * the noise of utils/general.py:25-30, as an epilogue of the similarity sweep: nothing of [M, K] in memory, one launch.
 *   idx[h*idx_hs + m*idx_rs] = first index of the maximum over k < K of  key = fl(fl(s * tau) + g)
 * with s the value vq_similarities_f32 writes (bit for bit), tau = 1 / temperature in fp32 and g the noise below; a NaN key
 * is the maximum and the lowest code wins among equal maxima (ATen's argmax).  Uses a->x, a->packed, a->idx (idx_rs, idx_hs),
 * H, M, K, D (<= 512: VQ_E_UNSUPPORTED beyond), metric; Q is ignored.  tau must be finite.
 * seed: TWO 64-bit words on the DEVICE (no host synchronisation; capturable in a hipGraph).
 *
 * The noise of entry (h, m, k) depends on (seed, h, m, k) only, never on the launch geometry: Philox4x32-10 with
 *   key      k0 = seed[0] bits 31..0, k1 = seed[0] bits 63..32
 *   counter  c0 = m bits 31..0, c1 = m bits 63..32, (c3 : c2) = ((h << 32) | (k >> 2)) + seed[1]  (mod 2^64, c2 the low word)
 * yields four 32-bit words; word k & 3 gives u = (word >> 8) * 2^-24 in [0, 1) and g = -log(max(-log(max(u, 1e-5)), 1e-5)).
 * vq_gumbel_noise_f32 writes exactly that g to noise[(h*M + m)*K + k] and, when bits is not NULL, the word to
 * bits[(h*M + m)*K + k] -- the hook that makes vq_gumbel_sample_f32 checkable entry by entry; no product path uses it.
 */
int vq_gumbel_sample_f32(const vq_args *a, float tau, const int64_t *seed /* 2 words, device */, void *stream);
int vq_gumbel_noise_f32(const int64_t *seed, int H, int64_t M, int K, float *noise, uint32_t *bits /* may be NULL */, void *stream);

/*
 * Lookup-free quantization (LFQ) over C codebooks of d sign bits each, 1 <= d <= 20 (implicit codebook {-a, +a}^d).
 * v: [N][C][d] fp32, element (m, c, i) at v[m * v_rs + c * d + i] (rows may be strided, each row's C * d values contiguous).
 *
 * vq_lfq_quantize_f32 -- the quantize step, lookup_free_quantization.py:250-276 (and the commitment loss, :323-336):
 *   q[(m * C + c) * d + i] = v > 0 ? qmag : -qmag  (0 and NaN give -qmag; qmag = codebook_scale, or the spherical code's
 *   l2-normalised magnitude); idx[m * C + c] = sum_i (v > 0) << (d - 1 - i)  (dim 0 is the MSB, the reference's mask);
 *   out (may be NULL) = xa + (q - xa) with xa [N][C][d] at xa[m * xa_rs + c * d + i] (straight-through, :281-283);
 *   commit_sum (device double, may be NULL) = sum over rows with mask[m] != 0 (mask NULL: all rows) of (v - q)^2, fixed
 *   summation order.  workspace: vq_lfq_workspace_bytes(N, 0, C, d) bytes when commit_sum is set.
 * vq_lfq_entropy_fwd_f32 -- the entropy aux loss, lookup_free_quantization.py:294-331, for the R rows listed in `rows`
 *   (int64 row numbers of v; NULL = rows 0 .. R-1), with a = code_scale and tau = inv_temperature:
 *   per_sample_sum (device double) = sum over (row, c) of -sum_k p_k log(max(p_k, 1e-5));  avg_prob [C][2^d] =
 *   mean over the rows of p  (p = softmax_k(2 tau a sum_i v_i (2 b_{k,i} - 1)), factorised per dim: no [R][2^d] buffer).
 *   workspace: vq_lfq_workspace_bytes(R, R, C, d) bytes (O(R * C * 2^ceil(d/2) + C * 2^d)).  Fixed summation order.
 * vq_lfq_entropy_bwd_f32 -- its backward with respect to v for the same rows (other rows of grad_v are not written):
 *   grad_v = d/dv [ w_ps[0] * sum_(row, c) H(p) + sum_(row, c, k) w_cb[c * 2^d + k] * p_k ]  where H(p) is the clamped entropy
 *   above;  the caller folds the upstream gradients and every mean factor into the device scalar w_ps and the table w_cb
 *   (for the codebook entropy: w_cb = g * dH/d avg_prob / (C * R * world size)).
 */
int64_t vq_lfq_workspace_bytes(int64_t N, int64_t R, int C, int d);
int vq_lfq_quantize_f32(const float *v, int64_t v_rs, const float *xa, int64_t xa_rs, int64_t N, int C, int d, float qmag,
                        const uint8_t *mask, float *q, float *out, int64_t *idx, double *commit_sum, void *workspace,
                        int64_t workspace_bytes, void *stream);
int vq_lfq_entropy_fwd_f32(const float *v, int64_t v_rs, const int64_t *rows, int64_t R, int C, int d, float code_scale,
                           float inv_temperature, float *avg_prob, double *per_sample_sum, void *workspace,
                           int64_t workspace_bytes, void *stream);
int vq_lfq_entropy_bwd_f32(const float *v, int64_t v_rs, const int64_t *rows, int64_t R, int C, int d, float code_scale,
                           float inv_temperature, const float *w_ps, const float *w_cb, float *grad_v, int64_t gv_rs,
                           void *stream);

/*
 * Residual LFQ (ResidualLFQ / GroupedResidualLFQ, residual_lfq.py of the reference), one codebook of d bits per stage.
 *
 * vq_lfq_entropy_staged_fwd_f32 / vq_lfq_entropy_staged_bwd_f32 -- vq_lfq_entropy_{fwd,bwd}_f32 (C = 1) for T stages in one
 *   call: stage t reads v + t * v_ss (rows [R][d] at row stride v_rs) and the row list rows + t * rows_ss (rows NULL: rows
 *   0 .. R-1 of every stage; rows_ss = 0: one list for all stages), uses code scale code_scale[t % period] (a device
 *   array of period floats), and writes per_sample_sum[t], avg_prob[t * 2^d ...] (forward) or reads
 *   w_ps[t], w_cb[t * 2^d ...] and writes grad_v + t * gv_ss (backward).  Stage t is bitwise equal to a single-stage call
 *   on its own inputs (same kernels, same row split, same summation order).  workspace: vq_lfq_staged_workspace_bytes(R, T, d)
 *   bytes (T times a single-stage call's).
 */
int64_t vq_lfq_staged_workspace_bytes(int64_t R, int T, int d);
int vq_lfq_entropy_staged_fwd_f32(const float *v, int64_t v_rs, int64_t v_ss, const int64_t *rows, int64_t rows_ss, int64_t R,
                                  int T, int d, const float *code_scale, int period, float inv_temperature, float *avg_prob,
                                  double *per_sample_sum, void *workspace, int64_t workspace_bytes, void *stream);
int vq_lfq_entropy_staged_bwd_f32(const float *v, int64_t v_rs, int64_t v_ss, const int64_t *rows, int64_t rows_ss, int64_t R,
                                  int T, int d, const float *code_scale, int period, float inv_temperature, const float *w_ps,
                                  const float *w_cb, float *grad_v, int64_t gv_rs, int64_t gv_ss, void *stream);

/*
 * vq_rlfq_quantize_f32 -- all S stages' quantize steps of G groups in one pass, each row's d <= 20 values in registers.
 *   Row m of group g is x[g * x_gs + m * x_rs + i] (i < d, contiguous).  stage_consts: device floats [3][S], rows
 *   qmag (|code entry| of stage s: its codebook scale, or the l2-normalised code's magnitude), clamp (soft clamp value,
 *   0 = none) and scale (codebook scale, the spherical l2norm's factor).  Per stage s:
 *   u = clamp[s] > 0 ? tanh(r / clamp[s]) * clamp[s] : r;  v = spherical ? u / max(|u|, 1e-12) * scale[s] : u;
 *   q = v > 0 ? qmag[s] : -qmag[s];  o = ste ? v + (q - v) : q;  r -= o;  out += o  (r starts at x, out at 0, stage order).
 *   Writes out[g * out_gs + m * out_rs + i], idx[(g * N + m) * S + s] (MSB first), v_all (may be NULL) [G][S][N][d] the stage
 *   inputs v, and commit_sum (device doubles, may be NULL) [G][S] = sum over rows with mask[m] != 0 (mask NULL: all) of
 *   (v - q)^2, each in the fixed order of vq_lfq_quantize_f32 (workspace: vq_rlfq_workspace_bytes(G, N, S) bytes).
 *   Without clamp and l2norm, out, idx and commit_sum are bitwise those of S vq_lfq_quantize_f32 calls chained in torch.
 * vq_rlfq_backward_f32 -- grad_x of the same chain (training, ste):  grad_x = sum_s J_s^T (g_out + (v - q) * w_commit[g * S + s]
 *   * mask + g_ent[((g * S + s) * N + m) * d + i]), J_s the clamp and l2norm Jacobians (the residual is detached, so
 *   d r_s / d x = I).  g_out, w_commit (device [G][S], 2 * the commitment sums' upstream gradient) and g_ent may be NULL.
 * Limits: 1 <= d <= 20, 1 <= S <= VQ_RLFQ_MAX_STAGES, 1 <= G <= 65535.
 */
#define VQ_RLFQ_MAX_STAGES 32
int64_t vq_rlfq_workspace_bytes(int64_t G, int64_t N, int S);
int vq_rlfq_quantize_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, int S, const float *stage_consts,
                         int spherical, int ste, const uint8_t *mask, float *out, int64_t out_gs, int64_t out_rs, int64_t *idx,
                         float *v_all, double *commit_sum, void *workspace, int64_t workspace_bytes, void *stream);
int vq_rlfq_backward_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, int S, const float *stage_consts,
                         int spherical, const uint8_t *mask, const float *g_out, int64_t g_gs, int64_t g_rs,
                         const float *w_commit, const float *g_ent, float *grad_x, int64_t gx_gs, int64_t gx_rs, void *stream);

/*
 * vq_fsq_quantize_f32 -- finite scalar quantization (FSQ, ResidualFSQ): all S stages of G groups in one pass, one thread per
 *   row of d <= 16 values.  Row m of group g is x[g * x_gs + m * x_rs + i] (i < d, contiguous).  levels: HOST int32 [d]
 *   (each >= 2; basis = cumprod of the levels before, which must fit int32).  consts: DEVICE floats [3 + S][d], rows
 *   half_l, offset, shift (the reference's bound constants, computed by the caller), then the S stage scales.  With
 *   bound(z) = tanh(z + shift) * half_l - offset and hw = L / 2, r starts at x (prebound = 0) or bound(x) (prebound = 1,
 *   ResidualFSQ), and per stage s:  c = rint(bound(r / scale[s])) / hw;  o = c * scale[s];  r -= o;  out += o  (out from
 *   +0, stage order);  idx[(g * N + m) * S + s] = (int32) sum_i ((c_i * hw_i) + hw_i) * basis_i in fp32, summed in the
 *   order of torch's CPU sum over d <= 7 (partials k < 4 from term k, terms 4 .. d-1 into partial 0, then p0 += p1, p2,
 *   p3), truncated; NaN gives INT32_MIN.  Writes out[g * out_gs + m * out_rs + i]; idx may be NULL.
 * vq_fsq_backward_f32 -- grad_x of the same chain (straight-through rounding):  grad_x = [bound'(x) if prebound] *
 *   sum_s bound'(r_s / scale[s]) / hw * g_out, recomputing r_s from x with the forward's code.  No atomics.
 * vq_fsq_decode_f32 -- idx [N][Q] (int32, or int64 when idx_64) -> codes ((i // basis) % L - hw) / hw * scales[q][i]
 *   (floor division and Python modulo, as torch's integer // and %), scales a DEVICE float array [Q][d].  With drop_null,
 *   an index of -1 gives a zero code.  codes_sum [N][d] (the sum over q in stage order) and all_codes [Q][N][d] may each
 *   be NULL, not both.
 * Errors (-1, vq_last_error): a null pointer, d outside [1, 16], a level below 2, G, N, S (Q) not positive, G > 65535.
 */
int vq_fsq_quantize_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, const int32_t *levels, int S,
                        const float *consts, int prebound, float *out, int64_t out_gs, int64_t out_rs, int32_t *idx,
                        void *stream);
int vq_fsq_backward_f32(const float *x, int64_t x_gs, int64_t x_rs, int64_t G, int64_t N, int d, const int32_t *levels, int S,
                        const float *consts, int prebound, const float *g_out, int64_t g_gs, int64_t g_rs, float *grad_x,
                        int64_t gx_gs, int64_t gx_rs, void *stream);
int vq_fsq_decode_f32(const void *idx, int idx_64, int64_t N, int Q, int d, const int32_t *levels, const float *scales,
                      int drop_null, float *codes_sum, float *all_codes, void *stream);

/*
 * vq_decode_f32 -- indices -> code vectors for VectorQuantize / ResidualVQ / GroupedResidualVQ in one pass: the gather of
 *   every stage's code and their sum, with nothing of [Q][N][D] in between (replaces vector_quantize_pytorch.py:156-180,
 *   residual_vq.py:94-132,293-305: Q gathers, a masked_fill over [Q][N][D] and a reduce over it again).
 *   Code (g, q, k) is cb[g * cb_gs + q * cb_qs + k * D + d] (cb_qs = 0: all stages share one codebook; cb_gs = 0: all
 *   groups do).  Index (g, n, q), q < Q_given <= Q, is idx[g * idx_gs + n * idx_rs + q * idx_qs] (int32, or int64 when
 *   idx_64; strides in elements, so a [.., :Q_given] view of a wider tensor is read in place); the stages q >= Q_given are
 *   dropped.  With t_q = the code of stage q, or +0.0 when the stage is dropped:
 *     all_codes[q * all_qs + g * all_gs + n * all_rs + d] = t_q                       (a bit copy of the codebook row)
 *     codes_sum[g * sum_gs + n * sum_rs + d * sum_ds]     = ((0 + t_0) + t_1) + ...   (one fp32 add per stage, stage order:
 *                                                            the order of vq_quantize_f32's `out`)
 *   Either output may be NULL, not both.  The strides let one call write a multi-head result already concatenated on the
 *   feature axis (sum_gs = D, sum_rs = G * D) or a channel-first result (sum_ds = the positions of a sample, sum_rs = 1,
 *   the samples on the group axis with cb_gs = 0).
 *   Index rule: drop_null = 1 (ResidualVQ, residual_vq.py:108-121): any i < 0 is a dropped stage.  drop_null = 0 (ATen's
 *   indexing, vector_quantize_pytorch.py:161): i in [-K, -1] means i + K.  In both, an index outside the valid range never
 *   becomes an address; it contributes +0.0 (ATen raises a device-side assert there: validating would cost the host a
 *   synchronisation).  A dropped stage's code is not read into the result: a NaN in code 0 does not leak.
 *   No host read, no allocation: the call can be captured in a hipGraph.  N == 0 returns 0 without a launch.
 * Errors (VQ_E_BADARG, vq_last_error; the device is not touched): cb or idx NULL, both outputs NULL, G, Q, K or D not
 *   positive, N negative, Q_given outside [1, Q], G * N * D beyond int64.
 */
int vq_decode_f32(const float *cb, int64_t cb_gs, int64_t cb_qs, int G, int Q, int K, int D,
                  const void *idx, int idx_64, int64_t idx_gs, int64_t idx_rs, int64_t idx_qs, int64_t N, int Q_given,
                  int drop_null,
                  float *codes_sum, int64_t sum_gs, int64_t sum_rs, int64_t sum_ds,   /* may be NULL; sum_ds != 1: channel-first */
                  float *all_codes, int64_t all_qs, int64_t all_gs, int64_t all_rs,   /* may be NULL */
                  void *stream);

/*
 * vq_residual_mask_f32 -- the mask pass of a residual stack: what ResidualVQ / GroupedResidualVQ compute with `mask=`
 *   (residual_vq.py:212-243 over vector_quantize_pytorch.py:347-364,413-418), from the indices vq_quantize_f32 wrote for ALL rows.
 *   Row (g, m) is x[g * x_gs + m * x_rs + d], code (g, q, k) is cb[g * cb_gs + q * cb_qs + k * D + d] (cb_qs = 0: the stages
 *   share one codebook), its index of stage q is idx[g * idx_gs + m * idx_rs + q * idx_qs], its mask byte is
 *   mask[g * mask_gs + m] (mask_gs = 0: every group uses the same mask; non-zero = kept).  Strides in elements.
 *   Per row, with r_0 = x, acc = +0.0, for q = 0 .. Q-1, every operation one IEEE fp32 operation in this order:
 *     kept row:        c = cb[g][q][idx_q];  e_q += sum_d (c - r_q)^2;  quant = train ? r_q + (c - r_q) : c
 *     masked-out row:  quant = r_q      (where(mask, quantize, orig_input), vector_quantize_pytorch.py:415-418)
 *     both:            acc = acc + quant;  r_{q+1} = r_q - quant  (residual_vq.py:232);  out = acc after the last stage
 *   A finite masked-out row so has r_q = 0 for q >= 1 and out = x.  The reference searches that zero row: the call WRITES
 *     idx_q = zero_idx[g * Q + q]  for q >= 1 on masked-out rows that are finite in every element (zero_idx: the answer
 *             of stage q's codebook to the all-zero row, from vq_quantize_f32 itself),
 *     idx_q = 0                    for q >= 1 on masked-out rows that hold a non-finite element (r_1 has a NaN there, and a
 *             row holding a NaN answers code 0; the NaN reaches out in those elements).
 *   idx of kept rows and stage 0 of every row are only read.  An index outside [0, K) never becomes an address: code 0 of
 *   the stage is read in its place.
 *   sq_err (may be NULL): device doubles, [Q] (the sum over all groups) or [G][Q] with sq_err_per_group, e_q summed over
 *   the KEPT rows only (the commitment loss is the mean over mask, vector_quantize_pytorch.py:347-360; no kept row: 0).  One
 *   fp32 partial per stage and <= 32 rows in `workspace`, then a fixed-order fp64 sum: no atomics, run-to-run identical.
 *   workspace (used only with sq_err): 4-byte aligned, 4 * G * Q * ceil(M / 2) bytes always suffice.
 *   No host read, no allocation: capturable in a hipGraph.  M == 0 returns 0 without a launch (sq_err is zeroed).
 * vq_residual_mask_backward_f32 -- its backward with respect to x, the masked counterpart of vq_quantize_backward_f32:
 *     grad_x[m] = (train ? Q * grad_out[m] : 0) + (mask[m] ? sum_q 2 * grad_sq_err[q] * (r_q - c_q[idx_q]) : 0)
 *   with the chain r_q rebuilt in the forward's fp32 order (every layer returns its input on a masked-out row, and every
 *   residual is x minus detached terms: d out / d x = Q * I there too).  grad_out (laid out like out) and grad_sq_err ([Q],
 *   or [G][Q] with sq_err_per_group, device doubles, read on the device) may each be NULL.  idx is only read.
 * Errors (VQ_E_BADARG, vq_last_error; the device is not touched): G outside [1, 65535], Q or K not positive, M negative,
 *   D outside [1, 512] (what one fused residual launch takes), G * M * D beyond int64, and with M > 0 a NULL x, cb, idx,
 *   mask, out / grad_x or zero_idx, or a workspace that is NULL, misaligned or too small while sq_err is given.
 */
int vq_residual_mask_f32(const float *x, int64_t x_gs, int64_t x_rs, const float *cb, int64_t cb_gs, int64_t cb_qs,
                         int64_t *idx, int64_t idx_gs, int64_t idx_rs, int64_t idx_qs,
                         const uint8_t *mask, int64_t mask_gs, const int64_t *zero_idx,
                         int G, int64_t M, int Q, int K, int D, int train,
                         float *out, int64_t out_gs, int64_t out_rs,
                         double *sq_err, int sq_err_per_group, void *workspace, int64_t workspace_bytes, void *stream);
int vq_residual_mask_backward_f32(const float *x, int64_t x_gs, int64_t x_rs, const float *cb, int64_t cb_gs, int64_t cb_qs,
                                  const int64_t *idx, int64_t idx_gs, int64_t idx_rs, int64_t idx_qs,
                                  const uint8_t *mask, int64_t mask_gs,
                                  int G, int64_t M, int Q, int K, int D, int train,
                                  const float *grad_out, int64_t go_gs, int64_t go_rs,
                                  const double *grad_sq_err, int sq_err_per_group,
                                  float *grad_x, int64_t gx_gs, int64_t gx_rs, void *stream);

/*
 * vq_lfq_decode_f32 -- indices -> code vectors for LFQ / ResidualLFQ / GroupedResidualLFQ in one pass.  The lookup-free
 *   family has no table: a code is a function of the index bits alone (replaces lookup_free_quantization.py:193-220,
 *   residual_lfq.py:80-118,240-252: per stage a cast, an and, a compare, a convert and a scale, then a stack, a masked_fill
 *   over [Q][N][d] and a reduce over it again).  The conventions are vq_decode_f32's.
 *   Index (g, n, q), q < Q_given <= Q, is idx[g * idx_gs + n * idx_rs + q * idx_qs] (int32, or int64 when idx_64; strides in
 *   elements, so any view is read in place); the stages q >= Q_given are dropped.  mag: Q host floats, the magnitude of
 *   every entry of a stage's codes (read on the host during the call; nothing is allocated).  With
 *     t_q[j] = +0.0 when stage q is dropped, else +mag[q] when bit d-1-j of the index is set, else -mag[q]
 *   (MSB first, the modules' mask = 2 ** arange(d-1, -1, -1); only the low 32 bits of an int64 index count, their .int()):
 *     all_codes[q * all_qs + g * all_gs + n * all_rs + j] = t_q[j]
 *     codes_sum[g * sum_gs + n * sum_rs + j * sum_ds]     = ((0 + t_0[j]) + t_1[j]) + ...   (one fp32 add per stage, stage order)
 *   Either output may be NULL, not both.  sum_gs = d, sum_rs = G * d writes a result already concatenated over the groups
 *   (LFQ's num_codebooks, GroupedResidualLFQ's groups) on the feature axis.
 *   drop_null = 1 (ResidualLFQ, residual_lfq.py:98): an index EQUAL to -1, the whole int64 value, is a dropped stage and
 *   nothing else is.  drop_null = 0 (LFQ): -1 is all bits set, the all-positive code.  No index value is invalid and none
 *   becomes an address.  No host read of device memory, no allocation: the call can be captured in a hipGraph.
 *   N == 0 returns 0 without a launch.
 * Errors (VQ_E_BADARG, vq_last_error; the device is not touched): idx or mag NULL, both outputs NULL, d outside [1, 20],
 *   Q outside [1, VQ_RLFQ_MAX_STAGES], Q_given outside [1, Q], G outside [1, 65535], N negative or N * d beyond 2^39.
 */
int vq_lfq_decode_f32(const void *idx, int idx_64, int64_t idx_gs, int64_t idx_rs, int64_t idx_qs, int G, int64_t N,
                      int Q_given, int Q, int d, const float *mag, int drop_null,
                      float *codes_sum, int64_t sum_gs, int64_t sum_rs, int64_t sum_ds,   /* may be NULL */
                      float *all_codes, int64_t all_qs, int64_t all_gs, int64_t all_rs,   /* may be NULL */
                      void *stream);

/*
 * vq_lq_quantize_f32 -- latent quantization (LatentQuantize): the per-dimension level search of every (batch, position,
 *   codebook) sub-row in one pass, one thread per sub-row of d <= 16 values.  Element i of sub-row (b, p, c) is
 *   z[b * z_bs + p * z_ps + (c * d + i) * z_cs] (strides in elements: a channel-first [B][C * d][P] tensor is z_ps = 1,
 *   z_cs = P; a channel-last one z_ps = C * d, z_cs = 1); codes is written with its own three strides.  levels: HOST int32
 *   [d] (each >= 2, their product below 2^31).  tables: DEVICE floats, the d value tables back to back (table i holds
 *   levels[i] floats at offset levels[0] + .. + levels[i-1]; any order, duplicates allowed; at most 4096 floats).  Per
 *   dimension:  j = argmin_j |z_i - v_i[j]| (the first minimum; a NaN distance is the minimum, the first NaN wins, as
 *   ATen's argmin);  q = v_i[j];  c_i = z_i + (q - z_i);  t_i = ((c_i * 2) * hw_i + hw_i) * basis_i (hw = L / 2, basis =
 *   cumprod of the levels before), every step one fp32 operation.  idx[(b * P + p) * C + c] = (int32) sum_i t_i, summed
 *   and truncated as vq_fsq_quantize_f32 does (NaN or out of range: INT32_MIN); idx may be NULL.
 *   loss (DEVICE float[2], may be NULL): loss[1] = m = sum (c_i - z_i)^2 / (B * P * C * d) (fp32 per-workgroup partials in
 *   workspace, added in a fixed order in fp64: no atomics), loss[0] = w_c * m + w_q * m in fp32, a zero weight
 *   multiplying 0 instead of m.  workspace: vq_lq_workspace_bytes(B, P, C) bytes when loss is given.
 * vq_lq_backward_f32 -- grad_x = g_out + (g_loss[0] * coef) * (out - x) over [B][P][W] elements, each tensor with its own
 *   three strides (batch, position, channel); g_loss a DEVICE scalar.  With coef = 2 / numel * (w_c - w_q) it is dL/dx of
 *   vq_lq_quantize_f32's codes and loss[0] (the straight-through value passes g_out on unchanged).
 * Errors (-1, vq_last_error): a null pointer, d outside [1, 16], a level below 2, a codebook size or a row count that
 *   overflows, tables above 4096 floats, B, P, C (W) not positive, a workspace that is too small.
 */
int64_t vq_lq_workspace_bytes(int64_t B, int64_t P, int C);
int vq_lq_quantize_f32(const float *z, int64_t z_bs, int64_t z_ps, int64_t z_cs, int64_t B, int64_t P, int C, int d,
                       const int32_t *levels, const float *tables, float *codes, int64_t c_bs, int64_t c_ps, int64_t c_cs,
                       int32_t *idx, float *loss, float w_c, float w_q, void *workspace, int64_t workspace_bytes,
                       void *stream);
int vq_lq_backward_f32(const float *x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float *out, int64_t o_bs, int64_t o_ps,
                       int64_t o_cs, const float *g_out, int64_t g_bs, int64_t g_ps, int64_t g_cs, const float *g_loss,
                       float coef, int64_t B, int64_t P, int W, float *grad_x, int64_t gx_bs, int64_t gx_ps, int64_t gx_cs,
                       void *stream);

const char *vq_last_error(void);
int vq_device_info(char *buf, size_t n); /* "gfx950 ... CUs" of the current device */

#ifdef __cplusplus
}
#endif
#endif /* VQ_MI355X_H */
