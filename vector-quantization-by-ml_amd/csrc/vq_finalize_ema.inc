// vq_finalize_ema.inc -- scalar fallback search, finalize-from-keys, loss reduction, EMA codebook update.
// Included by vq_kernels.hip.
// ------------------------------------------------------------------------------------------------
// scalar-FMA fallback search: one thread per row, any D / K.  Same chain order as the MFMA kernel
// (and the oracle), so it doubles as an on-device cross-check.  Emits packed keys.
// ------------------------------------------------------------------------------------------------
template <int METRIC>
__global__ void vq_search_simple(const float *__restrict__ x, long long x_rs, long long x_hs,
                                 const float *__restrict__ cb, long long cb_hs, long long M, int K, int D,
                                 long long idx_offset, long long *__restrict__ keys) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M) return;
    const int head = blockIdx.y;
    const float *xr = x + (long long)head * x_hs + row * x_rs;
    const float *c0 = cb + (long long)head * cb_hs;
    float xn = 0.0f;
    if (METRIC == VQ_METRIC_EUCLID)
        for (int d = 0; d < D; ++d) xn = fmaf(xr[d], xr[d], xn);
    float best = (METRIC == VQ_METRIC_EUCLID) ? __builtin_inff() : -__builtin_inff();
    int bi = 0;
    bool got_nan = false;  // a NaN similarity is argmax's maximum: the first one wins (utils/general.py:128)
    for (int k = 0; k < K && !got_nan; ++k) {
        const float *cr = c0 + (long long)k * D;
        float acc = 0.0f;
        if (METRIC == VQ_METRIC_EUCLID) {
            float cn = 0.0f;
            for (int d = 0; d < D; ++d) {
                const float cv = cr[d];
                acc = fmaf(xr[d], -2.0f * cv, acc);
                cn = fmaf(cv, cv, cn);
            }
            acc = fmaf(1.0f, xn, acc);
            acc = fmaf(cn, 1.0f, acc);
            const float s = sqrtf(acc < 0.0f ? 0.0f : acc);  // clamp_min_(0) keeps NaN
            if (s != s || s < best) {
                best = s;
                bi = k;
                got_nan = s != s;
            }
        } else {
            for (int d = 0; d < D; ++d) acc = fmaf(xr[d], cr[d], acc);
            if (acc != acc || acc > best) {
                best = acc;
                bi = k;
                got_nan = acc != acc;
            }
        }
    }
    atomicMin(keys + (long long)head * M + row, make_key<METRIC>(best, idx_offset + bi));
}

__global__ void vq_keys_init_kernel(long long *keys, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = 0x7FFFFFFFFFFFFFFFll;
}

// ------------------------------------------------------------------------------------------------
// finalize from keys: one wave per row (grid-strided), natural layout
// ------------------------------------------------------------------------------------------------
struct FinalizeParams {
    const long long *keys;   // [nparts][H][M]: the winner of a row is the MIN over the planes (K splits x shards)
    int nparts;
    long long part_stride;
    const float *x;
    long long x_rs, x_hs;
    const float *cb;
    long long cb_hs;
    float *out;
    long long out_rs, out_hs;
    long long *idx;
    long long idx_rs, idx_hs;
    float *best;
    float *loss_part;  // [H][gridDim.x * 4]
    long long M;
    int D, metric, ste;
    int vec;  // x / cb / out rows may be accessed as float4 (D % 4 == 0, strides % 4 == 0, 16-byte aligned bases)
    // one stage of a residual stack run stage by stage (the K-split tail of a residual launch; residual_vq.py:232-233):
    float *res_next;  // != NULL: r_{q+1} = r_q - quant_q goes here ([H][M][D] contiguous; may alias x: a row is read before it is written)
    int out_acc;      // out = out + quant_q instead of 0.0 + quant_q (stages after the first)
    int residual;     // this is a stage of a stack: out accumulates from 0.0 (the fused kernel's `o = 0; o = o + quant`)
};

// RESIDUAL: a stage of a residual stack run stage by stage (res_next / out_acc / residual are read in that instantiation only: the
// plain one -- the sharded step's finalize among others -- keeps its round-2 code)
template <bool RESIDUAL>
__global__ void __launch_bounds__(256) vq_finalize_kernel(const FinalizeParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int head = blockIdx.y;
    const long long nw = (long long)gridDim.x * 4;
    float e = 0.0f;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < p.M; row += nw) {
        long long key = p.keys[(long long)head * p.M + row];
        if (p.nparts > 1) {  // candidates of the K splits / shards: lanes take planes, one butterfly
            key = 0x7FFFFFFFFFFFFFFFll;
            for (int cnd = lane; cnd < p.nparts; cnd += 64) {
                const long long k2 = p.keys[(long long)cnd * p.part_stride + (long long)head * p.M + row];
                key = k2 < key ? k2 : key;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long k2 = __shfl_xor(key, o);
                key = k2 < key ? k2 : key;
            }
        }
        const long long i = (long long)(key & 0xFFFFFFFFll);
        if (lane == 0) {
            const long long o = (long long)head * p.idx_hs + row * p.idx_rs;
            if (p.idx) p.idx[o] = i;
            if (p.best) p.best[o] = key_value(key, p.metric);
        }
        const bool need_x = p.ste || p.loss_part || (RESIDUAL && p.res_next);
        if (!p.out && !p.loss_part && !(RESIDUAL && p.res_next)) continue;
        const float *xr = p.x + (long long)head * p.x_hs + row * p.x_rs;
        const float *crow = p.cb + (long long)head * p.cb_hs + i * p.D;
        float *orow = p.out ? p.out + (long long)head * p.out_hs + row * p.out_rs : nullptr;
        float *nrow = (RESIDUAL && p.res_next) ? p.res_next + ((long long)head * p.M + row) * p.D : nullptr;
        if (p.vec) {  // a wave moves 1 KiB of a row per access
            for (int d = 4 * lane; d < p.D; d += 256) {
                const f32x4 cv = *(const f32x4 *)(crow + d);
                f32x4 quant = cv;
                if (need_x) {
                    const f32x4 r = *(const f32x4 *)(xr + d);
                    const f32x4 diff = cv - r;
                    e = fmaf(diff.x, diff.x, e);
                    e = fmaf(diff.y, diff.y, e);
                    e = fmaf(diff.z, diff.z, e);
                    e = fmaf(diff.w, diff.w, e);
                    if (p.ste) quant = r + diff;
                    if (RESIDUAL && nrow) *(f32x4 *)(nrow + d) = r - quant;
                }
                if (orow) {
                    if (RESIDUAL) {
                        const f32x4 prev = p.out_acc ? *(const f32x4 *)(orow + d) : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                        *(f32x4 *)(orow + d) = prev + quant;
                    } else {
                        __builtin_nontemporal_store(quant, (f32x4 *)(orow + d));
                    }
                }
            }
            continue;
        }
        for (int d = lane; d < p.D; d += 64) {
            const float cv = crow[d];
            float quant = cv;
            if (need_x) {
                const float r = xr[d];
                const float diff = cv - r;
                e = fmaf(diff, diff, e);
                if (p.ste) quant = r + diff;
                if (RESIDUAL && nrow) nrow[d] = r - quant;
            }
            if (orow) orow[d] = RESIDUAL ? (p.out_acc ? orow[d] : 0.0f) + quant : quant;
        }
    }
    if (p.loss_part) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        if (lane == 0) p.loss_part[((long long)head * gridDim.x + blockIdx.x) * 4 + wave] = e;
    }
}

// sq_err[q] = sum over parts of loss_part[part*Q + q]   (double, fixed order)
__global__ void __launch_bounds__(256) vq_loss_reduce_kernel(const float *__restrict__ part, long long nparts, int Q,
                                                             double *__restrict__ sq_err, int accumulate = 0, int sq_err_hs = -1) {
    __shared__ double sh[256];
    const int q = blockIdx.x;
    part += (long long)blockIdx.y * nparts * Q;  // gridDim.y > 1: one sum per head (nparts = partials of ONE head)
    sq_err += (long long)blockIdx.y * (sq_err_hs >= 0 ? sq_err_hs : Q);  // (a stage of a stack run stage by stage: [H][Q of the stack])
    double s = 0.0;
    for (long long i = threadIdx.x; i < nparts; i += 256) s += (double)part[i * Q + q];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) sq_err[q] = accumulate ? sq_err[q] + sh[0] : sh[0];  // (accumulate: second part of a two-call launch plan)
}

// ------------------------------------------------------------------------------------------------
// backward of the quantize step with respect to x (autograd of vector_quantize_pytorch.py:261-279,361-364 and of the
// residual loop residual_vq.py:212-243): one pass over x / grad_out instead of PyTorch's gather + elementwise chain.
//   train (STE):  out = sum_q quant_q,  quant_q = r_q + (c_q - r_q).detach()  ->  d out / d x = Q * I
//   sq_err_q = sum (c_q - r_q)^2 with c_q detached                              ->  d / d x = 2 (r_q - c_q)
//   r_{q+1} = r_q - quant_q.detach()                                            (every residual is x minus constants)
// gx = (STE ? Q * grad_out : 0) + sum_q coef[q] * (r_q - c_q),  coef[q] = 2 * d loss / d sq_err_q.
// ------------------------------------------------------------------------------------------------
struct QuantBwdParams {
    const float *x;
    long long x_rs, x_hs;
    const float *cb;
    long long cb_hs, cb_qs;
    const long long *idx;
    long long idx_rs, idx_hs, idx_qs;
    const float *go;  // grad of out, or NULL
    long long go_rs, go_hs;
    const double *g_err;  // [Q] (or [H][Q] with g_err_hs = Q) grad of sq_err, or NULL
    long long g_err_hs;
    float *gx;
    long long gx_rs, gx_hs;
    long long M;
    int D, Q, ste, vec;
};

__global__ void __launch_bounds__(256) vq_quantize_backward_kernel(const QuantBwdParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.y;
    const long long nw = (long long)gridDim.x * 4;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float *cbh = p.cb + (long long)head * p.cb_hs;
    const long long *ih = p.idx + (long long)head * p.idx_hs;
    const float *goh = p.go ? p.go + (long long)head * p.go_hs : nullptr;
    float *gxh = p.gx + (long long)head * p.gx_hs;
    const float qf = (float)p.Q;
    const double *ge = p.g_err ? p.g_err + (long long)head * p.g_err_hs : nullptr;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < p.M; row += nw) {
        const float *xr = xh + row * p.x_rs;
        float *gr = gxh + row * p.gx_rs;
        if (p.vec) {
            for (int d = 4 * lane; d < p.D; d += 256) {
                f32x4 r = *(const f32x4 *)(xr + d);
                f32x4 g = {0.0f, 0.0f, 0.0f, 0.0f};
                if (p.ste && goh) g = __builtin_nontemporal_load((const f32x4 *)(goh + row * p.go_rs + d)) * qf;
                for (int q = 0; q < p.Q; ++q) {
                    const long long k = ih[row * p.idx_rs + q * p.idx_qs];
                    const f32x4 c = *(const f32x4 *)(cbh + (long long)q * p.cb_qs + k * p.D + d);
                    if (ge) g = g + (r - c) * (float)(2.0 * ge[q]);
                    const f32x4 quant = p.ste ? r + (c - r) : c;
                    r = r - quant;
                }
                __builtin_nontemporal_store(g, (f32x4 *)(gr + d));
            }
        } else {
            for (int d = lane; d < p.D; d += 64) {
                float r = xr[d];
                float g = (p.ste && goh) ? goh[row * p.go_rs + d] * qf : 0.0f;
                for (int q = 0; q < p.Q; ++q) {
                    const long long k = ih[row * p.idx_rs + q * p.idx_qs];
                    const float c = cbh[(long long)q * p.cb_qs + k * p.D + d];
                    if (ge) g += (r - c) * (float)(2.0 * ge[q]);
                    const float quant = p.ste ? r + (c - r) : c;
                    r = r - quant;
                }
                gr[d] = g;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// training-state step that follows the hot path (SURVEY 8f rank 1): exponential-moving-average update
//   counts[h,k]  = #rows of head h assigned to code k            (reference: embed_onehot.sum(1), codebooks.py:408)
//   sums[h,k,:]  = sum of those rows                              (einsum("h n d, h n c -> h c d"), codebooks.py:413)
// The reference builds both through the [h, M, K] one-hot tensor; here they are a scatter-add with float atomics
// shaped for the memory-side atomic units: one dword per lane, 256 contiguous bytes per wave instruction.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vq_ema_accumulate_kernel(const float *__restrict__ x, long long x_rs, long long x_hs,
                                                                const long long *__restrict__ idx, long long idx_rs,
                                                                long long idx_hs, const unsigned char *__restrict__ mask,
                                                                long long M, int K, int D, float *__restrict__ counts,
                                                                float *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int head = blockIdx.y;
    const long long nw = (long long)gridDim.x * 4;
    const float *xh = x + (long long)head * x_hs;
    const long long *ih = idx + (long long)head * idx_hs;
    float *ch = counts + (long long)head * K;
    float *sh = sums + (long long)head * K * D;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < M; row += nw) {
        if (mask && !mask[(long long)head * M + row]) continue;  // wave-uniform
        const long long k = ih[row * idx_rs];
        if (k < 0 || k >= K) continue;
        const float *xr = xh + row * x_rs;
        float *dst = sh + k * D;
        for (int d = lane; d < D; d += 64) atomicAdd(dst + d, xr[d]);
        if (lane == 0) atomicAdd(ch + k, 1.0f);
    }
}

// Residual stack (SURVEY 8f rank 1 for ResidualVQ): stage q's EMA statistics are those of the RESIDUAL r_q that stage
// quantized (residual_vq.py:212-233 feeds `residual` into every layer's Codebook.forward).  One pass per row: rebuild
// the chain from the indices of the fused launch and scatter-add each r_q into stage q's sums.
//   counts [H][Q][K], sums [H][Q][K][D];  r_0 = x,  r_{q+1} = r_q - (ste ? r_q + (c_q - r_q) : c_q)
__global__ void __launch_bounds__(256) vq_ema_accumulate_residual_kernel(const float *__restrict__ x, long long x_rs, long long x_hs,
                                                                         const float *__restrict__ cb, long long cb_hs,
                                                                         long long cb_qs, const long long *__restrict__ idx,
                                                                         long long idx_rs, long long idx_hs, long long idx_qs,
                                                                         long long M, int K, int D, int Q, int ste,
                                                                         float *__restrict__ counts, float *__restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.y;
    const long long nw = (long long)gridDim.x * 4;
    const float *xh = x + (long long)head * x_hs;
    const float *cbh = cb + (long long)head * cb_hs;
    const long long *ih = idx + (long long)head * idx_hs;
    float *ch = counts + (long long)head * Q * K;
    float *sh = sums + (long long)head * Q * K * D;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < M; row += nw) {
        const float *xr = xh + row * x_rs;
        for (int d0 = 0; d0 < D; d0 += 64 * 4) {  // 4 floats per lane and pass
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int d = d0 + e * 64 + lane;
                r[e] = (d < D) ? xr[d] : 0.0f;
            }
            for (int q = 0; q < Q; ++q) {
                const long long k = ih[row * idx_rs + q * idx_qs];
                if (k < 0 || k >= K) break;  // dropped stage (quantize dropout): the chain ends here
                const float *crow = cbh + (long long)q * cb_qs + k * D;
                float *dst = sh + ((long long)q * K + k) * D;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int d = d0 + e * 64 + lane;
                    if (d < D) {
                        atomicAdd(dst + d, r[e]);
                        const float c = crow[d];
                        const float quant = ste ? r[e] + (c - r[e]) : c;
                        r[e] = r[e] - quant;
                    }
                }
                if (d0 == 0 && lane == 0) atomicAdd(ch + (long long)q * K + k, 1.0f);
            }
        }
    }
}

// Owner-computes variant for codebooks with many rows per code: every WAVE owns `cw` consecutive codes (their [cw][D]
// partial sums live in a wave-private LDS region, plain read-add-write: nobody else touches them) and a contiguous range
// of rows.  It scans the indices of its rows 64 at a time, keeps the rows assigned to its codes (ballot + rank -> a
// small queue) and adds them -- whole rows, `UN` row loads in flight -- then flushes its non-zero partial sums once.
// Each x row is read exactly once, as a full row; global float atomics drop from M*D to (row blocks)*K*D.
// (LDS float atomics were tried for a workgroup-shared table and are far slower than this on gfx950.)
__global__ void __launch_bounds__(256) vq_ema_accumulate_owner_kernel(const float *__restrict__ x, long long x_rs, long long x_hs,
                                                                      const long long *__restrict__ idx, long long idx_rs,
                                                                      long long idx_hs, const unsigned char *__restrict__ mask,
                                                                      long long M, long long rows_per_block, int K, int cw, int D,
                                                                      float *__restrict__ counts, float *__restrict__ sums,
                                                                      float *__restrict__ part_sums, float *__restrict__ part_counts) {
    extern __shared__ __attribute__((aligned(16))) float lds_own[];  // per wave: [cw][D4] sums | [cw] counts | [64] rows | [64] codes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.z;
    const int D4 = (D + 3) & ~3;
    const int per_wave = cw * D4 + ((cw + 3) & ~3) + 64 * 2 + 64;  // floats
    float *tab = lds_own + (long long)wave * per_wave;
    float *cnt = tab + cw * D4;
    long long *qrow = (long long *)(cnt + ((cw + 3) & ~3));
    int *qk = (int *)(qrow + 64);
    const int k0 = (blockIdx.x * 4 + wave) * cw;
    if (k0 >= K) return;  // no workgroup barriers below: waves are independent
    for (int i = lane; i < cw * D4 + ((cw + 3) & ~3); i += 64) tab[i] = 0.0f;

    const float *xh = x + (long long)head * x_hs;
    const long long *ih = idx + (long long)head * idx_hs;
    const long long r_begin = (long long)blockIdx.y * rows_per_block;
    const long long r_end = (r_begin + rows_per_block < M) ? r_begin + rows_per_block : M;
    const bool vec = (D % 4 == 0) && (x_rs % 4 == 0) && (x_hs % 4 == 0) && (((uintptr_t)x & 15) == 0);
    constexpr int UN = 8;  // row loads in flight
    for (long long base = r_begin; base < r_end; base += 64) {
        const long long row = base + lane;
        long long k = -1;
        if (row < r_end && !(mask && !mask[(long long)head * M + row])) k = ih[row * idx_rs];
        const bool mine = k >= k0 && k < k0 + cw && k < K;
        const unsigned long long ball = __ballot(mine);
        const int count = __popcll(ball);
        if (mine) {
            const int rank = __popcll(ball & ((1ull << lane) - 1ull));
            qrow[rank] = row;
            qk[rank] = (int)(k - k0);
        }
        // wave-private LDS: the operations of one wave execute in order, no barrier needed
        for (int j0 = 0; j0 < count; j0 += UN) {
            for (int dc = 0; dc < D; dc += 256) {
                const int d = dc + 4 * lane;
                f32x4 v[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    v[u] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                    if (j0 + u < count && d < D) {
                        const float *src = xh + qrow[j0 + u] * x_rs + d;
                        if (vec) {
                            v[u] = __builtin_nontemporal_load((const f32x4 *)src);
                        } else {
                            v[u].x = src[0];
                            if (d + 1 < D) v[u].y = src[1];
                            if (d + 2 < D) v[u].z = src[2];
                            if (d + 3 < D) v[u].w = src[3];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < UN; ++u) {
                    if (j0 + u < count) {  // wave-uniform
                        const int kk = qk[j0 + u];
                        if (d < D) {
                            f32x4 *t = (f32x4 *)(tab + kk * D4 + d);
                            *t = *t + v[u];
                        }
                        if (dc == 0 && lane == 0) cnt[kk] += 1.0f;
                    }
                }
            }
        }
    }
    const int kvalid = (k0 + cw <= K) ? cw : K - k0;
    if (part_sums) {
        // reproducible variant: every (row block, owner) stores its partial sums -- zeros included -- to its own slots;
        // vq_ema_reduce_parts_kernel adds the row blocks in a fixed order (no float atomics anywhere)
        const long long slot = (long long)blockIdx.y * gridDim.z + head;
        float *ps = part_sums + (slot * K + k0) * D;
        for (int c = 0; c < kvalid; ++c)
            for (int d = lane; d < D; d += 64) ps[(long long)c * D + d] = tab[c * D4 + d];
        if (lane < kvalid) part_counts[slot * K + k0 + lane] = cnt[lane];
        return;
    }
    float *sh = sums + (long long)head * K * D;
    for (int c = 0; c < kvalid; ++c) {
        for (int d = lane; d < D; d += 64) {
            const float val = tab[c * D4 + d];
            if (val != 0.0f) atomicAdd(sh + (long long)(k0 + c) * D + d, val);
        }
    }
    if (lane < kvalid && cnt[lane] != 0.0f) atomicAdd(counts + (long long)head * K + k0 + lane, cnt[lane]);
}

// dst[i] += part[0][i] + part[1][i] + ... (left to right): the fixed-order second half of the reproducible accumulation
__global__ void __launch_bounds__(256) vq_ema_reduce_parts_kernel(const float *__restrict__ part, int nparts, long long n,
                                                                  float *__restrict__ dst) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = dst[i];
    for (int b = 0; b < nparts; ++b) s += part[(long long)b * n + i];
    dst[i] = s;
}

// cluster_size <- lerp(cluster_size, counts, 1 - decay);  total[h] = sum_k cluster_size      (codebooks.py:411,419-421)
__global__ void __launch_bounds__(256) vq_ema_sizes_kernel(float *__restrict__ cluster_size, const float *__restrict__ counts,
                                                           int K, float weight, float *__restrict__ total) {
    __shared__ float sh[256];
    const int head = blockIdx.x;
    float s = 0.0f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float old = cluster_size[(long long)head * K + k];
        const float nw = old + weight * (counts[(long long)head * K + k] - old);
        cluster_size[(long long)head * K + k] = nw;
        s += nw;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[head] = sh[0];
}

// embed_avg <- lerp(embed_avg, sums, 1 - decay); embeddings <- [l2norm](embed_avg / laplace-smoothed size)
// one wave per code row                                                             (codebooks.py:417-425)
__global__ void __launch_bounds__(256) vq_ema_codes_kernel(const float *__restrict__ cluster_size, const float *__restrict__ total,
                                                           float *__restrict__ embed_avg, const float *__restrict__ sums,
                                                           float *__restrict__ embeddings, int H, int K, int D, float weight,
                                                           float eps, int l2norm) {
    const int lane = threadIdx.x & 63;
    const long long rowid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rowid >= (long long)H * K) return;
    const int head = (int)(rowid / K);
    const float tot = total[head];
    const float cs = cluster_size[rowid];
    const float smoothed = (cs + eps) / (tot + (float)K * eps) * tot;
    float *avg = embed_avg + rowid * D;
    const float *sm = sums + rowid * D;
    float *emb = embeddings + rowid * D;
    float nrm = 0.0f;
    for (int d = lane; d < D; d += 64) {
        const float old = avg[d];
        const float a = old + weight * (sm[d] - old);
        avg[d] = a;
        const float e = a / smoothed;
        emb[d] = e;
        nrm = fmaf(e, e, nrm);
    }
    if (l2norm) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nrm += __shfl_xor(nrm, o);
        const float n = sqrtf(nrm);
        const float inv = 1.0f / (n < 1e-12f ? 1e-12f : n);  // clamp_min keeps a NaN norm (fmaxf would drop it): the row is NaN
        for (int d = lane; d < D; d += 64) emb[d] = emb[d] * inv;  // same lane wrote it
    }
}

