// vq_residual_mask.inc -- the mask pass of a residual stack (vq_residual_mask_f32, vq_residual_mask_backward_f32): what
// ResidualVQ / GroupedResidualVQ do with `mask=` (residual_vq.py:212-243 over vector_quantize_pytorch.py:347-364,413-418), applied
// to the indices the fused search wrote for ALL rows.  Per row, with r_0 = x and acc = +0.0, for q = 0 .. Q-1:
//
//   kept row (mask != 0):   c = cb[g][q][idx_q];  e_q += sum_d (c - r_q)^2;  quant = train ? r_q + (c - r_q) : c
//   masked-out row:         quant = r_q           (where(mask, quantize, orig_input), vector_quantize_pytorch.py:415-418)
//   both:                   acc = acc + quant;  r_{q+1} = r_q - quant;       out = acc after the last stage
//
// A finite masked-out row therefore has r_q = 0 for q >= 1 and out = x; the reference searches that zero row, so its index
// of stage q >= 1 is the stage's answer to the all-zero row (zero_idx, from the real search kernel).  A masked-out row with a
// non-finite element has NaN in r_1 and answers code 0 (the ATen rule for a row holding a NaN).  Stage 0 of every row and
// every stage of a kept row are the search's own results and are only read.
//
// Lane mapping (both kernels): one float4 per lane and 256-dim slice, LPR = the power of two >= ceil(D / 4) (at most 64)
// lanes per row, 64 / LPR rows per 64-lane access, rows wider than 256 dims hold two slices per lane.  A wave owns a UNIT of
// NI accesses and gathers QB stages of them at a time (the indices of all stages are known up front, so the gathers do not
// wait for the chain).  VEC: 16-byte accesses (D % 4 == 0, aligned pointers and strides); otherwise the same mapping with
// four guarded scalar accesses per lane.  Elements past D read as +0.0 and are never written.
// Squared errors: every unit stores ONE float per stage (fixed shuffle tree over the wave), vq_loss_reduce_kernel adds the
// units in a fixed order in fp64.  No atomics.

struct ResMaskParams {
    const float *x; long long x_gs, x_rs;
    const float *cb; long long cb_gs, cb_qs;
    long long *idx; long long idx_gs, idx_rs, idx_qs;
    const unsigned char *mask; long long mask_gs;
    const long long *zero_idx;                       // [G][Q] (forward)
    long long M;
    int Q, K, D, train;
    float *out; long long out_gs, out_rs;            // forward: out; backward: grad_x
    float *part;                                     // forward: [G][units][Q] squared-error partials, or NULL
    const float *go; long long go_gs, go_rs;         // backward: grad of out, or NULL
    const double *g_err; long long g_err_gs;         // backward: grad of sq_err [Q] (g_err_gs = 0) or [G][Q], or NULL
    int lpr_log2;
    long long units;                                 // per group
};

constexpr int kRmNI = 2;  // accesses in flight per lane
constexpr int kRmQB = 4;  // stages gathered together

template <bool VEC>
__device__ __forceinline__ f32x4 rm_load(const float *row, int d, int D) {
    f32x4 v = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC) {
        const f32x4 t = *(const f32x4 *)(row + (d < D ? d : 0));  // unconditional: a lane past D reads the row's start, unused
        if (d < D) v = t;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d + j < D) v[j] = row[d + j];
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void rm_store(float *row, int d, int D, f32x4 v) {
    if (VEC) {
        if (d < D) __builtin_nontemporal_store(v, (f32x4 *)(row + d));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d + j < D) row[d + j] = v[j];
    }
}

__device__ __forceinline__ bool rm_nonfinite(f32x4 v) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= (__float_as_uint(v[j]) & 0x7f800000u) == 0x7f800000u;
    return bad;
}

// the validated code of a stage: an index outside [0, K) never becomes an address (code 0 is read instead)
__device__ __forceinline__ long long rm_code(long long v, int K) { return (v >= 0 && v < K) ? v : 0; }

template <bool VEC, int NS>
__global__ void __launch_bounds__(256) vq_residual_mask_kernel(const ResMaskParams p) {
    const int lane = threadIdx.x & 63;
    const long long g = blockIdx.y;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const int lpr = 1 << p.lpr_log2, rpi = 64 >> p.lpr_log2;
    const int sub = lane >> p.lpr_log2, ll = lane & (lpr - 1);
    const int d0 = 4 * ll;
    const unsigned long long group = (lpr == 64 ? ~0ull : ((1ull << lpr) - 1ull)) << (sub * lpr);  // the lanes of this lane's row
    const float *xg = p.x + g * p.x_gs;
    const float *cbg = p.cb + g * p.cb_gs;
    long long *ig = p.idx + g * p.idx_gs;
    const unsigned char *mg = p.mask + g * p.mask_gs;
    const long long *zi = p.zero_idx + g * p.Q;
    float *og = p.out + g * p.out_gs;
    const bool train = p.train != 0;
    const f32x4 zero = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (long long u = wave; u < p.units; u += nwaves) {
        long long n[kRmNI];
        bool live[kRmNI], kept[kRmNI], finite[kRmNI];
        f32x4 r[kRmNI][NS], acc[kRmNI][NS];
#pragma unroll
        for (int k = 0; k < kRmNI; ++k) {
            const long long row = (u * kRmNI + k) * rpi + sub;
            live[k] = row < p.M;
            n[k] = live[k] ? row : p.M - 1;  // clamp: duplicates are computed, not stored
            kept[k] = mg[n[k]] != 0;
            bool bad = false;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                r[k][s] = rm_load<VEC>(xg + n[k] * p.x_rs, d0 + 256 * s, p.D);
                acc[k][s] = zero;
                bad |= rm_nonfinite(r[k][s]);
            }
            finite[k] = (__ballot(bad) & group) == 0ull;
        }
        for (int q0 = 0; q0 < p.Q; q0 += kRmQB) {
            long long code[kRmQB][kRmNI];
            f32x4 c[kRmQB][kRmNI][NS];
#pragma unroll
            for (int kq = 0; kq < kRmQB; ++kq) {
                const int q = q0 + kq < p.Q ? q0 + kq : p.Q - 1;  // clamp: stages past the end read a real index, unused
#pragma unroll
                for (int k = 0; k < kRmNI; ++k) code[kq][k] = rm_code(ig[n[k] * p.idx_rs + q * p.idx_qs], p.K);
            }
#pragma unroll
            for (int kq = 0; kq < kRmQB; ++kq) {
                const int q = q0 + kq < p.Q ? q0 + kq : p.Q - 1;
#pragma unroll
                for (int k = 0; k < kRmNI; ++k)
#pragma unroll
                    for (int s = 0; s < NS; ++s)
                        c[kq][k][s] = rm_load<VEC>(cbg + (long long)q * p.cb_qs + code[kq][k] * p.D, d0 + 256 * s, p.D);
            }
#pragma unroll
            for (int kq = 0; kq < kRmQB; ++kq) {
                const int q = q0 + kq;
                if (q < p.Q) {  // wave-uniform
                    float e = 0.0f;
#pragma unroll
                    for (int k = 0; k < kRmNI; ++k) {
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const f32x4 rr = r[k][s];
                            const f32x4 diff = c[kq][k][s] - rr;
                            const f32x4 hit = train ? rr + diff : c[kq][k][s];
                            const f32x4 quant = kept[k] ? hit : rr;
                            if (kept[k] && live[k]) e += ((diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]) + diff[3] * diff[3];
                            acc[k][s] = acc[k][s] + quant;
                            r[k][s] = rr - quant;
                        }
                        if (q >= 1 && live[k] && !kept[k] && ll == 0) ig[n[k] * p.idx_rs + q * p.idx_qs] = finite[k] ? zi[q] : 0ll;
                    }
                    if (p.part) {
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
                        if (lane == 0) p.part[(g * p.units + u) * p.Q + q] = e;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kRmNI; ++k)
            if (live[k]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) rm_store<VEC>(og + n[k] * p.out_rs, d0 + 256 * s, p.D, acc[k][s]);
            }
    }
}

// grad_x = (train ? Q * grad_out : 0) + (kept ? sum_q 2 * grad_sq_err[q] * (r_q - c_q) : 0), the chain of a kept row rebuilt
// in the forward's fp32 order (the arithmetic of vq_quantize_backward_kernel); a masked-out row gathers nothing.
template <bool VEC, int NS>
__global__ void __launch_bounds__(256) vq_residual_mask_backward_kernel(const ResMaskParams p) {
    const int lane = threadIdx.x & 63;
    const long long g = blockIdx.y;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const int lpr = 1 << p.lpr_log2, rpi = 64 >> p.lpr_log2;
    const int sub = lane >> p.lpr_log2, ll = lane & (lpr - 1);
    const int d0 = 4 * ll;
    const float *xg = p.x + g * p.x_gs;
    const float *cbg = p.cb + g * p.cb_gs;
    const long long *ig = p.idx + g * p.idx_gs;
    const unsigned char *mg = p.mask + g * p.mask_gs;
    const float *gog = (p.train && p.go) ? p.go + g * p.go_gs : nullptr;
    const double *ge = p.g_err ? p.g_err + g * p.g_err_gs : nullptr;
    float *og = p.out + g * p.out_gs;
    const bool train = p.train != 0;
    const float qf = (float)p.Q;
    const f32x4 zero = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (long long u = wave; u < p.units; u += nwaves) {
        long long n[kRmNI];
        bool live[kRmNI], kept[kRmNI];
        f32x4 r[kRmNI][NS], gx[kRmNI][NS];
#pragma unroll
        for (int k = 0; k < kRmNI; ++k) {
            const long long row = (u * kRmNI + k) * rpi + sub;
            live[k] = row < p.M;
            n[k] = live[k] ? row : p.M - 1;
            kept[k] = mg[n[k]] != 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                r[k][s] = rm_load<VEC>(xg + n[k] * p.x_rs, d0 + 256 * s, p.D);
                gx[k][s] = gog ? rm_load<VEC>(gog + n[k] * p.go_rs, d0 + 256 * s, p.D) * qf : zero;
            }
        }
        if (ge) {
            for (int q0 = 0; q0 < p.Q; q0 += kRmQB) {
                long long code[kRmQB][kRmNI];
                f32x4 c[kRmQB][kRmNI][NS];
#pragma unroll
                for (int kq = 0; kq < kRmQB; ++kq) {
                    const int q = q0 + kq < p.Q ? q0 + kq : p.Q - 1;
#pragma unroll
                    for (int k = 0; k < kRmNI; ++k) code[kq][k] = rm_code(ig[n[k] * p.idx_rs + q * p.idx_qs], p.K);
                }
#pragma unroll
                for (int kq = 0; kq < kRmQB; ++kq) {
                    const int q = q0 + kq < p.Q ? q0 + kq : p.Q - 1;
#pragma unroll
                    for (int k = 0; k < kRmNI; ++k)
#pragma unroll
                        for (int s = 0; s < NS; ++s)
                            c[kq][k][s] = rm_load<VEC>(cbg + (long long)q * p.cb_qs + code[kq][k] * p.D, d0 + 256 * s, p.D);
                }
#pragma unroll
                for (int kq = 0; kq < kRmQB; ++kq) {
                    const int q = q0 + kq;
                    if (q < p.Q) {
                        const float coef = (float)(2.0 * ge[q]);
#pragma unroll
                        for (int k = 0; k < kRmNI; ++k)
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const f32x4 rr = r[k][s], cc = c[kq][k][s];
                                if (kept[k]) gx[k][s] = gx[k][s] + (rr - cc) * coef;
                                const f32x4 quant = train ? rr + (cc - rr) : cc;
                                r[k][s] = rr - quant;
                            }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kRmNI; ++k)
            if (live[k]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) rm_store<VEC>(og + n[k] * p.out_rs, d0 + 256 * s, p.D, gx[k][s]);
            }
    }
}

// lanes per row and units per group of a call (rows of one unit: kRmNI * 64 / LPR)
void rm_plan(ResMaskParams &p) {
    const int d4 = (p.D + 3) / 4;
    p.lpr_log2 = 0;
    while ((1 << p.lpr_log2) < d4 && p.lpr_log2 < 6) ++p.lpr_log2;
    const long long rows_per_unit = (long long)kRmNI * (64 >> p.lpr_log2);
    p.units = (p.M + rows_per_unit - 1) / rows_per_unit;
}

inline bool rm_aligned(const void *q, std::initializer_list<long long> strides) {
    for (const long long st : strides)
        if (st % 4) return false;
    return ((uintptr_t)q & 15) == 0;
}

template <template <bool, int> class Launcher>
int rm_dispatch(const ResMaskParams &p, bool vec, int G, int cus, hipStream_t s, const char *what) {
    long long blocks = (p.units + 3) / 4;
    const long long max_blocks = 8ll * (cus > 0 ? cus : 256);
    if (blocks > max_blocks) blocks = max_blocks;
    const dim3 grid((unsigned)blocks, (unsigned)G);
    if (p.D <= 256) return vec ? Launcher<true, 1>::run(grid, s, what, p) : Launcher<false, 1>::run(grid, s, what, p);
    return vec ? Launcher<true, 2>::run(grid, s, what, p) : Launcher<false, 2>::run(grid, s, what, p);
}

template <bool VEC, int NS>
struct RmForward {
    static int run(dim3 grid, hipStream_t s, const char *what, const ResMaskParams &p) {
        return launch<vq_residual_mask_kernel<VEC, NS>>(grid, dim3(256), 0, s, what, p);
    }
};

template <bool VEC, int NS>
struct RmBackward {
    static int run(dim3 grid, hipStream_t s, const char *what, const ResMaskParams &p) {
        return launch<vq_residual_mask_backward_kernel<VEC, NS>>(grid, dim3(256), 0, s, what, p);
    }
};
