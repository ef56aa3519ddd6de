// vq_fsq.inc -- finite scalar quantization (FSQ / ResidualFSQ / GroupedResidualFSQ, finite_scalar_quantization.py and
// residual_fsq.py of the reference): every stage of every group in one pass, one thread per (group, row) sub-row of
// d <= 16 values held in registers across all S stages.  Plain FSQ is S = 1 without the extra bound.
// Included by vq_kernels.hip inside its anonymous namespace, build part 0.
//
// Constants.  The per-dim integers (levels L, basis = cumprod of the levels before) are passed by value and indexed only
// at compile-time dims (the kernels are instantiated per d, so the loops unroll).  The float constants are a device array
// k [3 + S][d]: half_l, offset, shift (computed in torch by the module with the reference's own expressions, so tanhf is
// the only transcendental here), then the stage scales, read at the loop-uniform stage index with scalar loads.
//
// Stage s of a row (finite_scalar_quantization.py:147-177, residual_fsq.py:137-189), r starting at x (plain FSQ) or at
// bound(x) (ResidualFSQ bounds once before its loop, so stage 0 quantizes bound(bound(x))):
//   z = r / scale[s];  b = tanh(z + shift) * half_l - offset;  c = rint(b) / hw          (hw = L / 2; round_ste is exact)
//   o = c * scale[s];  r = r - o;  out = out + o                                         (out starts at +0, stage order)
//   idx = (int32) sum_i ((c_i * hw_i) + hw_i) * basis_i  in fp32, summed as torch's CPU sum over d <= 7 does: partial k
//   starts at term k (k < 4), terms 4 .. d-1 go into partial 0, then p0 += p1, p0 += p2, p0 += p3.  The cast truncates;
//   NaN gives INT32_MIN (what the reference's CPU cast produces).  -ffp-contract=off keeps every step a single IEEE op.
//
//   fsq_quantize_kernel   grid (row blocks, G): out [g * out_gs + m * out_rs + i], idx [G][N][S] int32 (may be NULL)
//   fsq_backward_kernel   grid (row blocks, G): recomputes the chain from x with the same code (the same r_s), and
//                         grad_x = [bound'(x)] * sum_s bound'(r_s / scale_s) / hw * g_out (the residual's detach makes
//                         d r_s / d r_0 the identity), 1 - tanh^2 taken from exp(-2|u|) so it does not cancel where
//                         tanh saturates; per row, no atomics, so bitwise reproducible
//   fsq_decode_kernel     indices [N][Q] (int32 or int64; -1 = dropped stage when drop_null) -> the codes
//                         ((i // basis) % L - hw) / hw * scale[q] (one correctly rounded division of exact integers, as
//                         implicit_codebook is built), their sum over q in stage order and / or all_codes [Q][N][d]

constexpr int kFsqMaxDim = 16;
constexpr int kFsqThreads = 256;

struct FsqLevels {
    int L[kFsqMaxDim];
    int basis[kFsqMaxDim];
};

__host__ __device__ inline int64_t fsq_blocks(int64_t N) { return (N + kFsqThreads - 1) / kFsqThreads; }

// bound(z) of the reference: tanh(z + shift) * half_l - offset
template <int D>
__device__ __forceinline__ float fsq_bound(float z, const float *__restrict__ k, int i, float &th) {
    th = tanhf(z + k[2 * D + i]);
    return th * k[i] - k[D + i];
}

// bound'(z) / half_l = 1 - tanh^2(u), u = z + shift, as 4 e / (1 + e)^2 with e = exp(-2 |u|): no cancellation where tanh
// saturates (the fp32 1 - th * th of autograd loses every digit there)
__device__ __forceinline__ float fsq_sech2(float u) {
    const float e = expf(-2.0f * fabsf(u));
    const float p = 1.0f + e;
    return 4.0f * e / (p * p);
}

// torch's CPU sum over a row of D <= 7 fp32 values (see the header), then .to(int32)
template <int D>
__device__ __forceinline__ int32_t fsq_index(const float (&t)[D]) {
    float s = t[0];
#pragma unroll
    for (int i = 4; i < D; ++i) s = s + t[i];
#pragma unroll
    for (int i = 1; i < (D < 4 ? D : 4); ++i) s = s + t[i];
    return (s >= -2147483648.0f && s < 2147483648.0f) ? (int32_t)s : INT32_MIN;
}

template <int D>
__global__ void __launch_bounds__(kFsqThreads) fsq_quantize_kernel(
    const float *__restrict__ x, int64_t x_gs, int64_t x_rs, int64_t N, int S, FsqLevels lv, const float *__restrict__ k,
    bool prebound, float *__restrict__ out, int64_t out_gs, int64_t out_rs, int32_t *__restrict__ idx) {
    const int64_t g = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * kFsqThreads + threadIdx.x;
    if (m >= N) return;
    float r[D], acc[D], t[D], th;
    const float *xr = x + g * x_gs + m * x_rs;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        r[i] = xr[i];
        acc[i] = 0.0f;
    }
    if (prebound) {
#pragma unroll
        for (int i = 0; i < D; ++i) r[i] = fsq_bound<D>(r[i], k, i, th);
    }
    int32_t *ir = idx ? idx + (g * N + m) * S : nullptr;
    for (int s = 0; s < S; ++s) {
        const float *sc = k + (3 + s) * D;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float hw = (float)(lv.L[i] / 2);
            const float c = rintf(fsq_bound<D>(r[i] / sc[i], k, i, th)) / hw;
            const float o = c * sc[i];
            r[i] = r[i] - o;
            acc[i] = acc[i] + o;
            t[i] = ((c * hw) + hw) * (float)lv.basis[i];
        }
        if (ir) ir[s] = fsq_index<D>(t);
    }
    float *orow = out + g * out_gs + m * out_rs;
#pragma unroll
    for (int i = 0; i < D; ++i) orow[i] = acc[i];
}

template <int D>
__global__ void __launch_bounds__(kFsqThreads) fsq_backward_kernel(
    const float *__restrict__ x, int64_t x_gs, int64_t x_rs, int64_t N, int S, FsqLevels lv, const float *__restrict__ k,
    bool prebound, const float *__restrict__ g_out, int64_t g_gs, int64_t g_rs, float *__restrict__ gx, int64_t gx_gs,
    int64_t gx_rs) {
    const int64_t g = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * kFsqThreads + threadIdx.x;
    if (m >= N) return;
    float r[D], go[D], dx[D], d0[D], th;
    const float *xr = x + g * x_gs + m * x_rs;
    const float *gr = g_out + g * g_gs + m * g_rs;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        r[i] = xr[i];
        go[i] = gr[i];
        dx[i] = 0.0f;
        d0[i] = 1.0f;
    }
    if (prebound) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
            d0[i] = k[i] * fsq_sech2(r[i] + k[2 * D + i]);
            r[i] = fsq_bound<D>(r[i], k, i, th);
        }
    }
    for (int s = 0; s < S; ++s) {
        const float *sc = k + (3 + s) * D;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float hw = (float)(lv.L[i] / 2);
            const float z = r[i] / sc[i];
            const float c = rintf(fsq_bound<D>(z, k, i, th)) / hw;
            r[i] = r[i] - c * sc[i];
            // autograd's order: * scale (out), / hw (quantize), * half_l * bound'/half_l (bound), / scale (residual / scale)
            dx[i] += go[i] * sc[i] / hw * k[i] * fsq_sech2(z + k[2 * D + i]) / sc[i];
        }
    }
    float *dr = gx + g * gx_gs + m * gx_rs;
#pragma unroll
    for (int i = 0; i < D; ++i) dr[i] = dx[i] * d0[i];
}

// floor division and Python's modulo, as torch's // and % on integer tensors
__device__ __forceinline__ int64_t fsq_level_index(int64_t v, int basis, int L) {
    if (v >= 0 && v <= 0x7fffffff) return (int64_t)(((uint32_t)v / (uint32_t)basis) % (uint32_t)L);
    int64_t q = v / basis;
    if (q * basis != v && v < 0) q -= 1;
    int64_t r = q % L;
    return r < 0 ? r + L : r;
}

template <int D>
__global__ void __launch_bounds__(kFsqThreads) fsq_decode_kernel(const void *__restrict__ idx, bool idx64, int64_t N, int Q,
                                                                 FsqLevels lv, const float *__restrict__ scales, bool drop_null,
                                                                 float *__restrict__ sum, float *__restrict__ all) {
    const int64_t m = (int64_t)blockIdx.x * kFsqThreads + threadIdx.x;
    if (m >= N) return;
    float acc[D];
#pragma unroll
    for (int i = 0; i < D; ++i) acc[i] = 0.0f;
    for (int q = 0; q < Q; ++q) {
        const int64_t v = idx64 ? ((const int64_t *)idx)[m * Q + q] : (int64_t)((const int32_t *)idx)[m * Q + q];
        const bool dropped = drop_null && v == -1;
        const float *sc = scales + q * D;
        float *ar = all ? all + ((int64_t)q * N + m) * D : nullptr;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int hw = lv.L[i] / 2;
            const int64_t li = fsq_level_index(v, lv.basis[i], lv.L[i]);
            const float c = dropped ? 0.0f : ((float)(li - hw) / (float)hw) * sc[i];
            acc[i] = acc[i] + c;
            if (ar) ar[i] = c;
        }
    }
    if (sum) {
        float *sr = sum + m * D;
#pragma unroll
        for (int i = 0; i < D; ++i) sr[i] = acc[i];
    }
}

// checks shared by the three entry points; fills lv (basis = cumprod of the levels before, as the reference's _basis)
int fsq_check(int64_t G, int64_t N, int d, int S, const int32_t *levels, const float *consts, FsqLevels &lv, const char *who) {
    char msg[160];
    if (G < 1 || G > 65535 || N < 1 || S < 1) {
        snprintf(msg, sizeof msg, "%s: sizes must be positive (G <= 65535)", who);
        return fail(VQ_E_BADARG, msg);
    }
    if (d < 1 || d > kFsqMaxDim) {
        snprintf(msg, sizeof msg, "%s: d must be in [1, 16]", who);
        return fail(VQ_E_BADARG, msg);
    }
    if (!levels || !consts) {
        snprintf(msg, sizeof msg, "%s: null pointer", who);
        return fail(VQ_E_BADARG, msg);
    }
    int64_t basis = 1;
    for (int i = 0; i < kFsqMaxDim; ++i) {
        lv.L[i] = 2;
        lv.basis[i] = 1;
    }
    for (int i = 0; i < d; ++i) {
        if (levels[i] < 2) {
            snprintf(msg, sizeof msg, "%s: every level must be >= 2", who);
            return fail(VQ_E_BADARG, msg);
        }
        if (basis > 0x7fffffff) {
            snprintf(msg, sizeof msg, "%s: the codebook size overflows int32", who);
            return fail(VQ_E_BADARG, msg);
        }
        lv.L[i] = levels[i];
        lv.basis[i] = (int)basis;
        basis *= levels[i];
    }
    if (fsq_blocks(N) > 0x7fffffff) {
        snprintf(msg, sizeof msg, "%s: too many rows", who);
        return fail(VQ_E_BADARG, msg);
    }
    return 0;
}

// d -> the kernel instantiated for it
#define FSQ_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

#define FSQ_LAUNCHER(name, kernel)                                                                   \
    template <typename... A>                                                                         \
    int name(int d, dim3 grid, hipStream_t s, const char *what, A... args) {                         \
        switch (d) {                                                                                 \
            FSQ_CASES(FSQ_CASE_##kernel)                                                             \
        }                                                                                            \
        return 0;                                                                                    \
    }
#define FSQ_CASE_fsq_quantize_kernel(D) \
    case D: return launch<fsq_quantize_kernel<D>>(grid, dim3(kFsqThreads), 0, s, what, args...);
#define FSQ_CASE_fsq_backward_kernel(D) \
    case D: return launch<fsq_backward_kernel<D>>(grid, dim3(kFsqThreads), 0, s, what, args...);
#define FSQ_CASE_fsq_decode_kernel(D) \
    case D: return launch<fsq_decode_kernel<D>>(grid, dim3(kFsqThreads), 0, s, what, args...);
FSQ_LAUNCHER(fsq_launch_quantize, fsq_quantize_kernel)
FSQ_LAUNCHER(fsq_launch_backward, fsq_backward_kernel)
FSQ_LAUNCHER(fsq_launch_decode, fsq_decode_kernel)
#undef FSQ_LAUNCHER
#undef FSQ_CASE_fsq_quantize_kernel
#undef FSQ_CASE_fsq_backward_kernel
#undef FSQ_CASE_fsq_decode_kernel
