// vq_rlfq.inc -- residual LFQ (ResidualLFQ / GroupedResidualLFQ, residual_lfq.py of the reference): every stage's
// quantize step in one pass, one thread per row, the row's d <= 20 values held in registers across all S stages.
// Included by vq_kernels.hip inside its anonymous namespace, build part 0, after vq_lfq.inc (it reuses lfq_sum_kernel).
//
// The per-stage constants are a device array k [3][S] (qmag, clamp, scale), read at the loop-uniform stage index with
// scalar loads.  (A by-value struct of arrays indexed by the runtime stage is copied into registers: it cost the backward
// kernel its SGPR headroom, and the same pattern doubled lfq_entropy_fwd_kernel's VGPRs.)
//
// Stage s of a row (the reference's LFQ.forward on the residual, lookup_free_quantization.py:240-283 and :323-336):
//   u = clamp[s] > 0 ? tanh(r / clamp[s]) * clamp[s] : r          (soft clamp)
//   v = spherical ? u / max(|u|, 1e-12) * scale[s] : u             (l2norm times the stage's codebook scale)
//   q_i = v_i > 0 ? qmag[s] : -qmag[s];  idx = sum_i (v_i > 0) << (d - 1 - i)   (MSB first)
//   o = ste ? v + (q - v) : q                                      (the straight-through value; eval: q itself)
//   commitment: sum over the kept rows of (v - q)^2 in fp64
//   r = r - o;  out = out + o                                      (residual_lfq.py:176-177, stage order)
// With no clamp and no l2norm this is the same IEEE sequence as the stage-by-stage loop (-ffp-contract=off), so out, idx
// and the commitment sums are bitwise equal to it.  The commitment partials split the rows exactly as
// lfq_quantize_kernel does (256 rows per block, a tree per block, lfq_sum_kernel over the blocks), per (group, stage).
//
// Both kernels are instantiated per d (1 .. 20): the row loops unroll to exactly d lanes of work.
//   rlfq_quantize_kernel   grid (row blocks, G): idx [G][N][S], out, the stage inputs v_all [G][S][N][d], fp64 partials
//   rlfq_backward_kernel   grid (row blocks, G): recomputes the chain from x (the same code, so the same v, q, o) and
//                          sums J_s^T (g_out + (v - q) w_commit[s] mask + g_ent[s]) over the stages: the residual's detach
//                          makes d r_s / d x the identity; J_s is the clamp (1 - tanh^2) and l2norm Jacobian.

constexpr int kRlfqThreads = kLfqQuantThreads;

__host__ __device__ inline int64_t rlfq_blocks(int64_t N) { return (N + kRlfqThreads - 1) / kRlfqThreads; }

inline int64_t rlfq_ws_bytes(int64_t G, int64_t N, int S) { return lfq_align(G * S * (rlfq_blocks(N) > 0 ? rlfq_blocks(N) : 1) * 8); }

// stage input of a row: u (post clamp), th (tanh values when clamping), v; returns the norm's denominator (1 if not spherical)
__device__ __forceinline__ float rlfq_stage_input(const float (&r)[kLfqMaxDim], float (&u)[kLfqMaxDim], float (&th)[kLfqMaxDim],
                                                  float (&v)[kLfqMaxDim], int d, float clamp, bool sph, float scale) {
#pragma unroll
    for (int i = 0; i < kLfqMaxDim; ++i) {
        th[i] = 0.0f;
        u[i] = r[i];
        if (i < d && clamp > 0.0f) {
            th[i] = tanhf(r[i] / clamp);
            u[i] = th[i] * clamp;
        }
    }
    float den = 1.0f;
    if (sph) {
        float ss = 0.0f;
#pragma unroll
        for (int i = 0; i < kLfqMaxDim; ++i)
            if (i < d) ss += u[i] * u[i];
        den = fmaxf(sqrtf(ss), 1e-12f);
    }
#pragma unroll
    for (int i = 0; i < kLfqMaxDim; ++i) v[i] = sph ? u[i] / den * scale : u[i];
    return den;
}

template <int D>
__global__ void __launch_bounds__(kRlfqThreads) rlfq_quantize_kernel(
    const float *__restrict__ x, int64_t x_gs, int64_t x_rs, int64_t N, int S, const float *__restrict__ k, bool sph, bool ste,
    const uint8_t *__restrict__ mask, float *__restrict__ out, int64_t out_gs, int64_t out_rs, int64_t *__restrict__ idx,
    float *__restrict__ v_all, double *__restrict__ part) {
    __shared__ double red[kRlfqThreads];
    constexpr int d = D;
    const int64_t g = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * kRlfqThreads + threadIdx.x;
    const bool valid = m < N;
    const bool use = valid && (mask == nullptr || mask[m] != 0);
    float r[kLfqMaxDim], acc[kLfqMaxDim], u[kLfqMaxDim], th[kLfqMaxDim], v[kLfqMaxDim];
    const float *xr = x + g * x_gs + (valid ? m : 0) * x_rs;
#pragma unroll
    for (int i = 0; i < kLfqMaxDim; ++i) {
        r[i] = (valid && i < d) ? xr[i] : 0.0f;
        acc[i] = 0.0f;
    }
    for (int s = 0; s < S; ++s) {
        rlfq_stage_input(r, u, th, v, d, k[S + s], sph, k[2 * S + s]);
        const float a = k[s];
        int64_t code = 0;
        double se = 0.0;
        float *vo = v_all ? v_all + (((g * S + s) * N + (valid ? m : 0)) * d) : nullptr;
#pragma unroll
        for (int i = 0; i < kLfqMaxDim; ++i) {
            if (i < d) {
                const bool pos = v[i] > 0.0f;  // zero and NaN quantize to -a (torch.where(x > 0, ...))
                const float qi = pos ? a : -a;
                code = (code << 1) | (pos ? 1 : 0);
                const float o = ste ? v[i] + (qi - v[i]) : qi;
                if (use) {
                    const double e = (double)v[i] - (double)qi;
                    se += e * e;
                }
                if (vo && valid) vo[i] = v[i];
                r[i] = r[i] - o;
                acc[i] = acc[i] + o;
            }
        }
        if (valid) idx[(g * N + m) * S + s] = code;
        if (part) {
            red[threadIdx.x] = se;
            __syncthreads();
            for (int h = kRlfqThreads / 2; h > 0; h >>= 1) {
                if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
                __syncthreads();
            }
            if (threadIdx.x == 0) part[(g * S + s) * gridDim.x + blockIdx.x] = red[0];
            __syncthreads();
        }
    }
    if (valid) {
        float *orow = out + g * out_gs + m * out_rs;
#pragma unroll
        for (int i = 0; i < kLfqMaxDim; ++i)
            if (i < d) orow[i] = acc[i];
    }
}

template <int D>
__global__ void __launch_bounds__(kRlfqThreads) rlfq_backward_kernel(
    const float *__restrict__ x, int64_t x_gs, int64_t x_rs, int64_t N, int S, const float *__restrict__ k, bool sph,
    const uint8_t *__restrict__ mask, const float *__restrict__ g_out, int64_t g_gs, int64_t g_rs,
    const float *__restrict__ w_commit, const float *__restrict__ g_ent, float *__restrict__ gx, int64_t gx_gs, int64_t gx_rs) {
    constexpr int d = D;
    const int64_t g = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * kRlfqThreads + threadIdx.x;
    if (m >= N) return;
    const bool use = mask == nullptr || mask[m] != 0;
    // g_out is re-read every stage (a cached row) rather than held: it keeps the kernel clear of register spills
    float r[kLfqMaxDim], dx[kLfqMaxDim], u[kLfqMaxDim], th[kLfqMaxDim], v[kLfqMaxDim];
    const float *xr = x + g * x_gs + m * x_rs;
    const float *gr = g_out ? g_out + g * g_gs + m * g_rs : nullptr;
    const float *wcs = (w_commit && use) ? w_commit + g * S : nullptr;
    const float *ge = g_ent ? g_ent + (g * S * N + m) * d : nullptr;  // stage s: + s * N * d
#pragma unroll
    for (int i = 0; i < kLfqMaxDim; ++i) {
        r[i] = i < d ? xr[i] : 0.0f;
        dx[i] = 0.0f;
    }
    for (int s = 0; s < S; ++s) {
        const float clamp = k[S + s], scale = k[2 * S + s], a = k[s];
        const float den = rlfq_stage_input(r, u, th, v, d, clamp, sph, scale);
        const float wc = wcs ? wcs[s] : 0.0f;
        const float *ges = ge ? ge + (int64_t)s * N * d : nullptr;
        float dot = 0.0f;
#pragma unroll
        for (int i = 0; i < kLfqMaxDim; ++i) {
            if (i < d) {
                const float qi = v[i] > 0.0f ? a : -a;
                float t = gr ? gr[i] : 0.0f;
                if (wcs) t += (v[i] - qi) * wc;
                if (ges) t += ges[i];
                dot += t * (u[i] / den);
                const float o = v[i] + (qi - v[i]);
                r[i] = r[i] - o;
                v[i] = t;  // v is dead from here on: it holds the stage's gradient at v
            }
        }
#pragma unroll
        for (int i = 0; i < kLfqMaxDim; ++i) {
            if (i < d) {
                float t = v[i];
                if (sph) t = den > 1e-12f ? (scale / den) * (t - (u[i] / den) * dot) : t * (scale / den);
                if (clamp > 0.0f) t *= 1.0f - th[i] * th[i];
                dx[i] += t;
            }
        }
    }
    float *dr = gx + g * gx_gs + m * gx_rs;
#pragma unroll
    for (int i = 0; i < kLfqMaxDim; ++i)
        if (i < d) dr[i] = dx[i];
}

int rlfq_check(int64_t G, int64_t N, int d, int S, const float *stage_consts, const char *who) {
    if (G < 1 || G > 65535 || N < 0) return fail(VQ_E_BADARG, who, "G must be in [1, 65535] and N >= 0");
    if (d < 1 || d > kLfqMaxDim) return fail(VQ_E_UNSUPPORTED, who, "codebook_dim must be in [1, 20]");
    if (S < 1 || S > VQ_RLFQ_MAX_STAGES) return fail(VQ_E_UNSUPPORTED, who, "stage count must be in [1, 32]");
    if (!stage_consts) return fail(VQ_E_BADARG, who, "null stage constants");
    if (G * N > ((int64_t)1 << 40) || rlfq_blocks(N) > 0x7fffffff) return fail(VQ_E_BADARG, who, "too many rows");
    return 0;
}

// d -> the kernel instantiated for it
#define RLFQ_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20)

template <typename... A>
int rlfq_launch_quantize(int d, dim3 grid, hipStream_t s, const char *what, A... args) {
    switch (d) {
#define RLFQ_Q(D) \
    case D: return launch<rlfq_quantize_kernel<D>>(grid, dim3(kRlfqThreads), 0, s, what, args...);
        RLFQ_CASES(RLFQ_Q)
#undef RLFQ_Q
    }
    return 0;
}

template <typename... A>
int rlfq_launch_backward(int d, dim3 grid, hipStream_t s, const char *what, A... args) {
    switch (d) {
#define RLFQ_B(D) \
    case D: return launch<rlfq_backward_kernel<D>>(grid, dim3(kRlfqThreads), 0, s, what, args...);
        RLFQ_CASES(RLFQ_B)
#undef RLFQ_B
    }
    return 0;
}
