// vq_lq.inc -- latent quantization (LatentQuantize, latent_quantization.py of the reference): the per-dimension level
// search, the straight-through value, the index and the squared-error sum of every (batch, position, codebook) sub-row in
// one pass, one thread per sub-row of d <= 16 values held in registers.
// Included by vq_kernels.hip inside its anonymous namespace after vq_lfq.inc and vq_fsq.inc, build part 0.
//
// A sub-row m = (b * P + p) * C + c reads z[b * z_bs + p * z_ps + (c * d + i) * z_cs] (i < d) and writes codes with three
// strides of its own, so a channel-first tensor [b, dim, positions] is taken as it lies (z_ps = 1, z_cs = positions:
// consecutive lanes read consecutive positions of one channel) and so is a channel-last one (z_ps = C * d, z_cs = 1).
//
// Tables.  The sum_i L_i floats of the d value tables (table i at offset L_0 + .. + L_{i-1}; learnable, so they may be
// unsorted or hold duplicates) are staged into LDS once per workgroup; the offsets follow from the by-value levels.  In
// the scan every lane reads the same LDS address, which the LDS serves as a broadcast.
//
// Per dimension i (latent_quantization.py:140-184), every step one fp32 operation (-ffp-contract=off):
//   j = argmin_j |z_i - v_i[j]|   linear scan, strict <, and a NaN distance beats any non-NaN best while the first NaN
//                                 stays: ATen's first-minimum rule
//   q = v_i[j];  c = z_i + (q - z_i)                                   (the straight-through value: two rounded operations)
//   t = ((c * 2) * hw + hw) * basis                                    (hw = L_i / 2, basis = cumprod of the levels before)
//   idx = (int32) sum_i t_i  by fsq_index<D> (torch's CPU order for d <= 7, truncating, NaN / out of range -> INT32_MIN)
//
//   lq_quantize_kernel   grid (sub-row blocks): codes, idx [B][P][C] int32 (may be NULL), and with part != NULL one fp32
//                        partial sum_(rows, i) (c_i - z_i)^2 per workgroup (serial over i in a thread, an 8-level LDS tree
//                        over the 256 threads; no atomics)
//   lq_loss_kernel       one workgroup: the partials in a fixed order in fp64 -> loss[1] = the fp32 mean m over numel,
//                        loss[0] = w_c * m + w_q * m with the reference's "a zero weight multiplies 0, not m"
//   lq_backward_kernel   one thread per element: grad_x = g_out + (g_loss[0] * coef) * (out - x), three strides each

constexpr int kLqThreads = 256;
constexpr int kLqMaxTableFloats = 4096;  // 16 KiB of LDS: sum_i L_i above it takes the module's torch path
constexpr int kLqLossThreads = 1024;

__host__ __device__ inline int64_t lq_blocks(int64_t N) { return (N + kLqThreads - 1) / kLqThreads; }

struct LqStrides {
    int64_t bs, ps, cs;  // batch, position, channel, in elements
};

template <int D>
__global__ void __launch_bounds__(kLqThreads) lq_quantize_kernel(const float *__restrict__ z, LqStrides zs, int64_t P, int C,
                                                                 int64_t N, FsqLevels lv, const float *__restrict__ tables,
                                                                 int n_table, float *__restrict__ codes, LqStrides os,
                                                                 int32_t *__restrict__ idx, float *__restrict__ part) {
    __shared__ float tab[kLqMaxTableFloats];
    __shared__ float red[kLqThreads];
    for (int i = threadIdx.x; i < n_table; i += kLqThreads) tab[i] = tables[i];
    __syncthreads();
    const int64_t m = (int64_t)blockIdx.x * kLqThreads + threadIdx.x;
    float sq = 0.0f;
    if (m < N) {
        const int64_t bp = m / C;
        const int64_t c = m - bp * C;
        const int64_t b = bp / P;
        const int64_t p = bp - b * P;
        const float *zr = z + b * zs.bs + p * zs.ps + c * D * zs.cs;
        float *orow = codes + b * os.bs + p * os.ps + c * D * os.cs;
        float t[D];
        int off = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float zi = zr[i * zs.cs];
            const int L = lv.L[i];
            float q = tab[off];
            float best = fabsf(zi - q);
            for (int j = 1; j < L; ++j) {
                const float v = tab[off + j];
                const float dist = fabsf(zi - v);
                if (dist < best || (dist != dist && best == best)) {
                    best = dist;
                    q = v;
                }
            }
            off += L;
            const float ci = zi + (q - zi);
            const float hw = (float)(L / 2);
            t[i] = (((ci * 2.0f) * hw) + hw) * (float)lv.basis[i];
            orow[i * os.cs] = ci;
            if (part) {
                const float e = ci - zi;
                sq = sq + e * e;
            }
        }
        if (idx) idx[m] = fsq_index<D>(t);
    }
    if (part) {
        red[threadIdx.x] = sq;
        __syncthreads();
        for (int k = kLqThreads / 2; k > 0; k >>= 1) {
            if ((int)threadIdx.x < k) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + k];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[blockIdx.x] = red[0];
    }
}

__global__ void __launch_bounds__(kLqLossThreads) lq_loss_kernel(const float *__restrict__ part, int64_t n, double numel,
                                                                 float w_c, float w_q, float *__restrict__ loss) {
    __shared__ double red[kLqLossThreads];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kLqLossThreads) s += (double)part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = kLqLossThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float m = (float)(red[0] / numel);
        // the reference multiplies a zero weight with a constant 0, not with the mean (which may be inf or NaN)
        const float lc = w_c * (w_c != 0.0f ? m : 0.0f);
        const float lq = w_q * (w_q != 0.0f ? m : 0.0f);
        loss[0] = lc + lq;
        loss[1] = m;
    }
}

__global__ void __launch_bounds__(kLqThreads) lq_backward_kernel(const float *__restrict__ x, LqStrides xs,
                                                                 const float *__restrict__ out, LqStrides os,
                                                                 const float *__restrict__ g_out, LqStrides gs,
                                                                 const float *__restrict__ g_loss, float coef, int64_t P, int W,
                                                                 int64_t N, float *__restrict__ gx, LqStrides ds) {
    const int64_t e = (int64_t)blockIdx.x * kLqThreads + threadIdx.x;
    if (e >= N) return;
    // positions fastest: a channel-first tensor is read along its contiguous axis
    const int64_t bw = e / P;
    const int64_t p = e - bw * P;
    const int64_t b = bw / W;
    const int64_t w = bw - b * W;
    const float k = g_loss[0] * coef;
    const float xv = x[b * xs.bs + p * xs.ps + w * xs.cs];
    const float ov = out[b * os.bs + p * os.ps + w * os.cs];
    const float gv = g_out[b * gs.bs + p * gs.ps + w * gs.cs];
    gx[b * ds.bs + p * ds.ps + w * ds.cs] = gv + k * (ov - xv);
}

// checks of the quantize entry point beyond fsq_check's (d, levels, the basis)
int lq_check(int64_t B, int64_t P, int C, int d, const int32_t *levels, int &n_table, const char *who) {
    char msg[160];
    if (B < 1 || P < 1 || C < 1) {
        snprintf(msg, sizeof msg, "%s: sizes must be positive", who);
        return fail(VQ_E_BADARG, msg);
    }
    int64_t total = 0, size = 1;
    for (int i = 0; i < d; ++i) {
        total += levels[i];
        size *= levels[i];
        if (size > 0x7fffffff) {
            snprintf(msg, sizeof msg, "%s: the codebook size overflows int32", who);
            return fail(VQ_E_BADARG, msg);
        }
    }
    if (total > kLqMaxTableFloats) {
        snprintf(msg, sizeof msg, "%s: the value tables hold more than %d floats", who, kLqMaxTableFloats);
        return fail(VQ_E_BADARG, msg);
    }
    if (B > INT64_MAX / P || B * P > INT64_MAX / C || lq_blocks(B * P * C) > 0x7fffffff) {
        snprintf(msg, sizeof msg, "%s: too many rows", who);
        return fail(VQ_E_BADARG, msg);
    }
    n_table = (int)total;
    return 0;
}

#define LQ_CASE(D) \
    case D: return launch<lq_quantize_kernel<D>>(grid, dim3(kLqThreads), 0, s, what, args...);
template <typename... A>
int lq_launch_quantize(int d, dim3 grid, hipStream_t s, const char *what, A... args) {
    switch (d) { FSQ_CASES(LQ_CASE) }
    return 0;
}
#undef LQ_CASE
