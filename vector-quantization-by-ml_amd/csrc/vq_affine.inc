// vq_affine.inc -- affine re-parameterisation of a codebook (codebooks.py:275-348,379-384,400-403): per-column mean and
// sum of squared deviations of [H][M][D] rows in ONE read, and the elementwise moment-matching transform of [H][K][D].
// Included by vq_kernels.hip inside its anonymous namespace (build part 0).
//
// Column statistics, two stages, no atomics, every sum in a fixed order (bit-identical from run to run):
//   stage 1  workgroups of 256 threads = TC column groups x TR row lanes (TC * TR = 256, TC <= 64 a power of two).  A thread
//            owns VEC adjacent columns (VEC = 4: one float4 load per row, when base and strides are 16-byte aligned and
//            D % 4 == 0; VEC = 1 otherwise), so the TC threads of a row lane read TC * VEC contiguous floats of one row.
//            Workgroup (b, g, h) owns the columns [g * TC * VEC, (g + 1) * TC * VEC) of head h; its row lane r walks the rows
//            b * TR + r, + nblk * TR, ... with Welford's update on x minus the lane's first kept row (the reciprocal of the
//            running count is shared by the VEC columns).  From there on fp64: a lane's mean is shift + mean' (exact), the TR
//            lanes are merged pairwise in LDS (lane r takes lane r + s, s = TR / 2 .. 1) with Chan's formula and one partial
//            (n, mean, M2) per column goes to the workspace -- a mean rounded to fp32 would cost 2^-24 |mean| in every
//            difference of means that Chan's formula squares, which is what columns far from zero cannot afford.
//   stage 2  64 lanes per (head, column): lane j folds the partials b = j, j + 64, ... in that order, the lanes are merged
//            pairwise (lane j takes lane j + s, s = 32 .. 1); Chan's formula in fp64.
// The raw sum of squares is never formed.

struct AffineGeo {
    int vec;   // columns per thread: 4 (float4 loads) or 1
    int tc;    // threads across the columns of a workgroup (power of two, <= 64)
    int tr;    // row lanes of a workgroup: 256 / tc
    int cg;    // column groups (grid.y)
    int nblk;  // row blocks (grid.x) = partials per column
};

constexpr int kAffineMaxBlocks = 1024;   // partials per column at most
constexpr int kAffineRowsPerLane = 16;   // rows a row lane should get before another workgroup is worth its partial

inline AffineGeo affine_geo(int H, long long M, int D, bool vec) {
    AffineGeo g;
    g.vec = vec ? 4 : 1;
    const int per_row = (D + g.vec - 1) / g.vec;
    g.tc = 1;
    while (g.tc < per_row && g.tc < 64) g.tc *= 2;
    g.tr = 256 / g.tc;
    g.cg = (per_row + g.tc - 1) / g.tc;
    long long cap = kAffineMaxBlocks / ((long long)H * g.cg);
    if (cap < 1) cap = 1;
    long long nblk = (M + (long long)g.tr * kAffineRowsPerLane - 1) / ((long long)g.tr * kAffineRowsPerLane);
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    g.nblk = (int)nblk;
    return g;
}

// workspace: [n: H * nblk uint32, rounded to 64 entries][mean: H * nblk * D doubles][M2: H * nblk * D doubles]
inline long long affine_ws_counts(int H, int nblk) { return ((long long)H * nblk + 63) / 64 * 64; }

// Chan's pairwise merge of (nb, mb, qb) into (na, ma, qa)
__device__ __forceinline__ void affine_merge(double na, double &ma, double &qa, double nb, double mb, double qb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        ma = mb;
        qa = qb;
        return;
    }
    const double delta = mb - ma;
    const double w = nb / (na + nb);
    ma = ma + delta * w;
    qa = qa + qb + delta * delta * (na * w);
}

template <int VEC>
__global__ __launch_bounds__(256) void vq_affine_stats_kernel(const float *__restrict__ x, long long x_rs, long long x_hs,
                                                              const uint8_t *__restrict__ mask, long long m_rs, long long m_hs, long long M,
                                                              int D, int tc, int nblk, unsigned *__restrict__ part_n,
                                                              double *__restrict__ part_mean, double *__restrict__ part_m2) {
    __shared__ double s_mean[256 * VEC];
    __shared__ double s_m2[256 * VEC];
    __shared__ double s_n[256];
    const int tid = threadIdx.x;
    const int tr = 256 / tc;
    const int c_lane = tid % tc, r_lane = tid / tc;
    const int h = blockIdx.z;
    const int col = ((int)blockIdx.y * tc + c_lane) * VEC;  // first column of this thread
    const bool live = col < D;                              // (VEC = 4: D % 4 == 0, so the four columns are live together)
    const float *xh = x + (long long)h * x_hs + col;
    const uint8_t *mh = mask ? mask + (long long)h * m_hs : nullptr;

    // Welford on x - shift, shift = the lane's first kept row: the running mean stays of the size of the spread, so its
    // rounding does not grow with the columns' offset (mean 1000, sigma 1); the subtraction is exact for nearby values
    float mean[VEC], m2[VEC], shift[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) mean[v] = m2[v] = shift[v] = 0.0f;
    unsigned n = 0;
    const long long step = (long long)nblk * tr;
    for (long long r0 = (long long)blockIdx.x * tr + r_lane; r0 < M; r0 += 4 * step) {
        // four rows in flight, folded in row order
        float val[4][VEC];
        bool keep[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long r = r0 + u * step;
            keep[u] = live && r < M && (!mh || mh[r * m_rs] != 0);
            if (keep[u]) {
                if constexpr (VEC == 4) {
                    const f32x4 t = *reinterpret_cast<const f32x4 *>(xh + r * x_rs);
                    val[u][0] = t.x; val[u][1] = t.y; val[u][2] = t.z; val[u][3] = t.w;
                } else {
                    val[u][0] = xh[r * x_rs];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!keep[u]) continue;
            if (n == 0) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) shift[v] = val[u][v];
            }
            n += 1;
            const float inv = 1.0f / (float)n;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float t = val[u][v] - shift[v];
                const float d = t - mean[v];
                mean[v] = mean[v] + d * inv;
                m2[v] = m2[v] + d * (t - mean[v]);
            }
        }
    }

    // merge the row lanes: lane r takes lane r + s
    s_n[tid] = (double)n;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        s_mean[tid * VEC + v] = (double)shift[v] + (double)mean[v];
        s_m2[tid * VEC + v] = (double)m2[v];
    }
    __syncthreads();
    for (int s = tr / 2; s > 0; s >>= 1) {
        if (r_lane < s) {
            const int o = tid + s * tc;
            const double na = s_n[tid], nb = s_n[o];
#pragma unroll
            for (int v = 0; v < VEC; ++v) affine_merge(na, s_mean[tid * VEC + v], s_m2[tid * VEC + v], nb, s_mean[o * VEC + v], s_m2[o * VEC + v]);
            s_n[tid] = na + nb;
        }
        __syncthreads();
    }
    if (r_lane == 0 && live) {
        const long long slot = (long long)h * nblk + blockIdx.x;
        if (blockIdx.y == 0 && c_lane == 0) part_n[slot] = (unsigned)s_n[tid];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            part_mean[slot * D + col + v] = s_mean[tid * VEC + v];
            part_m2[slot * D + col + v] = s_m2[tid * VEC + v];
        }
    }
}

// stage 2: a workgroup owns 4 columns of a head; its 64 lanes per column fold the partials b = lane, lane + 64, ... in that
// order (four loads in flight) and are merged pairwise in LDS (lane j takes lane j + s, s = 32 .. 1).  All in fp64.
// (One thread per column walking all partials is a chain of up to 1024 dependent loads: 0.7 ms at cfg2, ten times stage 1.)
__global__ __launch_bounds__(256) void vq_affine_merge_kernel(const unsigned *__restrict__ part_n, const double *__restrict__ part_mean,
                                                              const double *__restrict__ part_m2, int H, int D, int nblk,
                                                              long long *__restrict__ count, float *__restrict__ mean, float *__restrict__ m2) {
    __shared__ double s_n[256], s_mean[256], s_m2[256];
    const int tid = threadIdx.x, c = tid & 3, j = tid >> 2;
    const int h = blockIdx.y, d = (int)blockIdx.x * 4 + c;
    double na = 0.0, ma = 0.0, qa = 0.0;
    if (d < D) {
        for (int b0 = j; b0 < nblk; b0 += 4 * 64) {
            double nb[4], mb[4], qb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int b = b0 + u * 64;
                nb[u] = mb[u] = qb[u] = 0.0;
                if (b < nblk) {
                    const long long slot = (long long)h * nblk + b;
                    nb[u] = (double)part_n[slot];
                    mb[u] = part_mean[slot * D + d];
                    qb[u] = part_m2[slot * D + d];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                affine_merge(na, ma, qa, nb[u], mb[u], qb[u]);
                na += nb[u];
            }
        }
    }
    s_n[tid] = na;
    s_mean[tid] = ma;
    s_m2[tid] = qa;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (j < s) {
            const int o = tid + s * 4;
            const double a = s_n[tid], b = s_n[o];
            affine_merge(a, s_mean[tid], s_m2[tid], b, s_mean[o], s_m2[o]);
            s_n[tid] = a + b;
        }
        __syncthreads();
    }
    if (j == 0 && d < D) {
        if (d == 0) count[h] = (long long)s_n[tid];
        mean[(long long)h * D + d] = (float)s_mean[tid];
        m2[(long long)h * D + d] = (float)s_m2[tid];
    }
}

// The moment-matching transform, std = sqrt(clamp(var, min = 1e-5)) as torch.clamp rounds it (a NaN variance stays NaN).
//   mode 0  codes -> batch space:             out = (in - cm) * (bstd / cstd) + bm           (codebooks.py:380-384, that operation order)
//   mode 1  accumulated sums -> codebook space: out = in * r + hits * (cm - bm * r), r = cstd / bstd
//           (= the sums of (x - bm) * r + cm over the rows of a code, codebooks.py:401-403, from the sums of the raw rows)
__device__ __forceinline__ float affine_std(float var) { return sqrtf(var < 1e-5f ? 1e-5f : var); }

__global__ __launch_bounds__(256) void vq_affine_apply_kernel(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hits,
                                                              const float *__restrict__ cm, const float *__restrict__ cv,
                                                              const float *__restrict__ bm, const float *__restrict__ bv, int K, int D, long long total,
                                                              int mode) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long hk = i / D;
    const int d = (int)(i % D);
    const long long s = (hk / K) * D + d;  // (head, column)
    const float cstd = affine_std(cv[s]), bstd = affine_std(bv[s]);
    if (mode == 0) {
        const float scale = bstd / cstd;
        out[i] = (in[i] - cm[s]) * scale + bm[s];
    } else {
        const float r = cstd / bstd;
        out[i] = in[i] * r + hits[hk] * (cm[s] - bm[s] * r);
    }
}
