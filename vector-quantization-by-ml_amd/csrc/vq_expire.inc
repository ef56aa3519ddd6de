// vq_expire.inc -- dead-code expiry decided and carried out on the device (codebooks.py:216-262: expire_codes_ / replace;
// Codebook.reseed_dead_codes here).  Included by vq_kernels.hip in build part 0, behind vq_sample.inc (philox4x32_10).
// ------------------------------------------------------------------------------------------------
// Two launches, both issued unconditionally; nothing is read back by the host.
//   vq_expire_scan_kernel   one workgroup per head.  256 threads x 4 consecutive codes = 1024 codes per pass; a thread counts
//                           its dead codes, the wave scans the counts with shuffles, the four wave totals cross one barrier per
//                           pass (two LDS rows, alternating), the running total carries the rank from pass to pass.  Writes
//                           the dead codes in ascending order to list[h][0 .. n_dead), n_dead[h], and picked = -1 for the live.
//   vq_expire_copy_kernel   one wave per dead slot r (grid-strided; a wave whose first slot is >= n_dead leaves at once):
//                           selects the pool row (the rule below, wave-uniform), rebuilds it from the residual chain when one
//                           is given, normalises it when asked to, and writes the three entries of code list[h][r].
// The selection rule is stated in include/vq_mi355x.h (vq_expire_codes_f32); expire_select below is that text in code.
// ------------------------------------------------------------------------------------------------
constexpr int kExpireScanCodes = 1024;  // codes per pass of the scan
constexpr int kExpireRounds = 6;        // Feistel rounds per application of the bijection
constexpr int kExpireWalkBound = 64;    // applications of the bijection before the walk gives up

// one application of the keyed bijection of [0, 2^b)
__device__ __forceinline__ unsigned long long expire_feistel(unsigned long long y, int b, unsigned c2, unsigned c3, unsigned k0,
                                                             unsigned k1) {
    int wl = b >> 1, wr = b - wl;  // widths of the high and of the low part; they swap every round
    for (int i = 0; i < kExpireRounds; ++i) {
        const unsigned long long hi = y >> wr, lo = y & ((1ull << wr) - 1ull);
        unsigned w[4];
        philox4x32_10((unsigned)lo, (unsigned)i, c2, c3, k0, k1, w);
        y = (lo << wl) | ((hi ^ (unsigned long long)w[0]) & ((1ull << wl) - 1ull));
        const int t = wl;
        wl = wr;
        wr = t;
    }
    return y;
}

// the pool row of the dead code of rank r in head h; always inside [0, N)
__device__ __forceinline__ long long expire_select(unsigned long long seed0, unsigned long long seed1, int h, long long r,
                                                   long long n_dead, long long N) {
    const unsigned k0 = (unsigned)seed0, k1 = (unsigned)(seed0 >> 32);
    const unsigned long long c = ((unsigned long long)(unsigned)h << 32) + seed1;
    const unsigned c2 = (unsigned)c, c3 = (unsigned)(c >> 32);
    if (n_dead > N) {  // more dead codes than rows: draws with replacement
        unsigned w[4];
        philox4x32_10((unsigned)r, 0xFFFFFFFFu, c2, c3, k0, k1, w);
        return (long long)((((unsigned long long)w[1] << 32) | (unsigned long long)w[0]) % (unsigned long long)N);
    }
    const unsigned long long last = (unsigned long long)(N - 1);
    const int b = last ? 64 - __clzll((long long)last) : 0;  // bit length of N - 1: 2^b < 2 N
    unsigned long long y = (unsigned long long)r;
    for (int t = 0; t < kExpireWalkBound; ++t) {
        y = expire_feistel(y, b, c2, c3, k0, k1);
        if (y < (unsigned long long)N) return (long long)y;
    }
    return (long long)(y - (unsigned long long)N);  // the bound: y < 2^b < 2 N, so this is in range (not injective any more)
}

__global__ void __launch_bounds__(256) vq_expire_scan_kernel(const float *__restrict__ cluster_size, int K, float threshold,
                                                             int *__restrict__ n_dead_ws, int *__restrict__ list_ws,
                                                             long long *__restrict__ picked, int *__restrict__ n_expired) {
    __shared__ int s_tot[2][4];
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *cs = cluster_size + (long long)h * K;
    int *list = list_ws + (long long)h * K;
    long long *pk = picked ? picked + (long long)h * K : nullptr;
    int ranked = 0;  // dead codes of the passes before this one
    for (int k0 = 0, pass = 0; k0 < K; k0 += kExpireScanCodes, ++pass) {
        const int k = k0 + tid * 4;
        bool dead[4];
        int mine = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dead[e] = k + e < K && cs[k + e] < threshold;  // (a NaN is not dead)
            mine += dead[e] ? 1 : 0;
        }
        int upto = mine;  // inclusive scan over the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int v = __shfl_up(upto, s, 64);
            if (lane >= s) upto += v;
        }
        if (lane == 63) s_tot[pass & 1][wave] = upto;
        __syncthreads();  // (the row written two passes later is read before the barrier in between)
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int t = s_tot[pass & 1][w];
            before += w < wave ? t : 0;
            total += t;
        }
        int r = ranked + before + upto - mine;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (k + e < K) {
                if (dead[e]) list[r++] = k + e;
                else if (pk) pk[k + e] = -1;
            }
        }
        ranked += total;
    }
    if (tid == 0) {
        n_dead_ws[h] = ranked;
        if (n_expired) n_expired[h] = ranked;
    }
}

struct ExpireChain {  // the residual chain of ONE head: row n of the pool is r_stage of x row n
    const float *x;
    long long x_rs;
    const float *cb;
    long long cb_qs;
    const long long *idx;
    long long idx_rs, idx_qs;
    int stage;
};

// Both load paths give a lane the same four consecutive elements d .. d + 3 (d = 4 lane + 256 i), so the sum of squares of
// the normalisation adds up in ONE order whether the row lies on the 16-byte grid or not; elements past D read as 0.
template <bool VEC>
__device__ __forceinline__ void expire_load(const float *p, int n, float (&v)[4]) {
    if constexpr (VEC) {
        const f32x4 t = *(const f32x4 *)p;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < n ? p[e] : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void expire_store(float *p, int n, const float (&v)[4]) {
    if constexpr (VEC) {
        *(f32x4 *)p = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) p[e] = v[e];
    }
}

// elements d .. d + n - 1 of pool row `sel`: the row itself, or _residual_chain(ste=True)'s operations on it, in its order
template <bool VEC>
__device__ __forceinline__ void expire_fetch(const float *src, const ExpireChain &ch, bool chained, long long sel, int K, int D,
                                             int d, int n, float (&r)[4]) {
    expire_load<VEC>(src + d, n, r);
    if (!chained) return;
    for (int j = 0; j < ch.stage; ++j) {
        const long long k = ch.idx[sel * ch.idx_rs + j * ch.idx_qs];
        if (k < 0 || k >= K) break;  // a dropped stage ends the row's chain (vq_ema_accumulate_residual_f32's rule)
        float c[4];
        expire_load<VEC>(ch.cb + j * ch.cb_qs + k * D + d, n, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float quant = r[e] + (c[e] - r[e]);
            r[e] = r[e] - quant;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void expire_write_row(const float *src, const ExpireChain &ch, bool chained, long long sel, int K, int D,
                                                 int lane, float reset, int l2norm, float *emb, float *avg) {
    float denom = 1.0f;
    if (l2norm) {  // F.normalize: row / max(||row||, 1e-12)
        float ss = 0.0f;
        for (int d = lane * 4; d < D; d += 256) {
            float r[4];
            expire_fetch<VEC>(src, ch, chained, sel, K, D, d, D - d, r);
#pragma unroll
            for (int e = 0; e < 4; ++e) ss += r[e] * r[e];
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) ss += __shfl_xor(ss, s, 64);
        const float norm = sqrtf(ss);
        denom = norm < 1e-12f ? 1e-12f : norm;  // (a NaN norm stays NaN, as clamp_min leaves it)
    }
    for (int d = lane * 4; d < D; d += 256) {
        float r[4], a[4];
        expire_fetch<VEC>(src, ch, chained, sel, K, D, d, D - d, r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (l2norm) r[e] = r[e] / denom;
            a[e] = r[e] * reset;
        }
        expire_store<VEC>(emb + d, D - d, r);
        expire_store<VEC>(avg + d, D - d, a);
    }
}

__device__ __forceinline__ bool expire_aligned16(const void *p) { return ((unsigned long long)p & 15ull) == 0; }

__global__ void __launch_bounds__(256) vq_expire_copy_kernel(float *__restrict__ cluster_size, float *__restrict__ embed_avg,
                                                             float *__restrict__ embeddings, const float *__restrict__ pool,
                                                             long long pool_rs, long long pool_hs, long long N, ExpireChain ch,
                                                             int chained, int K, int D, float reset, int l2norm,
                                                             const long long *__restrict__ seed, long long *__restrict__ picked,
                                                             const int *__restrict__ n_dead_ws, const int *__restrict__ list_ws) {
    const int h = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_dead = n_dead_ws[h];
    const unsigned long long seed0 = (unsigned long long)seed[0], seed1 = (unsigned long long)seed[1];
    for (int slot = blockIdx.x * 4 + wave; slot < n_dead; slot += gridDim.x * 4) {
        const int k = list_ws[(long long)h * K + slot];
        const long long sel = expire_select(seed0, seed1, h, slot, n_dead, N);
        const long long code = (long long)h * K + k;
        const float *src = chained ? ch.x + sel * ch.x_rs : pool + (long long)h * pool_hs + sel * pool_rs;
        float *emb = embeddings + code * D, *avg = embed_avg + code * D;
        const bool vec = D % 4 == 0 && expire_aligned16(src) && expire_aligned16(emb) && expire_aligned16(avg) &&
                         (!chained || ch.stage == 0 || (expire_aligned16(ch.cb) && ch.cb_qs % 4 == 0));
        if (vec) expire_write_row<true>(src, ch, chained != 0, sel, K, D, lane, reset, l2norm, emb, avg);
        else expire_write_row<false>(src, ch, chained != 0, sel, K, D, lane, reset, l2norm, emb, avg);
        if (lane == 0) {
            cluster_size[code] = reset;
            if (picked) picked[code] = sel;
        }
    }
}
