// vq_rotate.inc -- the rotation trick (Fifty et al., arXiv 2410.06424, section 4.2): backward of the quantize step with
// respect to x when the straight-through estimator is replaced by the rotation-and-rescale map.  Included by
// vq_kernels.hip inside its anonymous namespace, build part 0, after vq_finalize_ema.inc (QuantBwdParams).
//
// One stage, input row r (the residual that stage quantized), selected code c, eps = 1e-6:
//   a = max(|r|, eps)   b = max(|c|, eps)   u = r / a   qh = c / b   s = u + qh   w = s / max(|s|, eps)   lam = |c| / a
//   rot(r) = lam (r - 2 (r.w) w + 2 (r.u) qh)      with u, qh, w, lam constants of autograd; the VALUE is c (the forward
//   stays the straight-through launch), the gradient is    g -> lam (g - 2 (g.w) w + 2 (g.qh) u).
// In a residual stack every r_q is x minus detached terms, so the stages add up:
//   grad_x = sum_q lam_q (g - 2 (g.w_q) w_q + 2 (g.qh_q) u_q) + sum_q 2 grad_sq_err[q] (r_q - c_q)
// which the kernel evaluates as   sum_q ( lam_q g - alpha_q s_q + beta_q r_q + coef_q (r_q - c_q) ),
//   alpha = 2 lam (g.s) / max(|s|, eps)^2,   beta = 2 lam (g.c) / (a b),   coef = 2 grad_sq_err[q].
//
// One wave per row, four rows per 256-thread workgroup, grid-stride over the rows; no LDS, no barrier.  The row lives in
// registers: r, g and the accumulator as N values of type V per lane -- V = f32x4 at d = 4 lane + 256 j (N = ceil(D / 256)
// in {1, 2, 4}) when everything is 16-byte aligned and D % 4 == 0, else V = float at d = lane + 64 j (N = ceil(D / 64)
// rounded up to a power of two, at most 16).  Elements at d >= D are zeros: they add nothing to a dot product and are
// never stored.  Each stage runs two butterfly reductions (wave_sum4 / wave_sum2 below): |r|^2, |c|^2, g.c, then -- s formed
// elementwise in registers -- |s|^2 and g.s (|s|^2 is NOT 2 + 2 r.c / (a b): that cancels for near-antipodal rows).  The row's stage indices are loaded
// up front, one per lane, and broadcast by lane read; stage q + 1's code row is requested before stage q's reductions.
// The residual chain is the forward's: r <- r - (ste ? r + (c - r) : c), elementwise fp32, nothing contractable.
constexpr float kRotateEps = 1e-6f;
constexpr int kRotateMaxDim = 1024;

// The stage loop is bound by its vector instructions (profiles/rotation_trick.md), so the sums and the updates are explicit
// fused multiply-adds (the file is built with -ffp-contract=off; an fma only removes a rounding) and the three reciprocals and
// two square roots of a stage, which every lane computes alike, are the one-instruction forms (1 ulp each).
__device__ __forceinline__ float rot_dot(float a, float b, float acc) { return fmaf(a, b, acc); }
__device__ __forceinline__ float rot_dot(f32x4 a, f32x4 b, float acc) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}
__device__ __forceinline__ float rot_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ f32x4 rot_fma(f32x4 a, float b, f32x4 c) {
    return f32x4{fmaf(a.x, b, c.x), fmaf(a.y, b, c.y), fmaf(a.z, b, c.z), fmaf(a.w, b, c.w)};
}
__device__ __forceinline__ void rot_zero(float &v) { v = 0.0f; }
__device__ __forceinline__ void rot_zero(f32x4 &v) { v = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }

// Sums over the wave of four (two) per-lane values with the __shfl_xor butterfly, 7 (6) lane exchanges instead of 24 (12): at
// the first two steps (the first step) a lane hands the half it does not keep to its partner, so that from then on every lane
// carries ONE partial sum -- value i's in the lanes 16 i .. 16 i + 15 (32 i .. 32 i + 31).  Every total is still six
// additions deep; it is read back from its first lane as a scalar.
__device__ __forceinline__ float rot_lane_value(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

__device__ __forceinline__ void wave_sum2(float &v0, float &v1, int lane) {
    const bool hi = lane & 32;
    float k = (hi ? v1 : v0) + __shfl_xor(hi ? v0 : v1, 32);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) k += __shfl_xor(k, o);
    v0 = rot_lane_value(k, 0);
    v1 = rot_lane_value(k, 32);
}

__device__ __forceinline__ void wave_sum4(float &v0, float &v1, float &v2, float &v3, int lane) {
    const bool hi = lane & 32, mid = lane & 16;
    const float k0 = (hi ? v2 : v0) + __shfl_xor(hi ? v0 : v2, 32);
    const float k1 = (hi ? v3 : v1) + __shfl_xor(hi ? v1 : v3, 32);
    float k = (mid ? k1 : k0) + __shfl_xor(mid ? k0 : k1, 16);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) k += __shfl_xor(k, o);
    v0 = rot_lane_value(k, 0);
    v1 = rot_lane_value(k, 16);
    v2 = rot_lane_value(k, 32);
    v3 = rot_lane_value(k, 48);
}

// A row pointer is the same in every lane.  Passing it through a lane read keeps it a scalar of the row's iteration: the
// loads then address (scalar base) + (the lane's 32-bit offset) instead of one hoisted 64-bit pointer per lane and array.
// (The pointer comes back from integers, so its address space is stated: global memory.)
template <typename T>
using rot_global = T __attribute__((address_space(1)));

template <typename T>
__device__ __forceinline__ rot_global<T> *rot_uniform(T *ptr) {
    const unsigned long long v = (unsigned long long)ptr;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (rot_global<T> *)(((unsigned long long)hi << 32) | lo);
}

// (rows of up to 256 dims: at most 64 VGPRs, so that eight waves share a SIMD and hide each other's gather latency)
template <typename V, int N>
constexpr int kRotateMinWaves = sizeof(V) / 4 * N <= 4 ? 8 : 1;

template <typename V, int N>
__global__ void __launch_bounds__(256, (kRotateMinWaves<V, N>)) vq_rotate_backward_kernel(const QuantBwdParams p) {
    constexpr int W = sizeof(V) / 4;  // floats per lane and slot
    // (the wave number through a lane read: the row and every row pointer are then scalars, and a lane keeps only its offset)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = blockIdx.y;
    const long long nw = (long long)gridDim.x * 4;
    const float *xh = p.x + (long long)head * p.x_hs;
    const float *cbh = p.cb + (long long)head * p.cb_hs;
    const long long *ih = p.idx + (long long)head * p.idx_hs;
    const float *goh = p.go ? p.go + (long long)head * p.go_hs : nullptr;
    float *gxh = p.gx + (long long)head * p.gx_hs;
    const double *ge = p.g_err ? p.g_err + (long long)head * p.g_err_hs : nullptr;
    const int D = p.D, Q = p.Q;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < p.M; row += nw) {
        const auto *xr = rot_uniform(xh + row * p.x_rs);
        const auto *ir = rot_uniform(ih + row * p.idx_rs);
        const auto *gor = rot_uniform(goh ? goh + row * p.go_rs : nullptr);
        V r[N], g[N], acc[N], c[N];
        // stage `lane`'s index and loss coefficient, read by lane number in the stage loop (stages 64 .. : reloaded there)
        int kreg = lane < Q ? (int)ir[lane * p.idx_qs] : 0;
        float coefreg = (ge && lane < Q) ? (float)(2.0 * ge[lane]) : 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int d = W * lane + 64 * W * j;
            rot_zero(r[j]);
            rot_zero(g[j]);
            rot_zero(acc[j]);
            if (d < D) {
                r[j] = *(const rot_global<const V> *)(xr + d);
                if (gor) g[j] = __builtin_nontemporal_load((const rot_global<const V> *)(gor + d));
            }
        }
        {
            const auto *cr = rot_uniform(cbh + (long long)__builtin_amdgcn_readlane(kreg, 0) * D);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int d = W * lane + 64 * W * j;
                rot_zero(c[j]);
                if (d < D) c[j] = *(const rot_global<const V> *)(cr + d);
            }
        }
#pragma nounroll
        for (int q = 0; q < Q; ++q) {
            // stage q + 1's code row: it does not depend on r, so its loads are in flight during this stage's reductions
            V cn[N];
#pragma unroll
            for (int j = 0; j < N; ++j) rot_zero(cn[j]);
            if (q + 1 < Q) {
                if (((q + 1) & 63) == 0) kreg = (q + 1 + lane) < Q ? (int)ir[(long long)(q + 1 + lane) * p.idx_qs] : 0;
                const auto *cr = rot_uniform(cbh + (long long)(q + 1) * p.cb_qs + (long long)__builtin_amdgcn_readlane(kreg, (q + 1) & 63) * D);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const int d = W * lane + 64 * W * j;
                    if (d < D) cn[j] = *(const rot_global<const V> *)(cr + d);
                }
            }
            float rr = 0.0f, cc = 0.0f, gc = 0.0f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                rr = rot_dot(r[j], r[j], rr);
                cc = rot_dot(c[j], c[j], cc);
                gc = rot_dot(g[j], c[j], gc);
            }
            float unused = 0.0f;
            wave_sum4(rr, cc, gc, unused, lane);
            const float nc = __builtin_amdgcn_sqrtf(cc);
            const float a = fmaxf(__builtin_amdgcn_sqrtf(rr), kRotateEps), b = fmaxf(nc, kRotateEps);
            const float ia = __builtin_amdgcn_rcpf(a), ib = __builtin_amdgcn_rcpf(b);
            const float lam = nc * ia;
            V s[N];
            float ss = 0.0f, gs = 0.0f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                s[j] = r[j] * ia + c[j] * ib;  // (two rounded products: c = -r gives s = 0 exactly, an fma would leave a residue)
                ss = rot_dot(s[j], s[j], ss);
                gs = rot_dot(g[j], s[j], gs);
            }
            wave_sum2(ss, gs, lane);
            const float n2 = fmaxf(ss, kRotateEps * kRotateEps);  // max(|s|, eps)^2 without the root
            const float two_lam = 2.0f * lam;
            const float alpha = two_lam * gs * __builtin_amdgcn_rcpf(n2);
            const float beta = two_lam * gc * ia * ib;
            const float coef = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, coefreg), q & 63));
#pragma unroll
            for (int j = 0; j < N; ++j) {
                acc[j] = rot_fma(r[j], beta, rot_fma(s[j], -alpha, rot_fma(g[j], lam, acc[j])));
                if (ge) acc[j] = rot_fma(r[j] - c[j], coef, acc[j]);
                const V quant = p.ste ? r[j] + (c[j] - r[j]) : c[j];
                r[j] = r[j] - quant;
                c[j] = cn[j];
            }
            if (((q + 1) & 63) == 0) coefreg = (ge && (q + 1 + lane) < Q) ? (float)(2.0 * ge[q + 1 + lane]) : 0.0f;
        }
        auto *gr = rot_uniform(gxh + row * p.gx_rs);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int d = W * lane + 64 * W * j;
            if (d < D) __builtin_nontemporal_store(acc[j], (rot_global<V> *)(gr + d));
        }
    }
}
