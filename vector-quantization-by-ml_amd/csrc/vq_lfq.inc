// vq_lfq.inc -- lookup-free quantization (LFQ, lookup_free_quantization.py:294-348 of the reference): the sign quantizer
// and the entropy aux loss over the implicit codebook {-a, +a}^d, without ever holding a [rows, 2^d] matrix.
// Included by vq_kernels.hip inside its anonymous namespace, build part 0 (see "Build parts" there).
//
// The softmax over {+-a}^d factorises per dim: p_k = prod_i pi_i(b_{k,i}), pi_i(1) = sigmoid(z_i), pi_i(0) = sigmoid(-z_i),
// z_i = 4 tau a v_i (the reference's logits are 2 tau a sum_i v_i (2 b_{k,i} - 1)).  Code k = u * NB + w: the high
// h = ceil(d / 2) dims are the bits of u, the low d - h dims the bits of w, so p_k = A_u * B_w with two per-row tables of
// at most 1024 entries (log p_k = LA_u + LB_w).  Bit b_{k,i} is bit d - 1 - i of k (dim 0 is the MSB, the reference's mask).
//
//   lfq_quantize_kernel     one thread per (row, codebook): signs -> +-qmag, int64 index, straight-through, squared error
//                           (fp64 per-block partials, summed in a fixed order by lfq_sum_kernel)
//   lfq_entropy_fwd_kernel  one wave per (selected row, codebook): tables in LDS, the 2^d-pair sweep of the clamped
//                           per-sample entropy; writes A and B to the workspace for the codebook term
//   lfq_avg_prob_kernel     avg_prob[c, k] = sum_rows A_u B_w: one thread per code, rows split over blockIdx.y, fp64
//                           partials; lfq_avg_reduce_kernel adds the splits in order and divides by the row count
//   lfq_entropy_bwd_kernel  one wave per (selected row, codebook): tables rebuilt in LDS, one sweep gives
//                           S0 = sum_k g_k p_k and S_i = sum_k g_k p_k b_{k,i};  dL/dv_i = 4 tau a (S_i - pi_i(1) S0)
//                           with g_k centred first (see the kernel: the difference cancels when g_k is nearly constant)
// No float atomics anywhere: every sum has one fixed order, so results are bitwise run-to-run reproducible.
//
// Stage axis (the residual LFQ's stage-batched calls, vq_lfq_entropy_staged_*): every entropy kernel and lfq_sum_kernel take
// a stage index from one grid axis and offset their inputs and outputs by per-stage strides; the code scale comes from
// LfqCoef.  A single-stage call is the T = 1 case of the same kernels, so stage t of a staged call runs exactly the
// arithmetic of a single-stage call on that stage's inputs (same row split, same summation order: bitwise equal).

constexpr int kLfqMaxDim = 20;
constexpr int kLfqSumThreads = 1024;
constexpr int kLfqQuantThreads = 256;
constexpr int kLfqAvgCodes = 256;  // codes per lfq_avg_prob_kernel block
constexpr float kLfqEps = 1e-5f;   // the reference's log clamp (utils/general.py:25-26)
// The stage coefficient 4 tau a of an entropy kernel: coef0 for a single-stage call; with a device array code_scale
// (a staged call), four_tau * code_scale[t % period].  (Not a by-value array indexed by the stage: such an argument is
// copied into registers, which doubled lfq_entropy_fwd_kernel's VGPRs.  A device array indexed by the block-uniform t is
// a scalar load.)  four_tau * code_scale is the host's 4.0f * tau * code_scale, operation for operation.
struct LfqCoef {
    float coef0, four_tau;
    const float *code_scale;
    int period;
};

__device__ __forceinline__ float lfq_coef(const LfqCoef &k, int t) {
    return k.code_scale ? k.four_tau * k.code_scale[t % k.period] : k.coef0;
}

__device__ __forceinline__ float lfq_sigmoid(float z) {
    // both branches are exact-ish: no 1 - sigmoid cancellation (pi_i(0) is sigmoid(-z) evaluated directly)
    if (z >= 0.0f) return 1.0f / (1.0f + expf(-z));
    const float e = expf(z);
    return e / (1.0f + e);
}

__device__ __forceinline__ float lfq_logsigmoid(float z) { return fminf(z, 0.0f) - log1pf(expf(-fabsf(z))); }

__device__ __forceinline__ float lfq_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lane 0's value in every lane (a butterfly sum may differ in its last bit from lane to lane)
__device__ __forceinline__ float lfq_readfirstlane(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// ------------------------------------------------------------------------------------------------
// quantize step (lookup_free_quantization.py:250-276, 323-336 commitment)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLfqQuantThreads) lfq_quantize_kernel(
    const float *__restrict__ v, int64_t v_rs, const float *__restrict__ xa, int64_t xa_rs, int64_t N, int C, int d,
    float qmag, const uint8_t *__restrict__ mask, float *__restrict__ q, float *__restrict__ out, int64_t *__restrict__ idx,
    double *__restrict__ part) {
    __shared__ double red[kLfqQuantThreads];
    const int64_t task = (int64_t)blockIdx.x * kLfqQuantThreads + threadIdx.x;
    double se = 0.0;
    if (task < N * C) {
        const int64_t m = task / C;
        const int c = (int)(task - m * C);
        const float *vr = v + m * v_rs + (int64_t)c * d;
        const int64_t o = task * d;
        const bool use = mask == nullptr || mask[m] != 0;
        int64_t code = 0;
        for (int i = 0; i < d; ++i) {
            const float x = vr[i];
            const bool pos = x > 0.0f;  // zero and NaN quantize to -a (torch.where(x > 0, ...))
            const float qi = pos ? qmag : -qmag;
            code = (code << 1) | (pos ? 1 : 0);
            q[o + i] = qi;
            if (out) {
                const float a = xa[m * xa_rs + (int64_t)c * d + i];
                out[o + i] = a + (qi - a);
            }
            if (use) {
                const double e = (double)x - (double)qi;
                se += e * e;
            }
        }
        idx[task] = code;
    }
    if (part) {
        red[threadIdx.x] = se;
        __syncthreads();
        for (int s = kLfqQuantThreads / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[blockIdx.x] = red[0];
    }
}

// one block: out[0] = sum of n values in a fixed order (thread-strided fp64 sums, then a tree)
// (block b sums in[b * in_stride ...] into out[b]: one block per stage of a staged call)
template <typename T>
__global__ void __launch_bounds__(kLfqSumThreads) lfq_sum_kernel(const T *__restrict__ in, int64_t n, double *__restrict__ out,
                                                                 int64_t in_stride) {
    __shared__ double red[kLfqSumThreads];
    in += (int64_t)blockIdx.x * in_stride;
    out += blockIdx.x;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kLfqSumThreads) s += (double)in[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = kLfqSumThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ------------------------------------------------------------------------------------------------
// per-row tables in LDS (one wave per (selected row, codebook) task)
// ------------------------------------------------------------------------------------------------
struct LfqShape {
    int d, h, l, NA, NB;  // h = ceil(d / 2) high dims (bits of u), l = d - h low dims (bits of w), NA = 2^h, NB = 2^l
};

__host__ __device__ inline LfqShape lfq_shape(int d) {
    LfqShape s;
    s.d = d;
    s.h = (d + 1) / 2;
    s.l = d - s.h;
    s.NA = 1 << s.h;
    s.NB = 1 << s.l;
    return s;
}

// floats of LDS one task uses: 4 per-dim arrays (padded to 32) + A, LA, B, LB
__host__ __device__ inline int lfq_task_lds_floats(const LfqShape &s) { return 4 * 32 + 2 * s.NA + 2 * s.NB; }

// Fills the task's LDS region: s1/s0 = sigmoid(+-z), l1/l0 = logsigmoid(+-z) per dim, then A/LA (high dims) and B/LB
// (low dims).  Lane i < d holds z_i on return (0 elsewhere).  Every lane of the block must reach both barriers.
// Centred (the backward): l1/l0 hold the logs minus their mean under pi, logsigmoid(+-z) + H_i = s0 z and -s1 z (exact
// because logsigmoid(z) - logsigmoid(-z) = z), so LA_u + LB_w = log p_k + H with H = sum_i H_i the row's entropy; lane
// i < d returns H_i in *h_i and max(logsigmoid(+-z_i)) in *lmax_i (0 elsewhere).
__device__ __forceinline__ float lfq_build_tables(float *lds, const LfqShape &S, const float *vr, float coef, bool valid,
                                                  int lane, float *h_i = nullptr, float *lmax_i = nullptr) {
    float *s1 = lds, *s0 = lds + 32, *l1 = lds + 64, *l0 = lds + 96;
    float *A = lds + 128, *LA = A + S.NA, *B = LA + S.NA, *LB = B + S.NB;
    float z = 0.0f;
    if (valid && lane < S.d) {
        z = coef * vr[lane];
        const float p1 = lfq_sigmoid(z), p0 = lfq_sigmoid(-z);
        const float g1 = lfq_logsigmoid(z), g0 = lfq_logsigmoid(-z);
        s1[lane] = p1;
        s0[lane] = p0;
        if (h_i) {
            // (a zero probability times an infinite log or z counts as 0: an infinite input stays finite here)
            *h_i = -((p1 > 0.0f ? p1 * g1 : 0.0f) + (p0 > 0.0f ? p0 * g0 : 0.0f));
            *lmax_i = fmaxf(g1, g0);
            l1[lane] = p0 > 0.0f ? p0 * z : 0.0f;
            l0[lane] = p1 > 0.0f ? -(p1 * z) : 0.0f;
        } else {
            l1[lane] = g1;
            l0[lane] = g0;
        }
    }
    __syncthreads();
    if (valid) {
        for (int u = lane; u < S.NA; u += 64) {
            float p = 1.0f, lp = 0.0f;
            for (int i = 0; i < S.h; ++i) {
                const bool b = (u >> (S.h - 1 - i)) & 1;
                p *= b ? s1[i] : s0[i];
                lp += b ? l1[i] : l0[i];
            }
            A[u] = p;
            LA[u] = lp;
        }
        for (int w = lane; w < S.NB; w += 64) {
            float p = 1.0f, lp = 0.0f;
            for (int j = 0; j < S.l; ++j) {
                const int i = S.h + j;
                const bool b = (w >> (S.l - 1 - j)) & 1;
                p *= b ? s1[i] : s0[i];
                lp += b ? l1[i] : l0[i];
            }
            B[w] = p;
            LB[w] = lp;
        }
    }
    __syncthreads();
    return z;
}

// ------------------------------------------------------------------------------------------------
// entropy forward: per-sample entropy of every task + the A / B tables for the codebook term
// ------------------------------------------------------------------------------------------------
// stage t = blockIdx.y: v + t * v_ss, rows + t * rows_ss; ent / tabA / tabB are [T][R * C][...]
__global__ void __launch_bounds__(256) lfq_entropy_fwd_kernel(const float *__restrict__ v, int64_t v_rs, int64_t v_ss,
                                                              const int64_t *__restrict__ rows, int64_t rows_ss, int64_t R,
                                                              int C, int d, LfqCoef coefs, float *__restrict__ ent,
                                                              float *__restrict__ tabA, float *__restrict__ tabB) {
    extern __shared__ float lfq_lds[];
    const LfqShape S = lfq_shape(d);
    const int t = blockIdx.y;
    const float coef = lfq_coef(coefs, t);
    v += (int64_t)t * v_ss;
    if (rows) rows += (int64_t)t * rows_ss;
    ent += (int64_t)t * R * C;
    tabA += (int64_t)t * R * C * S.NA;
    tabB += (int64_t)t * R * C * S.NB;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    const bool valid = task < R * C;
    const int64_t j = valid ? task / C : 0;
    const int c = valid ? (int)(task - j * C) : 0;
    const int64_t m = valid ? (rows ? rows[j] : j) : 0;
    float *lds = lfq_lds + wave * lfq_task_lds_floats(S);
    lfq_build_tables(lds, S, v + m * v_rs + (int64_t)c * d, coef, valid, lane);
    if (!valid) return;
    const float *A = lds + 128, *LA = A + S.NA, *B = LA + S.NA, *LB = B + S.NB;
    float *gA = tabA + task * S.NA, *gB = tabB + task * S.NB;
    for (int u = lane; u < S.NA; u += 64) gA[u] = A[u];
    for (int w = lane; w < S.NB; w += 64) gB[w] = B[w];
    const int P = 1 << d;
    const float log_eps = logf(kLfqEps);
    float acc = 0.0f;
    for (int k = lane; k < P; k += 64) {
        const int u = k >> S.l, w = k & (S.NB - 1);
        const float p = A[u] * B[w];
        const float lg = p >= kLfqEps ? LA[u] + LB[w] : log_eps;
        acc = fmaf(p, lg, acc);
    }
    acc = lfq_wave_sum(acc);
    if (lane == 0) ent[task] = -acc;
}

// avg_prob partials: part[(split * C + c) * P + k] = sum over the split's rows of A_u B_w  (fp64, rows in order)
// (stage t = blockIdx.z / C: its tables at tabA / tabB + t * R * C * NA / NB, its partials at part + t * splits * C * P)
__global__ void __launch_bounds__(kLfqAvgCodes) lfq_avg_prob_kernel(const float *__restrict__ tabA, const float *__restrict__ tabB,
                                                                    int64_t R, int C, int d, int64_t rows_per_split,
                                                                    int64_t splits, double *__restrict__ part) {
    const LfqShape S = lfq_shape(d);
    const int P = 1 << d;
    const int k = blockIdx.x * kLfqAvgCodes + threadIdx.x;
    const int t = blockIdx.z / C;
    const int c = blockIdx.z - t * C;
    const int split = blockIdx.y;
    if (k >= P) return;
    tabA += (int64_t)t * R * C * S.NA;
    tabB += (int64_t)t * R * C * S.NB;
    part += (int64_t)t * splits * C * P;
    const int u = k >> S.l, w = k & (S.NB - 1);
    const int64_t r0 = (int64_t)split * rows_per_split;
    const int64_t r1 = r0 + rows_per_split < R ? r0 + rows_per_split : R;
    double acc = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t t = r * C + c;
        acc += (double)(tabA[t * S.NA + u] * tabB[t * S.NB + w]);
    }
    part[((int64_t)split * C + c) * P + k] = acc;
}

__global__ void __launch_bounds__(256) lfq_avg_reduce_kernel(const double *__restrict__ part, int splits, int64_t CP,
                                                             double inv_rows, float *__restrict__ avg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= CP) return;
    part += (int64_t)blockIdx.y * splits * CP;  // stage blockIdx.y
    avg += (int64_t)blockIdx.y * CP;
    double s = 0.0;
    for (int z = 0; z < splits; ++z) s += part[(int64_t)z * CP + i];
    avg[i] = (float)(s * inv_rows);
}

// ------------------------------------------------------------------------------------------------
// entropy backward.  g_k = w_ps * G(p_k) + w_cb[c, k]: G(x) = -(log x + 1) for x >= 1e-5, -log 1e-5 below (the clamp);
// w_ps (device scalar) carries the upstream gradient of the per-sample entropy and its 1 / (rows * C); w_cb the codebook
// term's G(avg_prob) with its upstream gradient, 1 / (C * world * rows) folded in by the caller.
// Pair k = s * 64 + lane: the low 6 bits of k are the lane's own, so their S_i are bit * S0 of the lane; the bits above
// are the same for the whole wave (one add per set bit per pair).
// Centring.  sum_k p_k (b_{k,i} - pi_i(1)) = 0, so S_i - pi_i(1) S0 does not change when one constant is subtracted from
// every g_k; in fp32 it decides whether the difference cancels.  Uncentred, g_k nearly constant (the codebook term once
// avg_prob is near uniform, the per-sample term at small tau a |v|) left fp32 sums of 2^d / 64 terms of size |g| whose
// difference is a small fraction of |g|: errors of percents of the gradient at d = 16, all of it at d = 20.  The kernel
// subtracts w_ps (H - 1 + D) + c_cb, an estimate of sum_k g_k p_k made of wave-uniform constants of the task:
//   H - 1   the p-weighted mean of G without the clamp (H = sum_i H_i, the row's entropy), so the unclamped branch is
//           G - (H - 1) = -(LA_u + LB_w) on the centred tables (no rounding of log p_k against H);
//   D       0, or -log 1e-5 + 1 - H when every code lies below the clamp (sum_i max logsigmoid < log 1e-5): then every
//           centred G is exactly 0, as is the exact per-sample gradient;
//   c_cb    p_m w_cb[c, k_m] + (1 - p_m) wbar: k_m the row's most likely code (the signs of z), p_m its probability,
//           wbar the mean of w_cb[c, .] over 64 codes spread evenly over the 2^d (all of them when d < 6).  A saturated
//           row puts its weight on k_m, a flat one spreads it: either way c_cb is close to the p-weighted mean of w_cb.
// Per pair that is one subtraction, w_cb[k] - c_cb, before the fma: the difference of two nearby fp32 values is exact, and
// the fma then rounds the centred g_k once.  (Folding c_cb / w_ps into D instead saves the subtraction but rounds
// -(LA + LB + D) at the scale of c_cb / w_ps, which is the cancellation again when the two terms nearly cancel.)
// Each constant is read from lane 0 (readfirstlane): one value for the whole sweep, or the identity would not hold.
// ------------------------------------------------------------------------------------------------
// stage t = blockIdx.y: v + t * v_ss, rows + t * rows_ss, w_ps + t, w_cb + t * C * 2^d, gv + t * gv_ss
__global__ void __launch_bounds__(256) lfq_entropy_bwd_kernel(const float *__restrict__ v, int64_t v_rs, int64_t v_ss,
                                                              const int64_t *__restrict__ rows, int64_t rows_ss, int64_t R,
                                                              int C, int d, LfqCoef coefs, const float *__restrict__ w_ps,
                                                              const float *__restrict__ w_cb, float *__restrict__ gv,
                                                              int64_t gv_rs, int64_t gv_ss) {
    extern __shared__ float lfq_lds[];
    const LfqShape S = lfq_shape(d);
    const int t = blockIdx.y;
    const float coef = lfq_coef(coefs, t);
    v += (int64_t)t * v_ss;
    if (rows) rows += (int64_t)t * rows_ss;
    w_ps += t;
    w_cb += (int64_t)t * C * ((int64_t)1 << d);
    gv += (int64_t)t * gv_ss;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    const bool valid = task < R * C;
    const int64_t j = valid ? task / C : 0;
    const int c = valid ? (int)(task - j * C) : 0;
    const int64_t m = valid ? (rows ? rows[j] : j) : 0;
    float *lds = lfq_lds + wave * lfq_task_lds_floats(S);
    const float wps = w_ps[0];
    float h_i = 0.0f, lmax_i = 0.0f;
    const float z = lfq_build_tables(lds, S, v + m * v_rs + (int64_t)c * d, coef, valid, lane, &h_i, &lmax_i);
    if (!valid) return;
    const float *A = lds + 128, *LA = A + S.NA, *B = LA + S.NA, *LB = B + S.NB;
    const float *wc = w_cb + (int64_t)c * ((int64_t)1 << d);
    const int P = 1 << d;
    // the centring constants (see above)
    const float H = lfq_readfirstlane(lfq_wave_sum(h_i));
    const float lmax = lfq_readfirstlane(lfq_wave_sum(lmax_i));
    const float gclamp = -logf(kLfqEps) + 1.0f - H;  // G - (H - 1) below the clamp
    const float dlt = lfq_readfirstlane(lmax < logf(kLfqEps) ? gclamp : 0.0f);
    const float gcl = lfq_readfirstlane(gclamp - dlt);
    const unsigned long long pos = __ballot(lane < d && z > 0.0f);  // bit i: dim i of the most likely code
    const int km = (int)(__brevll(pos) >> (64 - d));
    const float wsamp = P >= 64 ? wc[lane * (P >> 6)] : (lane < P ? wc[lane] : 0.0f);
    const float wbar = lfq_readfirstlane(lfq_wave_sum(wsamp) * (P >= 64 ? 1.0f / 64.0f : 1.0f / (float)P));
    const float pm = expf(lmax);
    const float ccb = lfq_readfirstlane(pm * wc[km] + (1.0f - pm) * wbar);
    constexpr int kHi = kLfqMaxDim - 6;
    const int nhi = d > 6 ? d - 6 : 0;
    float s0 = 0.0f;
    float hi[kHi];
#pragma unroll
    for (int b = 0; b < kHi; ++b) hi[b] = 0.0f;
    for (int k = lane, s = 0; k < P; k += 64, ++s) {
        const int u = k >> S.l, w = k & (S.NB - 1);
        const float p = A[u] * B[w];
        const float G = p >= kLfqEps ? -(LA[u] + LB[w] + dlt) : gcl;
        const float t = fmaf(wps, G, wc[k] - ccb) * p;
        s0 += t;
#pragma unroll
        for (int b = 0; b < kHi; ++b)
            if (b < nhi && ((s >> b) & 1)) hi[b] += t;
    }
    // dim i is bit pos = d - 1 - i of k: pos < 6 -> the lane's own bit; pos >= 6 -> bit pos - 6 of s
    float mine = 0.0f;
    for (int i = 0; i < d; ++i) {
        const int pos = d - 1 - i;
        float si = 0.0f;
        if (pos < 6) {
            si = ((lane >> pos) & 1) ? s0 : 0.0f;
        } else {
#pragma unroll
            for (int b = 0; b < kHi; ++b)
                if (b == pos - 6) si = hi[b];
        }
        si = lfq_wave_sum(si);
        if (lane == i) mine = si;
    }
    const float S0 = lfq_wave_sum(s0);
    if (lane < d) {
        const float s1 = lds[lane];  // sigmoid(z_lane) = pi_lane(1)
        gv[m * gv_rs + (int64_t)c * d + lane] = coef * (mine - s1 * S0);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int lfq_task_waves(int d) { return d >= 19 ? 2 : 4; }  // 64 KiB of LDS per block at most

size_t lfq_block_lds_bytes(int d) { return (size_t)lfq_task_waves(d) * lfq_task_lds_floats(lfq_shape(d)) * sizeof(float); }

int64_t lfq_quant_blocks(int64_t N, int C) { return (N * C + kLfqQuantThreads - 1) / kLfqQuantThreads; }

// rows per split of the codebook-term sum: ~1024 blocks in all, at least 32 rows per split (fixed by (R, C, d) alone)
int64_t lfq_rows_per_split(int64_t R, int C, int d) {
    const int64_t ktiles = ((1 << d) + kLfqAvgCodes - 1) / kLfqAvgCodes;
    int64_t splits = (1024 + ktiles * C - 1) / (ktiles * C);
    const int64_t max_splits = (R + 31) / 32;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    return (R + splits - 1) / splits;
}

inline int64_t lfq_align(int64_t b) { return (b + 255) / 256 * 256; }

struct LfqWs {
    int64_t commit, ent, tabA, tabB, part, total;  // byte offsets
};

// T stages of R selected rows each (T = 1: a single-stage call)
LfqWs lfq_ws_layout(int64_t N, int64_t R, int C, int d, int64_t T = 1) {
    const LfqShape S = lfq_shape(d);
    const int64_t rps = lfq_rows_per_split(R > 0 ? R : 1, C, d);
    const int64_t splits = ((R > 0 ? R : 1) + rps - 1) / rps;
    LfqWs w;
    int64_t off = 0;
    w.commit = off;
    off += lfq_align(lfq_quant_blocks(N, C) * (int64_t)sizeof(double));
    w.ent = off;
    off += lfq_align(T * R * C * (int64_t)sizeof(float));
    w.tabA = off;
    off += lfq_align(T * R * C * S.NA * (int64_t)sizeof(float));
    w.tabB = off;
    off += lfq_align(T * R * C * S.NB * (int64_t)sizeof(float));
    w.part = off;
    off += lfq_align(T * splits * C * ((int64_t)1 << d) * (int64_t)sizeof(double));
    w.total = off;
    return w;
}

int lfq_check_shape(int64_t N, int C, int d) {
    if (N < 0 || C < 1) return fail(VQ_E_BADARG, "vq_lfq: N must be >= 0 and C >= 1");
    if (d < 1 || d > kLfqMaxDim) return fail(VQ_E_UNSUPPORTED, "vq_lfq: codebook_dim must be in [1, 20]");
    if (N * C > ((int64_t)1 << 40)) return fail(VQ_E_BADARG, "vq_lfq: too many rows");
    return 0;
}

// code_scale_dev (device, `period` values) for a staged call, else the host value *code_scale
LfqCoef lfq_coef_args(const float *code_scale, const float *code_scale_dev, int period, float inv_temperature) {
    LfqCoef k;
    k.four_tau = 4.0f * inv_temperature;
    k.coef0 = code_scale_dev ? 0.0f : 4.0f * inv_temperature * code_scale[0];
    k.code_scale = code_scale_dev;
    k.period = period;
    return k;
}

// The entropy forward of T stages (T = 1: vq_lfq_entropy_fwd_f32).  Stage t uses code_scale_dev[t % period] (a device
// array) or, when code_scale_dev is NULL, the host value code_scale[0].
int lfq_entropy_fwd_run(const float *v, int64_t v_rs, int64_t v_ss, const int64_t *rows, int64_t rows_ss, int64_t R, int T, int C,
                        int d, const float *code_scale, const float *code_scale_dev, int period, float inv_temperature, float *avg_prob,
                        double *per_sample_sum, void *workspace, int64_t workspace_bytes, void *stream, const char *who) {
    int rc = lfq_check_shape(R, C, d);
    if (rc) return rc;
    if (R < 1) return fail(VQ_E_BADARG, who, "no rows selected");
    if (T < 1 || T > 65535 || period < 1 || (!code_scale_dev && period != 1)) return fail(VQ_E_BADARG, who, "bad stage count");
    if (!v || !avg_prob || !per_sample_sum || !workspace || (!code_scale && !code_scale_dev)) return fail(VQ_E_BADARG, who, "null pointer");
    if (v_rs < (int64_t)C * d) return fail(VQ_E_BADARG, who, "row stride < C * d");
    const LfqWs ws = lfq_ws_layout(R, R, C, d, T);
    if (workspace_bytes < ws.total) return fail(VQ_E_BADARG, who, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)workspace;
    float *ent = (float *)(base + ws.ent), *tabA = (float *)(base + ws.tabA), *tabB = (float *)(base + ws.tabB);
    double *part = (double *)(base + ws.part);
    const LfqCoef coefs = lfq_coef_args(code_scale, code_scale_dev, period, inv_temperature);
    const int waves = lfq_task_waves(d);
    const int64_t tasks = R * C;
    rc = launch<lfq_entropy_fwd_kernel>(dim3((unsigned)((tasks + waves - 1) / waves), (unsigned)T), dim3(waves * 64),
                                        lfq_block_lds_bytes(d), s, who, v, v_rs, v_ss, rows, rows_ss, R, C, d, coefs, ent, tabA, tabB);
    if (rc) return rc;
    rc = launch<lfq_sum_kernel<float>>(dim3((unsigned)T), dim3(kLfqSumThreads), 0, s, who, ent, tasks, per_sample_sum, tasks);
    if (rc) return rc;
    const int64_t rps = lfq_rows_per_split(R, C, d);
    const int64_t splits = (R + rps - 1) / rps;
    const int P = 1 << d;
    rc = launch<lfq_avg_prob_kernel>(dim3((unsigned)((P + kLfqAvgCodes - 1) / kLfqAvgCodes), (unsigned)splits, (unsigned)(C * T)),
                                     dim3(kLfqAvgCodes), 0, s, who, tabA, tabB, R, C, d, rps, splits, part);
    if (rc) return rc;
    const int64_t CP = (int64_t)C * P;
    return launch<lfq_avg_reduce_kernel>(dim3((unsigned)((CP + 255) / 256), (unsigned)T), dim3(256), 0, s, who, part, (int)splits,
                                         CP, 1.0 / (double)R, avg_prob);
}

// The entropy backward of T stages (T = 1: vq_lfq_entropy_bwd_f32).
int lfq_entropy_bwd_run(const float *v, int64_t v_rs, int64_t v_ss, const int64_t *rows, int64_t rows_ss, int64_t R, int T, int C,
                        int d, const float *code_scale, const float *code_scale_dev, int period, float inv_temperature, const float *w_ps, const float *w_cb,
                        float *grad_v, int64_t gv_rs, int64_t gv_ss, void *stream, const char *who) {
    int rc = lfq_check_shape(R, C, d);
    if (rc) return rc;
    if (R == 0) return 0;
    if (T < 1 || T > 65535 || period < 1 || (!code_scale_dev && period != 1)) return fail(VQ_E_BADARG, who, "bad stage count");
    if (!v || !w_ps || !w_cb || !grad_v || (!code_scale && !code_scale_dev)) return fail(VQ_E_BADARG, who, "null pointer");
    if (v_rs < (int64_t)C * d || gv_rs < (int64_t)C * d) return fail(VQ_E_BADARG, who, "row stride < C * d");
    hipStream_t s = (hipStream_t)stream;
    const LfqCoef coefs = lfq_coef_args(code_scale, code_scale_dev, period, inv_temperature);
    const int waves = lfq_task_waves(d);
    const int64_t tasks = R * C;
    return launch<lfq_entropy_bwd_kernel>(dim3((unsigned)((tasks + waves - 1) / waves), (unsigned)T), dim3(waves * 64),
                                          lfq_block_lds_bytes(d), s, who, v, v_rs, v_ss, rows, rows_ss, R, C, d, coefs, w_ps, w_cb, grad_v,
                                          gv_rs, gv_ss);
}
