// vq_lfq_decode.inc -- indices -> code vectors for LFQ / ResidualLFQ / GroupedResidualLFQ (vq_lfq_decode_f32).  There is no
// table: a code is a function of the index bits alone, so the pass reads the indices and writes the codes, nothing else.
//
//   t_q[j]          = dropped(q) ? +0.0 : (bit d-1-j of i_q ? +mag[q] : -mag[q])    i_q = idx[g][n][q], MSB first: the modules'
//                                                                                   mask = 2 ** arange(d-1, -1, -1)
//   all[q][g][n][:] = t_q
//   sum[g][n][:]    = ((0 + t_0) + t_1) + ... + t_{Q-1}                             (one IEEE fp32 add per stage, in stage order)
//
// Only the low 32 bits of an int64 index carry bits (the modules' `.int()`), so any index value is valid and none becomes an
// address.  dropped(q): q >= Q_given, or drop_null and the index EQUAL to -1 (ResidualLFQ's `indices == -1`, taken on the whole
// int64 value); without drop_null a -1 is all bits set, the all-positive code.
//
// Lane mapping: one thread per float of a [G][N][d] result, consecutive lanes on consecutive dims of a row and then on the
// next row, so a wave's stores cover 64 consecutive floats where rows are dense, and the d lanes of a row load the same index
// words (one request).  A thread walks the stages kLfqDecodeQB at a time: the index loads of a batch issue together, then the
// selects, the adds and the stores.  The magnitudes travel by value in the kernel arguments.

constexpr int kLfqDecodeThreads = 256;
constexpr int kLfqDecodeQB = 8;  // index loads in flight per thread

struct LfqDecodeParams {
    const void *idx; int idx64; long long idx_gs, idx_rs, idx_qs;
    long long N;
    int Q, Qg, d, drop_null;
    float *sum; long long sum_gs, sum_rs, sum_ds;
    float *all; long long all_qs, all_gs, all_rs;
    float mag[VQ_RLFQ_MAX_STAGES];
};

__global__ void __launch_bounds__(kLfqDecodeThreads) vq_lfq_decode_kernel(const LfqDecodeParams p) {
    const long long e = (long long)blockIdx.x * kLfqDecodeThreads + threadIdx.x;  // element of group g's [N][d]
    if (e >= p.N * p.d) return;
    const long long g = blockIdx.y;
    // (a 32-bit division where the element number allows it: the 64-bit one is a long software sequence)
    const long long n = e <= 0x7fffffffll ? (long long)((unsigned)e / (unsigned)p.d) : e / p.d;
    const int j = (int)(e - n * p.d);
    const int shift = p.d - 1 - j;
    const bool idx64 = p.idx64 != 0, drop_null = p.drop_null != 0;
    const long long at = g * p.idx_gs + n * p.idx_rs;
    const int nq = p.all ? p.Q : p.Qg;  // `all` holds zero rows for the stages the indices do not carry
    float *all = p.all ? p.all + g * p.all_gs + n * p.all_rs + j : nullptr;
    float acc = 0.0f;
    for (int q0 = 0; q0 < nq; q0 += kLfqDecodeQB) {
        long long raw[kLfqDecodeQB];
#pragma unroll
        for (int k = 0; k < kLfqDecodeQB; ++k) {
            const int q = q0 + k < p.Qg ? q0 + k : p.Qg - 1;  // clamp: stages past the end read a real index, unused
            raw[k] = idx64 ? ((const long long *)p.idx)[at + q * p.idx_qs] : (long long)((const int *)p.idx)[at + q * p.idx_qs];
        }
#pragma unroll
        for (int k = 0; k < kLfqDecodeQB; ++k) {
            const int q = q0 + k;
            if (q < nq) {
                const bool dropped = q >= p.Qg || (drop_null && raw[k] == -1);
                const float m = p.mag[q];
                const float t = dropped ? 0.0f : ((((unsigned)raw[k] >> shift) & 1u) ? m : -m);
                acc = acc + t;
                if (all) all[(long long)q * p.all_qs] = t;
            }
        }
    }
    if (p.sum) p.sum[g * p.sum_gs + n * p.sum_rs + (long long)j * p.sum_ds] = acc;
}

inline long long lfq_decode_blocks(long long N, int d) { return (N * d + kLfqDecodeThreads - 1) / kLfqDecodeThreads; }

int lfq_decode_launch(const LfqDecodeParams &p, int G, hipStream_t s) {
    return launch<vq_lfq_decode_kernel>(dim3((unsigned)lfq_decode_blocks(p.N, p.d), (unsigned)G), dim3(kLfqDecodeThreads), 0, s,
                                        "vq_lfq_decode launch", p);
}
