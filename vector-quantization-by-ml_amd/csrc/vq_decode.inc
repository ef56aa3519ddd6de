// vq_decode.inc -- indices -> code vectors for VectorQuantize / ResidualVQ / GroupedResidualVQ (vq_decode_f32): the gather of
// every stage's code and their left-to-right fp32 sum in one pass, nothing of [Q, N, D] unless the caller asks for it.
//
//   t_q             = valid(i_q) ? cb[g][q][i_q][:] : +0.0          i_q = idx[g][n][q]; stages q >= Q_given are dropped
//   all[q][g][n][:] = t_q                                            (bit copies of codebook rows, or +0.0)
//   sum[g][n][:]    = ((0 + t_0) + t_1) + ... + t_{Q-1}              (one IEEE fp32 add per stage, in stage order: the order of
//                                                                    the fused forward's `out`, vq_search.inc "fused finalize")
//
// Index rule (decode_code): drop_null = 1 is ResidualVQ's (any i < 0 is a dropped stage), drop_null = 0 is ATen's indexing
// (i in [-K, -1] wraps to i + K).  In both, an index outside the valid range NEVER becomes an address: the lane reads code 0
// of its stage (always there) and a select replaces what it read with +0.0 -- no multiply, so a NaN in code 0 cannot leak.
// Every load is therefore unconditional and the loads of a batch issue back to back (the gathers are latency-bound).
//
// Lane mapping of the vector kernel (D % 4 == 0, 16-byte aligned pointers and strides): one float4 per lane, LPR = the power of
// two >= D / 4 (at most 64) lanes per row, so a 64-lane access covers 64 / LPR rows (16 / 4 / 2 / 1 at D = 16 / 64 / 128 /
// 256); rows wider than 256 dims are cut into 256-dim slices, each slice of a row chunk a work unit of its own.  A wave owns
// NI such accesses x QB stages at a time: NI * QB index loads, then NI * QB gathers, then the adds and the stores.
// The scalar kernel (any D, any alignment, channel-first sums) is one thread per output element.

struct DecodeParams {
    const float *cb; long long cb_gs, cb_qs;
    int G, Q, K, D;
    const void *idx; int idx64; long long idx_gs, idx_rs, idx_qs;
    long long N;
    int Qg;         // stages the indices carry (1 <= Qg <= Q)
    int drop_null;
    float *sum; long long sum_gs, sum_rs, sum_ds;
    float *all; long long all_qs, all_gs, all_rs;
    int lpr_log2;   // vector kernel: log2 of the lanes per row (slice)
    int nslices;    //                256-dim slices per row (1 unless D > 256)
    long long chunks;  //             row chunks per group (a chunk = NI * 64 / LPR rows)
};

// the validated code index, or -1 for "contributes +0.0"
__device__ __forceinline__ int decode_code(long long v, int K, bool drop_null) {
    if (!drop_null && v < 0) v += K;
    return (v >= 0 && v < K) ? (int)v : -1;
}

__device__ __forceinline__ long long decode_load_index(const void *idx, bool idx64, long long at) {
    return idx64 ? ((const long long *)idx)[at] : (long long)((const int *)idx)[at];
}

template <int QB, int NI>
__global__ void __launch_bounds__(256) vq_decode_vec_kernel(const DecodeParams p) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const int rpi = 64 >> p.lpr_log2;                       // rows per 64-lane access
    const int sub = lane >> p.lpr_log2;                     // this lane's row within an access
    const int dlane = 4 * (lane & ((1 << p.lpr_log2) - 1));
    const long long units_per_group = p.chunks * p.nslices, units = units_per_group * p.G;
    const bool idx64 = p.idx64 != 0, drop_null = p.drop_null != 0;
    const int nq = p.all ? p.Q : p.Qg;                      // `all` holds zero rows for the stages the indices do not carry
    const f32x4 zero = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (long long u = wave; u < units; u += nwaves) {
        const long long g = u / units_per_group, rem = u - g * units_per_group;
        const long long chunk = rem / p.nslices;
        const int slice = (int)(rem - chunk * p.nslices);
        const int dl = slice * 256 + dlane;
        const bool dok = dl < p.D;                          // (D % 4 == 0: the whole float4 is inside the row)
        const float *cbg = p.cb + g * p.cb_gs + (dok ? dl : 0);
        long long n[NI];
        bool live[NI];
        f32x4 o[NI];
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const long long row = (chunk * NI + k) * rpi + sub;
            live[k] = dok && row < p.N;
            n[k] = row < p.N ? row : p.N - 1;               // clamp: duplicates are computed, not stored
            o[k] = zero;
        }
        for (int q0 = 0; q0 < nq; q0 += QB) {
            long long raw[QB][NI];
            f32x4 t[QB][NI];
#pragma unroll
            for (int kq = 0; kq < QB; ++kq) {
                const int q = q0 + kq < p.Qg ? q0 + kq : p.Qg - 1;  // clamp: stages past the end read a real index, unused
#pragma unroll
                for (int k = 0; k < NI; ++k) raw[kq][k] = decode_load_index(p.idx, idx64, g * p.idx_gs + n[k] * p.idx_rs + q * p.idx_qs);
            }
#pragma unroll
            for (int kq = 0; kq < QB; ++kq) {
                const int q = q0 + kq < p.Q ? q0 + kq : p.Q - 1;
                const bool carried = q0 + kq < p.Qg;
#pragma unroll
                for (int k = 0; k < NI; ++k) {
                    const int i = carried ? decode_code(raw[kq][k], p.K, drop_null) : -1;
                    const f32x4 c = *(const f32x4 *)(cbg + (long long)q * p.cb_qs + (long long)(i < 0 ? 0 : i) * p.D);
                    t[kq][k] = i < 0 ? zero : c;
                }
            }
#pragma unroll
            for (int kq = 0; kq < QB; ++kq) {
                if (q0 + kq < nq) {
#pragma unroll
                    for (int k = 0; k < NI; ++k) {
                        o[k] = o[k] + t[kq][k];
                        if (p.all && live[k])
                            __builtin_nontemporal_store(t[kq][k], (f32x4 *)(p.all + (long long)(q0 + kq) * p.all_qs + g * p.all_gs + n[k] * p.all_rs + dl));
                    }
                }
            }
        }
        if (p.sum) {
#pragma unroll
            for (int k = 0; k < NI; ++k)
                if (live[k]) __builtin_nontemporal_store(o[k], (f32x4 *)(p.sum + g * p.sum_gs + n[k] * p.sum_rs + dl));
        }
    }
}

// One thread per output element.  `rows_fastest`: consecutive lanes take consecutive rows (a channel-first sum is then written
// coalesced); otherwise consecutive dims of a row.
__global__ void __launch_bounds__(256) vq_decode_scalar_kernel(const DecodeParams p, int rows_fastest) {
    const long long per_group = p.N * p.D, total = per_group * p.G;
    const bool idx64 = p.idx64 != 0, drop_null = p.drop_null != 0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long g = e / per_group, rem = e - g * per_group;
        const long long n = rows_fastest ? rem % p.N : rem / p.D;
        const int d = (int)(rows_fastest ? rem / p.N : rem - n * p.D);
        const float *cbg = p.cb + g * p.cb_gs + d;
        float acc = 0.0f;
        for (int q = 0; q < p.Q; ++q) {
            int i = -1;
            if (q < p.Qg) i = decode_code(decode_load_index(p.idx, idx64, g * p.idx_gs + n * p.idx_rs + q * p.idx_qs), p.K, drop_null);
            const float c = cbg[(long long)q * p.cb_qs + (long long)(i < 0 ? 0 : i) * p.D];
            const float t = i < 0 ? 0.0f : c;
            acc = acc + t;
            if (p.all) p.all[(long long)q * p.all_qs + g * p.all_gs + n * p.all_rs + d] = t;
        }
        if (p.sum) p.sum[g * p.sum_gs + n * p.sum_rs + (long long)d * p.sum_ds] = acc;
    }
}

constexpr int kDecodeQB = 4;  // stages gathered together (a stack)
constexpr int kDecodeNI = 4;  // accesses in flight per stage (a stack); a single stage keeps 2 * kDecodeNI

// true when the vector kernel may take the call: float4 accesses on the codebooks and on every requested output
bool decode_vec_ok(const DecodeParams &p) {
    auto al = [](const void *q) { return ((uintptr_t)q & 15) == 0; };
    if (p.D % 4 || !al(p.cb) || p.cb_gs % 4 || p.cb_qs % 4) return false;
    if (p.sum && (p.sum_ds != 1 || !al(p.sum) || p.sum_gs % 4 || p.sum_rs % 4)) return false;
    if (p.all && (!al(p.all) || p.all_qs % 4 || p.all_gs % 4 || p.all_rs % 4)) return false;
    return true;
}

int decode_launch(DecodeParams &p, int cus, hipStream_t s) {
    const long long max_blocks = 8ll * (cus > 0 ? cus : 256);
    if (decode_vec_ok(p)) {
        const int d4 = p.D / 4;
        p.lpr_log2 = 0;
        while ((1 << p.lpr_log2) < d4 && p.lpr_log2 < 6) ++p.lpr_log2;
        p.nslices = (p.D + 255) / 256;
        const int ni = p.Qg == 1 && p.Q == 1 ? 2 * kDecodeNI : kDecodeNI;
        const long long rows_per_chunk = (long long)ni * (64 >> p.lpr_log2);
        p.chunks = (p.N + rows_per_chunk - 1) / rows_per_chunk;
        const long long units = p.chunks * p.nslices * p.G;
        long long blocks = (units + 3) / 4;
        if (blocks > max_blocks) blocks = max_blocks;
        if (ni == kDecodeNI) return launch<vq_decode_vec_kernel<kDecodeQB, kDecodeNI>>(dim3((unsigned)blocks), dim3(256), 0, s, "vq_decode launch", p);
        return launch<vq_decode_vec_kernel<1, 2 * kDecodeNI>>(dim3((unsigned)blocks), dim3(256), 0, s, "vq_decode launch", p);
    }
    const long long total = p.N * p.D * p.G;
    long long blocks = (total + 255) / 256;
    if (blocks > max_blocks) blocks = max_blocks;
    const int rows_fastest = (p.sum && p.sum_ds != 1 && p.sum_rs == 1) ? 1 : 0;
    return launch<vq_decode_scalar_kernel>(dim3((unsigned)blocks), dim3(256), 0, s, "vq_decode launch", p, rows_fastest);
}
