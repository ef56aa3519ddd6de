// vq_sample.inc -- counter-based Gumbel noise for Gumbel-max code sampling (utils/general.py:112-129:
// ind = argmax(similarities / temperature + gumbel_noise)).  Included by vq_kernels.hip in front of vq_similarity.inc, whose
// kAuxSample epilogue is the one product user of gumbel_noise4; the element-per-thread kernel below writes the same noise to
// memory so that tests can check a random kernel exactly.
// ------------------------------------------------------------------------------------------------
// The noise of entry (head, row, code) is a function of (seed, head, row, code) ONLY -- never of grid, wave, tile or chunk
// geometry.  Philox4x32-10 (Salmon et al., SC'11), one call per group of 4 consecutive codes 4 * (code >> 2) .. + 3:
//   key      k0 = seed[0] bits 31..0        k1 = seed[0] bits 63..32
//   counter  c0 = row bits 31..0            c1 = row bits 63..32                       (the row keeps all 64 bits)
//            (c3 : c2) = ((head << 32) | (code >> 2)) + seed[1]   (mod 2^64; c2 the low word)
//   word e of the output belongs to code 4 * (code >> 2) + e:
//   u = (word >> 8) * 2^-24  in [0, 1)      g = -log(max(-log(max(u, 1e-5)), 1e-5))    (the two clamps of utils/general.py:25-30)
// Accuracy of g against the fp64 transform of the same word: the outer logarithm is the native v_log_f32 (argument in
// [1e-5, 11.6]: absolute error ~1e-6); the inner one decides g's ABSOLUTE error through its RELATIVE one (g = -log t), which
// the native instruction does not bound for u -> 1, so for 1 - u < 2^-6 it is the series  d + d^2/2 + d^3/3 + d^4/4,
// d = 1 - u exact (truncation < d^4 / 5 = 1.2e-8 relative).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;  // (one v_mad_u64_u32 gives both halves)
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        c0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        c1 = (unsigned)p1;
        c2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c3 = (unsigned)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ float gumbel_of_word(unsigned word) {
    constexpr float LN2 = 0.69314718055994531f;
    const float u = fmaxf((float)(word >> 8) * 0x1p-24f, 1e-5f);
    const float d = 1.0f - u;  // exact from u >= 0.5 on
    const float series = d * fmaf(d, fmaf(d, fmaf(d, 0.25f, 0.33333333333f), 0.5f), 1.0f);
    const float t = fmaxf(d < 0x1p-6f ? series : -LN2 * __log2f(u), 1e-5f);
    return -LN2 * __log2f(t);
}

// seed0 / seed1: the two seed words; -> the noise of codes 4 * code_group .. + 3 of (head, row); `raw`: also the Philox words
__device__ __forceinline__ f32x4 gumbel_noise4(unsigned long long seed0, unsigned long long seed1, int head, long long row,
                                               int code_group, unsigned *raw = nullptr) {
    const unsigned long long hi = (((unsigned long long)(unsigned)head << 32) | (unsigned long long)(unsigned)code_group) + seed1;
    unsigned w[4];
    philox4x32_10((unsigned)(unsigned long long)row, (unsigned)((unsigned long long)row >> 32), (unsigned)hi, (unsigned)(hi >> 32),
                  (unsigned)seed0, (unsigned)(seed0 >> 32), w);
    if (raw) {
        raw[0] = w[0]; raw[1] = w[1]; raw[2] = w[2]; raw[3] = w[3];
    }
    return (f32x4){gumbel_of_word(w[0]), gumbel_of_word(w[1]), gumbel_of_word(w[2]), gumbel_of_word(w[3])};
}

#if VQ_OWN(0)
// noise[h][m][k] (and the raw Philox word of every entry), one entry per thread: the test hook, not a product path
__global__ void __launch_bounds__(256) vq_gumbel_noise_kernel(const long long *seed, int H, long long M, int K, float *noise,
                                                              unsigned *bits) {
    const unsigned long long seed0 = (unsigned long long)seed[0], seed1 = (unsigned long long)seed[1];
    const long long n = (long long)H * M * K;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int k = (int)(i % K);
        const long long hm = i / K;
        unsigned raw[4];
        const f32x4 g = gumbel_noise4(seed0, seed1, (int)(hm / M), hm % M, k >> 2, raw);
        const int e = k & 3;
        noise[i] = e == 0 ? g.x : e == 1 ? g.y : e == 2 ? g.z : g.w;
        if (bits) bits[i] = e == 0 ? raw[0] : e == 1 ? raw[1] : e == 2 ? raw[2] : raw[3];
    }
}
#endif
