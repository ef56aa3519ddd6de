// vq_diversity.inc -- the codebook diversity loss (vector_quantize_pytorch.py:324-334, utils/general.py:25-30) without [M, K]:
// what is not a role of vq_gumbel_sweep.  Included by vq_kernels.hip (build part 0, after vq_gumbel.inc).
// ------------------------------------------------------------------------------------------------
//   s = similarities [H, M, K]   z = -T s   p = softmax_k(z)   n(m) = (m / pos_div) % N   C = H M / N rows per position
//   A_nk = (1 / C) sum_{h, m : n(m) = n} p_hmk         loss = (1 / N) sum_nk A_nk log(max(A_nk, 1e-5))
//   U_nk = g / (N C) (log(max(A_nk, 1e-5)) + [A_nk >= 1e-5])      delta_m = sum_k p_mk U[n(m)][k]
//   w_mk = dL/ds_mk = -T p_mk (U[n(m)][k] - delta_m), then through the similarities as in vq_gumbel.inc
// Sweeps (roles of vq_gumbel_sweep with tau = -T, see there): kDivStats -> lse2;  vq_gumbel_pack_rows with a RowMap, kDivAcc
// -> one partial of A per head, added here in head order;  kDivDelta -> delta;  kDivX -> grad_x.  loss and U are [N, K]
// element-wise work and stay with the caller.
// ------------------------------------------------------------------------------------------------

// A[n][k] = (parts[0][n][k] + parts[1][n][k] + ...) / count in head order, i over [N][stride]; 0 in the padding past K
__global__ void __launch_bounds__(256) vq_diversity_reduce_heads(const float *__restrict__ parts, long long n, long long stride, int K, int H,
                                                                 float count, float *__restrict__ A) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i % stride >= K) {
        A[i] = 0.0f;
        return;
    }
    float s = parts[i];
    for (int h = 1; h < H; ++h) s += parts[(long long)h * n + i];
    A[i] = s / count;
}
