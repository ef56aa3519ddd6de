"""Plain numpy models of the training-side kernels of csrc/vq_finalize_ema.inc, their error bounds and the inputs the
tests feed them (test helper; CPU only, imports neither oracle/ nor the reference).

  quantize_backward_model   vq_quantize_backward_kernel    gx = (ste ? Q go : 0) + sum_q 2 ge[q] (r_q - c_q)
  ema_update_model          vq_ema_sizes_kernel + vq_ema_codes_kernel   lerp / Laplace smoothing / optional l2norm
  residual_stats_model      vq_ema_accumulate_residual_kernel           per-stage counts and sums of the residual chain
  accumulate_model          vq_ema_accumulate_kernel, vq_ema_accumulate_owner_kernel + vq_ema_reduce_parts_kernel
                                                                        counts and sums of the rows of each code

The residual chain r_0 = x, quant = ste ? r + (c - r) : c, r <- r - quant is elementwise IEEE add / sub: there is nothing a
compiler can contract, so the fp32 chain computed here is the chain on the device bit for bit.  Everything after the chain
is evaluated in fp64 from those fp32 values.

Error bounds.  u = 2^-24 is the unit roundoff of fp32; every bound counts the fp32 roundings of the kernel's arithmetic and
doubles the count.  None of them is fitted to a measurement.

  backward.  Per element the kernel rounds Q * go once, and per stage r - c once, float(2 ge[q]) once and their product once:
    every term t of g = Q go + sum_q 2 ge[q] (r_q - c_q) is off by at most 3u |t| (1 + O(u)).  The Q accumulations
    (Q + 1 with the first one into 0, which is exact) each add at most u times the partial sum, itself at most
    S = |Q go| + sum_q |2 ge[q]| |r_q - c_q|.  Together (Q + 4) u S; an fma only removes roundings.  Doubled and rounded up:
        |got - g| <= (Q + 5) 2^-23 S.
    (The go term enters S only when the kernel reads go: ste on and grad_out given.)
  cluster_size.  cs' = old + w (counts - old): a subtraction, a product, an addition, each at most u times a magnitude that
    A_cs = |old| + w |counts - old| bounds: 3u A_cs (1 + O(u)) <= 4u A_cs, doubled:  2^-21 A_cs.
  embed_avg.  The same expression over embed_avg and sums:  2^-21 A_avg.
  embeddings, no l2norm.  e = avg' / sm with sm = (cs' + eps) / (tot + K eps) * tot.  The error of avg' passes through the
    division as tol_avg / sm; the relative error of sm and the division's own rounding scale |e|:
        tol_e = tol_avg / sm + |e| rel_s,    rel_s = tol_cs / (cs' + eps) + (2 ceil(K / 256) + 32) u.
    rel_s: the error of cs' relative to cs' + eps; tot is a sum of non-negative numbers, ceil(K / 256) serial additions per
    thread and 8 tree levels, and d sm / d tot is at most sm / tot, so ceil(K / 256) + 8 roundings; (float)K * eps, the two
    additions, the division, the product and e's division are 6 more; the counted ceil(K / 256) + 14 are covered twice by
    2 ceil(K / 256) + 32 (the four spare u absorb the second-order terms).
  embeddings, l2norm.  e^ = e / max(|e|_2, 1e-12).  With n = |e|_2:  d e^_i = d e_i / n - e^_i (e . d e) / n^2, so
        tol = tol_e / n + |e^| (sum_d |e_d| tol_e_d / n^2 + (D / 64 + 16) u),
    where the last term counts the kernel's own work on the norm: ceil(D / 64) fmaf steps per lane and 6 butterfly steps on
    the sum of squares (halved by the square root), then sqrtf, the reciprocal and the product: at most
    (D / 64 + 7) / 2 + 3 roundings, doubled D / 64 + 13 <= D / 64 + 16.  The same count bounds how far the fp64 norm of a
    stored row is from 1.
  residual sums.  A code's sum is n_k fp32 additions (atomics in any order, or the owner kernel's partial sums plus their
    fixed-order reduction: never more than n_k additions touch a value, the one into 0 being exact); each is off by at
    most u times a partial sum of at most sum |terms| (1 + O(n u)):  n_k 2^-23 sum |terms|, in any order.
  accumulated sums (accumulate_model: vq_ema_accumulate_kernel, vq_ema_accumulate_owner_kernel and
    vq_ema_reduce_parts_kernel).  The same bound, counted per kernel.  Let code k have n_k rows, n_b of them in row block b,
    B row blocks non-empty.  Inside a block its partial sum is n_b additions, the first one into 0 (exact): n_b - 1
    roundings, whether a wave adds its queued rows into its LDS table or (one block, B = 1, n_b = n_k) the rows arrive as
    float atomics in any order.  Merging the B partials -- atomics into the zeroed output, or the fixed-order reduction,
    whose first addition is again into 0 -- rounds B - 1 times.  sum_b (n_b - 1) + B - 1 = n_k - 1 roundings in all, each
    at most u times a partial sum of at most sum |terms| (1 + O(n u)); doubled and rounded up to n_k this is
    residual_sums_bound, in any order, for all three kernels.  (Output that was not zero before the call adds one more
    addition; the tests of the += contract use exact data.)
  exact data (exact_inputs).  Rows are integers in [-15, 15] times 2^-3, so every partial sum of at most M <= 2^20 of them
    is an integer below 2^24 times 2^-3: representable, every fp32 addition exact, in any order and any blocking.  On such
    data all three kernels must return the integer model bit for bit, and an empty code +0.0.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
F32 = np.float32
CLAMP = float(F32(1e-12))  # the kernel's 1e-12f


def _np32(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=F32)


def _idx(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.int64)


# ------------------------------------------------------------------------------------------------
# residual chain
# ------------------------------------------------------------------------------------------------
def residual_chain(x, cb, idx, *, ste, share, dtype=F32):
    """x [H, M, D], cb [H, Q | 1, K, D], idx [H, M, Q] -> list over q of (r_q, c_q, live_q): the residual stage q quantized,
    the code it picked (zeros on rows that are not live) and the rows whose chain has not ended (first idx < 0 ends it).
    Computed in `dtype` (fp32: the device's chain bit for bit)."""
    x, cb, idx = _np32(x).astype(dtype), _np32(cb).astype(dtype), _idx(idx)
    H, M, D = x.shape
    Q = idx.shape[-1]
    harange = np.arange(H)[:, None]
    r = x.copy()
    live = np.ones((H, M), dtype=bool)
    stages = []
    for q in range(Q):
        iq = idx[..., q]
        live = live & (iq >= 0)
        c = cb[:, 0 if share else q][harange, np.where(live, iq, 0)]  # [H, M, D]
        c = np.where(live[..., None], c, dtype(0))
        stages.append((r.copy(), c, live.copy()))
        quant = r + (c - r) if ste else c
        r = np.where(live[..., None], r - quant, r)
    return stages


# ------------------------------------------------------------------------------------------------
# quantize backward
# ------------------------------------------------------------------------------------------------
def quantize_backward_model(x, cb, idx, go, ge, *, ste, share, per_head, chain_dtype=F32, factor=2.0, ge_stage0=False):
    """-> (g, S) fp64 [H, M, D]: the gradient and the magnitude sum its error bound scales with.  ge: [Q] (or [H, Q] with
    per_head) fp64 or None.  `factor` and `ge_stage0` build deliberately wrong models (tests of the bound's bite)."""
    idx = _idx(idx)
    H, M, Q = idx.shape
    stages = residual_chain(x, cb, idx, ste=ste, share=share, dtype=chain_dtype)
    D = stages[0][0].shape[-1]
    g = np.zeros((H, M, D), dtype=np.float64)
    S = np.zeros((H, M, D), dtype=np.float64)
    if ste and go is not None:
        g += float(Q) * _np32(go).astype(np.float64)
        S += np.abs(g)
    if ge is not None:
        ge = np.asarray(ge.detach().cpu().numpy() if isinstance(ge, torch.Tensor) else ge, dtype=np.float64)
        ge = ge.reshape(H, Q) if per_head else np.broadcast_to(ge.reshape(1, Q), (H, Q))
        for q, (r, c, _live) in enumerate(stages):
            coef = factor * ge[:, 0 if ge_stage0 else q][:, None, None]
            diff = r.astype(np.float64) - c.astype(np.float64)
            g += coef * diff
            S += np.abs(coef) * np.abs(diff)
    return g, S


def quantize_backward_bound(S, Q):
    return (Q + 5) * 2.0 ** -23 * S


def backward_inputs(H, M, D, Q, K, seed, *, per_head=False, share=False):
    """CPU tensors of one backward case: x, go ~ N(0, 1), codebooks ~ 0.5 N(0, 1), indices from torch.randint (the kernel does
    not care whether they are winners), g_err of order 0.1 - 1 with both signs so the loss term matches the ste term."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((H, M, D), generator=g)
    cb = torch.randn((H, 1 if share else Q, K, D), generator=g) * 0.5
    idx = torch.randint(0, K, (H, M, Q), generator=g)
    go = torch.randn((H, M, D), generator=g)
    ge = (0.1 + 0.9 * torch.rand((H, Q) if per_head else (Q,), generator=g, dtype=torch.float64))
    ge = ge * torch.where(torch.rand(ge.shape, generator=g) < 0.3, -1.0, 1.0).double()
    return x, cb, idx, go, ge


BWD_DIMS = (1, 3, 4, 63, 64, 65, 130, 252, 256, 260, 512, 1028)
BWD_STAGES = (1, 2, 5)
BWD_M, BWD_K = 37, 11  # 10 workgroups of 4 rows, the last one ragged


def backward_cases():
    """D x Q x H x ste thinned to 108 cases: every one at H = 1, every other one (a checkerboard) at H = 3.
    H = 3 uses a g_err row per head unless Q = 2 (one shared row: head stride 0)."""
    cases = []
    for i, D in enumerate(BWD_DIMS):
        for j, Q in enumerate(BWD_STAGES):
            for H in (1, 3):
                for ste in (True, False):
                    if H == 3 and (i + j + int(ste)) % 2:
                        continue
                    cases.append((D, Q, H, ste, H == 3 and Q != 2))
    return cases


def backward_case_inputs(D, Q, H, ste, per_head):
    seed = 1000 + D * 16 + Q * 4 + H + int(ste)
    return backward_inputs(H, BWD_M, D, Q, BWD_K, seed, per_head=per_head)


# ------------------------------------------------------------------------------------------------
# EMA update
# ------------------------------------------------------------------------------------------------
def ema_update_model(cluster_size, embed_avg, counts, sums, decay, eps, l2norm, *, laplace=True, total_head0=False,
                     clamp=True):
    """fp64 evaluation of the EMA step from the fp32 inputs ([H, K], [H, K, D], [H, K], [H, K, D]) with the kernel's weight
    w = float32(1.0 - decay) (the subtraction in double, as the reference's lerp_(.., 1 - decay)) and eps = float32(eps).  -> dict(cs, avg, emb, e, tot, sm, A_cs, A_avg), e the
    embeddings before the l2norm.  `laplace`, `total_head0`, `clamp` build deliberately wrong models."""
    old, avg0 = _np32(cluster_size).astype(np.float64), _np32(embed_avg).astype(np.float64)
    cnt, sm_in = _np32(counts).astype(np.float64), _np32(sums).astype(np.float64)
    K = old.shape[-1]
    w = float(F32(1.0 - float(decay)))
    eps = float(F32(eps))
    cs = old + w * (cnt - old)
    A_cs = np.abs(old) + w * np.abs(cnt - old)
    tot = cs.sum(-1, keepdims=True)
    if total_head0:
        tot = np.broadcast_to(tot[:1], tot.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        sm = (cs + eps) / (tot + (K * eps if laplace else 0.0)) * tot
        avg = avg0 + w * (sm_in - avg0)
        A_avg = np.abs(avg0) + w * np.abs(sm_in - avg0)
        e = avg / sm[..., None]
        emb = e
        if l2norm:
            n = np.sqrt((e * e).sum(-1, keepdims=True))
            emb = e / (np.maximum(n, CLAMP) if clamp else n)
    return dict(cs=cs, avg=avg, emb=emb, e=e, tot=tot, sm=sm, A_cs=A_cs, A_avg=A_avg, eps=eps)


def ema_update_bounds(m, K, D, l2norm):
    """m: ema_update_model's result -> (tol_cs, tol_avg, tol_emb), elementwise."""
    tol_cs = 2.0 ** -21 * m["A_cs"]
    tol_avg = 2.0 ** -21 * m["A_avg"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_s = tol_cs / (m["cs"] + m["eps"]) + (2 * math.ceil(K / 256) + 32) * U
        tol_e = tol_avg / m["sm"][..., None] + np.abs(m["e"]) * rel_s[..., None]
        if l2norm:
            e = m["e"]
            n = np.maximum(np.sqrt((e * e).sum(-1, keepdims=True)), CLAMP)
            tol_e = tol_e / n + np.abs(m["emb"]) * ((np.abs(e) * tol_e).sum(-1, keepdims=True) / n ** 2 + (D / 64 + 16) * U)
    return tol_cs, tol_avg, tol_e


EMA_SHAPES = ((1, 1, 1), (1, 7, 5), (3, 7, 64), (2, 33, 65), (1, 256, 16), (3, 257, 100), (2, 1030, 8), (1, 301, 600),
              (1, 5000, 4))
EMA_DECAYS = (0.5, 0.8, 0.99)
EMA_EPS = 1e-5


def ema_inputs(H, K, D, seed, *, rate=3.0, size_scale=5.0):
    """CPU tensors (cluster_size, embed_avg, counts, sums): Poisson counts with every fifth one 0, old sizes with every tenth
    one 0 (codes 0, 10, 20 .. have both: dead codes), sums and embed_avg scaled by them (a dead code's rows are 0).
    K = 1 keeps its only code alive: a head with nothing but dead codes has total 0 and embeddings 0 / 0 (that edge is
    ema_isolation_inputs')."""
    rng = np.random.default_rng(seed)
    counts = rng.poisson(rate, (H, K)).astype(F32)
    old = (rng.random((H, K)) * size_scale).astype(F32)
    if K > 1:
        counts[:, ::5] = 0
        old[:, ::10] = 0
    # (+ 0: x * 0 is -0 for x < 0, and old + w (new - old) turns a -0 into +0 at any weight, as the reference's lerp_ does)
    sums = (rng.standard_normal((H, K, D)) * counts[..., None]).astype(F32) + F32(0)
    avg = (rng.standard_normal((H, K, D)) * old[..., None]).astype(F32) + F32(0)
    return tuple(torch.from_numpy(a) for a in (old, avg, counts, sums))


def ema_case_inputs(H, K, D):
    """The inputs of one EMA shape.  K = 5000 is the Laplace case: about 50 hits in all and old sizes to match, so that
    K eps / total >= 1e-3 (asserted by the tests that use it)."""
    seed = 7000 + H * 100000 + K * 16 + D
    if K == 5000:
        return ema_inputs(H, K, D, seed, rate=0.01, size_scale=0.01)
    return ema_inputs(H, K, D, seed)


def ema_laplace_heads_inputs():
    """H = 2, K = 3000, D = 4: about 30 hits in head 0 and 90 in head 1, so K eps / total is 1e-3 and 3e-4: the two heads'
    Laplace terms differ by far more than the tolerance, which makes the head a row's total is read from visible."""
    a = ema_inputs(1, 3000, 4, 7101, rate=0.01, size_scale=0.01)
    b = ema_inputs(1, 3000, 4, 7102, rate=0.03, size_scale=0.03)
    return tuple(torch.cat([s, t]) for s, t in zip(a, b))


def ema_isolation_inputs(empty_head):
    """H = 2, K = 33, D = 5: `empty_head` has zero counts and zero old sizes (its total is 0, its smoothed sizes 0, its
    embeddings x / 0) but non-zero embed_avg / sums with some zero rows and elements; the other head is ordinary."""
    old, avg, counts, sums = ema_inputs(2, 33, 5, 7200 + empty_head)
    rng = np.random.default_rng(7210 + empty_head)
    a = rng.standard_normal((33, 5)).astype(F32)
    s_ = rng.standard_normal((33, 5)).astype(F32)
    a[::4] = 0
    s_[::4] = 0  # rows 0, 4, 8 ..: 0 / 0
    a[1, 2] = s_[1, 2] = 0  # a zero among non-zeros
    old[empty_head] = 0
    counts[empty_head] = 0
    avg[empty_head] = torch.from_numpy(a)
    sums[empty_head] = torch.from_numpy(s_)
    return old, avg, counts, sums


# ------------------------------------------------------------------------------------------------
# residual EMA statistics
# ------------------------------------------------------------------------------------------------
def residual_stats_model(x, cb, idx, *, ste, share):
    """-> (counts [H, Q, K] int64, sums [H, Q, K, D] fp64, abs_sums [H, Q, K, D] fp64) of the fp32 residual each stage
    quantized; a row's chain ends at its first idx < 0."""
    idx = _idx(idx)
    H, M, Q = idx.shape
    K = cb.shape[2]
    stages = residual_chain(x, cb, idx, ste=ste, share=share)
    D = stages[0][0].shape[-1]
    counts = np.zeros((H, Q, K), dtype=np.int64)
    sums = np.zeros((H, Q, K, D), dtype=np.float64)
    abs_sums = np.zeros((H, Q, K, D), dtype=np.float64)
    for q, (r, _c, live) in enumerate(stages):
        for h in range(H):
            rows = np.nonzero(live[h])[0]
            k = idx[h, rows, q]
            np.add.at(counts[h, q], k, 1)
            r64 = r[h, rows].astype(np.float64)
            np.add.at(sums[h, q], k, r64)
            np.add.at(abs_sums[h, q], k, np.abs(r64))
    return counts, sums, abs_sums


def residual_sums_bound(counts, abs_sums):
    return counts[..., None].astype(np.float64) * 2.0 ** -23 * abs_sums


def residual_inputs(H, M, D, Q, K, seed, *, share, drop=True):
    """x ~ N(0, 1), codebooks ~ 0.5 N(0, 1), random indices; about a third of the rows are dropped from a random stage
    (0 included) onward: idx = -1 for that stage and every later one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((H, M, D), generator=g)
    cb = torch.randn((H, 1 if share else Q, K, D), generator=g) * 0.5
    idx = torch.randint(0, K, (H, M, Q), generator=g)
    if drop:
        dropped = torch.rand((H, M), generator=g) < 1.0 / 3.0
        first = torch.randint(0, Q, (H, M), generator=g)
        gone = dropped[..., None] & (torch.arange(Q)[None, None, :] >= first[..., None])
        idx = torch.where(gone, torch.full_like(idx, -1), idx)
    return x, cb, idx


# ------------------------------------------------------------------------------------------------
# EMA accumulation (the scatter-add)
# ------------------------------------------------------------------------------------------------
def _scatter_rows(vals, k, K):
    """vals fp64 [n, D], k [n] in [0, K) -> [K, D]: the rows of each code added up in fp64, in row order."""
    out = np.zeros((K, vals.shape[1]), dtype=np.float64)
    if k.size:
        order = np.argsort(k, kind="stable")
        ks = k[order]
        starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        with np.errstate(invalid="ignore"):  # (inf - inf of the non-finite inputs)
            out[ks[starts]] = np.add.reduceat(vals[order], starts, axis=0)
    return out


def accumulate_model(x, idx, mask, K):
    """x [H, M, D] fp32, idx [H, M], mask [H, M] or None -> (counts int64 [H, K], sums fp64 [H, K, D], abs_sums fp64
    [H, K, D]).  A row contributes when its mask byte is non-zero (or there is no mask) and 0 <= idx < K."""
    x, idx = _np32(x), _idx(idx)
    H, M, D = x.shape
    assert idx.shape == (H, M)
    keep = (idx >= 0) & (idx < K)
    if mask is not None:
        m = np.asarray(mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else mask)
        assert m.shape == (H, M)
        keep &= m != 0
    counts = np.zeros((H, K), dtype=np.int64)
    sums = np.zeros((H, K, D), dtype=np.float64)
    abs_sums = np.zeros((H, K, D), dtype=np.float64)
    for h in range(H):
        rows = np.flatnonzero(keep[h])
        k = idx[h, rows]
        counts[h] = np.bincount(k, minlength=K)
        v = x[h, rows].astype(np.float64)
        sums[h] = _scatter_rows(v, k, K)
        abs_sums[h] = _scatter_rows(np.abs(v), k, K)
    return counts, sums, abs_sums


# (H, M, K, D): what each shape is for is told where the GPU tests use them (tests/test_gpu_ema_accumulate.py)
ACC_SHAPES = (
    (1, 1024, 8, 32), (1, 1023, 8, 32), (1, 5000, 3, 4), (2, 4500, 70, 20), (1, 3000, 40, 5), (1, 2048, 1, 64),
    (1, 2100, 2, 256), (1, 2100, 2, 257), (1, 2100, 2, 260), (1, 2100, 2, 512), (1, 3100, 7, 600), (1, 2100, 2, 2048),
    (1, 2100, 2, 2052), (1, 37, 5, 3), (2, 1000, 256, 64), (1, 300, 8192, 16), (1, 1, 4, 8), (1, 0, 4, 8),
)
ACC_PATTERNS = ("uniform", "one_code", "last_code", "half_empty", "runs")
ACC_MASK_SHAPES = ((2, 4500, 70, 20), (1, 3000, 40, 5))
# owner path, atomic path, and cw = 64 with K = 70 inside the last owner's range [64, 128)
ACC_RANGE_SHAPES = ((1, 3000, 40, 5), (2, 1000, 256, 64), (2, 4500, 70, 20))
ACC_NONFINITE_SHAPES = ((1, 3000, 40, 5), (2, 1000, 256, 64))  # owner path, atomic path
ACC_ROWS_PER_BLOCK = 2048  # the owner kernel's row block at these sizes (ema_owner_plan: at least 2048 rows per block)


def acc_seed(H, M, K, D):
    return 9000 + H * 1000003 + M * 4099 + K * 131 + D


def _acc_indices(rng, H, M, K, pattern):
    if pattern == "uniform":
        return rng.integers(0, K, (H, M))
    if pattern == "one_code":
        return np.zeros((H, M), dtype=np.int64)
    if pattern == "last_code":
        return np.full((H, M), K - 1, dtype=np.int64)
    if pattern == "half_empty":
        return 2 * rng.integers(0, (K + 1) // 2, (H, M))
    if pattern == "runs":
        return np.repeat(rng.integers(0, K, (H, (M + 63) // 64)), 64, axis=1)[:, :M]
    raise ValueError(pattern)


def exact_inputs(H, M, K, D, seed, pattern):
    """-> (x [H, M, D] fp32, idx [H, M] int64) CPU tensors: rows of integers in [-15, 15] times 2^-3, whose sums are exact in
    fp32 in any order (module docstring), and one of ACC_PATTERNS: uniform / one_code (every row to code 0) / last_code
    (every row to K - 1) / half_empty (odd codes never hit) / runs (64 consecutive rows share a code: a whole scan group
    of the owner kernel belongs to one owner, the next group to none of its codes)."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-15, 16, (H, M, D)).astype(F32) * F32(0.125)).astype(F32)
    idx = _acc_indices(rng, H, M, K, pattern).astype(np.int64).reshape(H, M)
    return torch.from_numpy(x), torch.from_numpy(idx)


def float_inputs(H, M, K, D, seed):
    """-> (x, idx): randn rows with a power-of-two scale per column, 2^-20 .. 2^20 (column d: 2^(-20 + 17 d mod 41), the
    last column 2^20), uniform indices; for the codes with k % 4 == 1 the rows come in pairs v, -v (1 - 2^-10 t), t uniform
    in [-1, 1] (an odd row out is scaled by 2^-10), so that those sums are about 2^-10 of sum |terms|."""
    rng = np.random.default_rng(seed)
    e = -20 + (17 * np.arange(D)) % 41
    if D > 1:
        e[-1] = 20
    x = (rng.standard_normal((H, M, D)) * np.exp2(e)).astype(F32)
    idx = rng.integers(0, K, (H, M)).astype(np.int64).reshape(H, M)
    for h in range(H):
        for k in range(1, K, 4):
            rows = np.flatnonzero(idx[h] == k)
            a, b = rows[0:len(rows) // 2 * 2:2], rows[1::2]
            t = rng.uniform(-1.0, 1.0, (len(a), D))
            x[h, b] = (-x[h, a].astype(np.float64) * (1.0 - 2.0 ** -10 * t)).astype(F32)
            x[h, rows[len(a) + len(b):]] *= F32(2.0 ** -10)  # (the odd row out)
    return torch.from_numpy(x), torch.from_numpy(idx)


def acc_mask(H, M, seed, keep=0.7):
    """A random bool mask that keeps about `keep` of the rows."""
    return torch.from_numpy(np.random.default_rng(seed + 1).random((H, M)) < keep)


def out_of_range_indices(idx, K, seed):
    """About a tenth of the rows get an index outside [0, K): -1, K, K + 63, 2^40, -2^63 in turn.
    -> (idx', the rows changed [H, M] bool)."""
    rng = np.random.default_rng(seed + 2)
    idx = _idx(idx).copy()
    hit = rng.random(idx.shape) < 0.1
    bad = np.array([-1, K, K + 63, 2 ** 40, -2 ** 63], dtype=np.int64)
    idx[hit] = bad[np.arange(int(hit.sum())) % len(bad)]
    return torch.from_numpy(idx), torch.from_numpy(hit)


def nonfinite_inputs(H, M, K, D, seed):
    """float_inputs with three rows of the last head changed (D >= 3, K >= 2): row a = M // 7 has NaN in column 0; rows
    b = M // 3 and c = M - 2 share a code other than a's, b has +inf in columns 1 and 2, c has -inf in columns 1 and 0.
    The model's sums are then NaN at (code of a, 0) and (code of b, 1), +inf at (code of b, 2), -inf at (code of b, 0).
    -> (x, idx, (a, b, c))."""
    assert D >= 3 and K >= 2 and M >= 8
    x, idx = float_inputs(H, M, K, D, seed)
    a, b, c = M // 7, M // 3, M - 2
    ka = int(idx[-1, a])
    kb = (ka + 1 + int(idx[-1, b])) % K
    if kb == ka:
        kb = (ka + 1) % K
    idx[-1, b] = idx[-1, c] = kb
    x[-1, a, 0] = float("nan")
    x[-1, b, 1] = x[-1, b, 2] = float("inf")
    x[-1, c, 1] = x[-1, c, 0] = float("-inf")
    return x, idx, (a, b, c)


def error_ratio(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0, anything non-finite or x / 0 with x > 0 as inf)."""
    got, want, tol = (np.asarray(a, dtype=np.float64) for a in (got, want, tol))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / tol)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    return float(ratio.max()) if ratio.size else 0.0
