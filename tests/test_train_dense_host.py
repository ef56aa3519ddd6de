"""CPU checks of tests/train_dense.py: the models are right (fp64 autograd, the reference's own fp32 torch ops), the
reference alone stays within the derived bounds, and the bounds bite: deliberately wrong models fall outside them on the
very inputs the GPU tests use (tests/test_gpu_quantize_backward.py, tests/test_gpu_ema_update.py,
tests/test_gpu_ema_accumulate.py)."""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

import train_dense as td
from helpers import OracleBackend


# ------------------------------------------------------------------------------------------------
# quantize backward
# ------------------------------------------------------------------------------------------------
def _autograd64(x, cb, idx, go, ge, *, ste, share, per_head):
    """torch fp64 autograd of the reference formulation (straight-through output, detached codes, detached residual step)."""
    H, M, Q = idx.shape
    xs = x.double().requires_grad_(True)
    cbd = cb.double()
    harange = torch.arange(H)[:, None]
    gev = ge.reshape(H, Q) if per_head else ge.reshape(1, Q).expand(H, Q)
    r, out, loss = xs, 0.0, 0.0
    for q in range(Q):
        c = cbd[:, 0 if share else q][harange, idx[..., q]].detach()
        quant = r + (c - r).detach() if ste else c
        sq_err = ((c - r) ** 2).sum(dim=(1, 2))  # one per head
        loss = loss + (gev[:, q] * sq_err).sum()
        out = out + quant
        r = r - quant.detach()
    ((out * go.double()).sum() + loss).backward()
    return xs.grad.numpy()


@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("ste", [True, False])
def test_backward_model_equals_fp64_autograd(ste, share, per_head, Q):
    x, cb, idx, go, ge = td.backward_inputs(2, 9, 7, Q, 5, 11 + Q, per_head=per_head, share=share)
    want = _autograd64(x, cb, idx, go, ge, ste=ste, share=share, per_head=per_head)
    got, S = td.quantize_backward_model(x, cb, idx, go, ge, ste=ste, share=share, per_head=per_head, chain_dtype=np.float64)
    assert np.abs(got).max() > 0.1
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(S >= np.abs(got) * (1 - 1e-12))


def _reference_fp32_backward(x, cb, idx, go, ge, *, ste, share, per_head):
    """The package's own fp32 gather + elementwise formulas (_QuantizeFn.backward without a fused backend), on the CPU."""
    from vector_quantization import search

    ctx = types.SimpleNamespace(saved_tensors=(x, cb, idx), ste=ste, share=share, cb_err=False, per_head=per_head,
                                needs_input_grad=(True, False))
    search.set_backend(OracleBackend)  # has no quantize_backward: the torch formulas run
    try:
        return search._QuantizeFn.backward(ctx, go if ste else None, None, ge)[0]
    finally:
        search.set_backend(None)


@pytest.mark.parametrize("case", td.backward_cases()[::7], ids=str)
def test_reference_fp32_backward_is_within_the_bound(case):
    D, Q, H, ste, per_head = case
    x, cb, idx, go, ge = td.backward_case_inputs(*case)
    got = _reference_fp32_backward(x, cb, idx, go, ge, ste=ste, share=False, per_head=per_head)
    g, S = td.quantize_backward_model(x, cb, idx, go, ge, ste=ste, share=False, per_head=per_head)
    ratio = td.error_ratio(got.numpy(), g, td.quantize_backward_bound(S, Q))
    print(f"backward fp32 reference D={D} Q={Q} H={H} ste={ste}: error / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", td.backward_cases(), ids=str)
def test_wrong_backward_models_fall_outside_the_bound(case):
    D, Q, H, ste, per_head = case
    x, cb, idx, go, ge = td.backward_case_inputs(*case)
    kw = dict(ste=ste, share=False, per_head=per_head)
    g, S = td.quantize_backward_model(x, cb, idx, go, ge, **kw)
    tol = td.quantize_backward_bound(S, Q)
    # the loss term is as large as the straight-through term: otherwise the bound would hide it
    loss_part = np.abs(g - (Q * go.double().numpy() if ste else 0.0)).mean()
    assert loss_part > 0.1 * np.abs(g).mean()
    half, _ = td.quantize_backward_model(x, cb, idx, go, ge, factor=1.0, **kw)
    assert td.error_ratio(half, g, tol) > 1e4
    if Q > 1:
        stage0, _ = td.quantize_backward_model(x, cb, idx, go, ge, ge_stage0=True, **kw)
        assert td.error_ratio(stage0, g, tol) > 1e4
    if per_head:
        head0, _ = td.quantize_backward_model(x, cb, idx, go, ge[:1].expand(H, Q), **kw)
        assert td.error_ratio(head0[1:], g[1:], tol[1:]) > 1e4


def test_backward_cases_cover_the_issue_grid():
    cases = td.backward_cases()
    assert 90 <= len(cases) <= 120 and len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == set(td.BWD_DIMS) and {c[1] for c in cases} == set(td.BWD_STAGES)
    for D in td.BWD_DIMS:
        for Q in td.BWD_STAGES:
            assert {(c[2], c[3]) for c in cases if c[0] == D and c[1] == Q} >= {(1, True), (1, False)}
            assert any(c[2] == 3 for c in cases if c[0] == D and c[1] == Q)
    assert any(c[4] for c in cases) and any(c[2] == 3 and not c[4] for c in cases)


@pytest.mark.parametrize("scale", [1.0, 1e-4, 1e4])
def test_straight_through_and_plain_residual_chains_agree_bitwise(scale):
    """r - fl(r + fl(c - r)) = fl(r - c): with d = fl(c - r) = c - r + e, the sum r + d = c + e is either representable (then
    r - (c + e) = -d exactly) or rounds to a q with r - q = -d - e2, |e2| below half an ulp of d.  So the straight-through
    rule changes `out`, never the residual: a backward (or EMA statistics) kernel that used `quant = c` regardless of
    `ste` computes the same bits, and no test of gx can tell the two apart."""
    x, cb, idx, _go, _ge = td.backward_inputs(2, 500, 16, 5, 11, 77)
    x = x * scale  # rows far larger and far smaller than the codes
    a = td.residual_chain(x, cb, idx, ste=True, share=False)
    b = td.residual_chain(x, cb, idx, ste=False, share=False)
    for (ra, ca, _), (rb, cb_, _) in zip(a, b):
        assert np.array_equal(ra.view(np.int32), rb.view(np.int32))


# ------------------------------------------------------------------------------------------------
# EMA update
# ------------------------------------------------------------------------------------------------
def _reference_fp32_ema(inputs, decay, eps, l2norm):
    old, avg, counts, sums = (t.clone() for t in inputs)
    emb = torch.empty_like(avg)
    OracleBackend.ema_update(old, avg, emb, counts, sums, decay=decay, eps=eps, l2norm=l2norm)
    return old.numpy(), avg.numpy(), emb.numpy()


@pytest.mark.parametrize("l2norm", [False, True])
@pytest.mark.parametrize("decay", td.EMA_DECAYS)
@pytest.mark.parametrize("shape", td.EMA_SHAPES, ids=str)
def test_reference_fp32_ema_update_is_within_the_bounds(shape, decay, l2norm):
    H, K, D = shape
    inputs = td.ema_case_inputs(H, K, D)
    cs, avg, emb = _reference_fp32_ema(inputs, decay, td.EMA_EPS, l2norm)
    m = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm)
    tol_cs, tol_avg, tol_e = td.ema_update_bounds(m, K, D, l2norm)
    assert np.isfinite(m["emb"]).all() and np.isfinite(tol_e).all()
    ratios = (td.error_ratio(cs, m["cs"], tol_cs), td.error_ratio(avg, m["avg"], tol_avg), td.error_ratio(emb, m["emb"], tol_e))
    print(f"ema fp32 reference {shape} decay={decay} l2norm={l2norm}: error / bound cs {ratios[0]:.3f} avg {ratios[1]:.3f} "
          f"emb {ratios[2]:.3f}")
    assert max(ratios) <= 1.0


def test_ema_inputs_have_dead_codes_and_the_laplace_case():
    for H, K, D in td.EMA_SHAPES[1:]:
        old, avg, counts, sums = td.ema_case_inputs(H, K, D)
        dead = (old == 0) & (counts == 0)
        assert bool(dead[:, 0].all())
        assert bool((avg[dead] == 0).all()) and bool((sums[dead] == 0).all())
    inputs = td.ema_case_inputs(1, 5000, 4)
    assert 20 <= float(inputs[2].sum()) <= 80
    for decay in td.EMA_DECAYS:
        m = td.ema_update_model(*inputs, decay, td.EMA_EPS, False)
        assert 5000 * m["eps"] / float(m["tot"].min()) >= 1e-3
    m = td.ema_update_model(*td.ema_laplace_heads_inputs(), 0.8, td.EMA_EPS, False)
    assert m["tot"][1, 0] > 2 * m["tot"][0, 0] and 3000 * m["eps"] / float(m["tot"].max()) >= 2e-4


@pytest.mark.parametrize("l2norm", [False, True])
@pytest.mark.parametrize("decay", td.EMA_DECAYS)
def test_wrong_ema_models_fall_outside_the_bounds(decay, l2norm):
    # K eps dropped: the Laplace case
    inputs = td.ema_case_inputs(1, 5000, 4)
    m = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm)
    tol_e = td.ema_update_bounds(m, 5000, 4, l2norm)[2]
    wrong = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm, laplace=False)
    if not l2norm:  # (the l2norm divides a row's common factor out again)
        assert td.error_ratio(wrong["emb"], m["emb"], tol_e) > 100
    # the total of head 0 for every head: heads whose Laplace terms differ, and an empty head next to a live one
    inputs = td.ema_laplace_heads_inputs()
    m = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm)
    tol_e = td.ema_update_bounds(m, 3000, 4, l2norm)[2]
    wrong = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm, total_head0=True)
    assert np.array_equal(wrong["emb"][0], m["emb"][0])
    if not l2norm:
        assert td.error_ratio(wrong["emb"][1], m["emb"][1], tol_e[1]) > 100
    inputs = td.ema_isolation_inputs(0)
    m = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm)
    wrong = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm, total_head0=True)
    assert np.isfinite(m["emb"][1]).all() and not np.isfinite(wrong["emb"][1]).all()


@pytest.mark.parametrize("shape", td.EMA_SHAPES[1:], ids=str)
def test_ema_model_without_the_clamp_is_nan_on_dead_codes(shape):
    H, K, D = shape
    inputs = td.ema_case_inputs(H, K, D)
    m = td.ema_update_model(*inputs, 0.8, td.EMA_EPS, True)
    tol_e = td.ema_update_bounds(m, K, D, True)[2]
    wrong = td.ema_update_model(*inputs, 0.8, td.EMA_EPS, True, clamp=False)
    assert np.all(m["emb"][:, 0] == 0) and np.all(tol_e[:, 0] == 0)
    assert np.isnan(wrong["emb"][:, 0]).all()
    assert td.error_ratio(wrong["emb"], m["emb"], tol_e) == np.inf


# ------------------------------------------------------------------------------------------------
# residual statistics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("ste", [True, False])
def test_residual_stats_model_equals_reference_scatter(ste, share):
    """Every stage live: the model is OracleBackend.ema_accumulate_residual (the reference's scatter in fp32)."""
    x, cb, idx = td.residual_inputs(2, 300, 5, 4, 40, 21, share=share, drop=False)
    counts, sums, abs_sums = td.residual_stats_model(x, cb, idx, ste=ste, share=share)
    hits, ref = OracleBackend.ema_accumulate_residual(x, cb, idx, ste=ste, share=share)
    assert np.array_equal(counts, hits.numpy().astype(np.int64))
    assert td.error_ratio(ref.numpy(), sums, td.residual_sums_bound(counts, abs_sums)) <= 1.0


def test_residual_stats_model_ends_a_chain_at_the_first_dropped_stage():
    x, cb, idx = td.residual_inputs(1, 200, 5, 4, 40, 22, share=False)
    assert 0.2 < float((idx[..., -1] < 0).float().mean()) < 0.45 and bool((idx[..., 0] < 0).any())
    counts, sums, _ = td.residual_stats_model(x, cb, idx, ste=True, share=False)
    assert np.array_equal(counts.sum(-1)[0], (idx[0] >= 0).sum(0).numpy())
    # a live index after a dropped stage is not reached
    idx2 = idx.clone()
    row = int(torch.nonzero(idx[0, :, 1] < 0)[0])
    idx2[0, row, 3] = 7
    c2, s2, _ = td.residual_stats_model(x, cb, idx2, ste=True, share=False)
    assert np.array_equal(c2, counts) and np.array_equal(s2, sums)


# ------------------------------------------------------------------------------------------------
# EMA accumulation (the scatter-add): model, bound, exact data, mutants
# ------------------------------------------------------------------------------------------------
def _f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _keep(idx, mask, K):
    keep = (idx >= 0) & (idx < K)
    return keep if mask is None else keep & (mask != 0)


def _fp32_scatter(x, idx, keep, K, rows):
    """fp32 np.add.at (one rounded addition per row, in the order of `rows`) of the kept rows among `rows` -> [K, D]."""
    s = np.zeros((K, x.shape[1]), dtype=np.float32)
    rows = rows[keep[rows]]
    with np.errstate(invalid="ignore"):
        np.add.at(s, idx[rows], x[rows])
    return s


def _fp32_blocked(x, idx, keep, K, block=td.ACC_ROWS_PER_BLOCK):
    """The owner kernel's order: one fp32 partial per block of 2048 rows, then the partials merged left to right into 0."""
    total = np.zeros((K, x.shape[1]), dtype=np.float32)
    for r0 in range(0, x.shape[0], block):
        total = total + _fp32_scatter(x, idx, keep, K, np.arange(r0, min(r0 + block, x.shape[0])))
    return total


def test_accumulate_model_equals_a_plain_loop():
    H, M, K, D = 2, 200, 7, 3
    x, idx = td.float_inputs(H, M, K, D, 5)
    idx, hit = td.out_of_range_indices(idx, K, 5)
    mask = td.acc_mask(H, M, 5)
    assert 5 < int(hit.sum()) < 60 and 100 < int(mask.sum()) < 2 * M - 100
    counts, sums, abs_sums = td.accumulate_model(x, idx, mask, K)
    wc, ws, wa = np.zeros((H, K), np.int64), np.zeros((H, K, D)), np.zeros((H, K, D))
    for h in range(H):
        for m in range(M):
            k = int(idx[h, m])
            if bool(mask[h, m]) and 0 <= k < K:
                wc[h, k] += 1
                ws[h, k] += x[h, m].double().numpy()
                wa[h, k] += x[h, m].double().abs().numpy()
    assert np.array_equal(counts, wc) and int(wc.sum()) < int(mask.sum())
    assert np.abs(sums - ws).max() <= 1e-13 * wa.max() and np.abs(abs_sums - wa).max() <= 1e-13 * wa.max()
    # uint8 mask bytes other than 1 count as true; no mask keeps every in-range row
    c2, s2, _ = td.accumulate_model(x, idx, mask.to(torch.uint8) * 5, K)
    assert np.array_equal(c2, counts) and np.array_equal(s2, sums)
    assert int(td.accumulate_model(x, idx, None, K)[0].sum()) == int((~hit).sum())


@pytest.mark.parametrize("pattern", td.ACC_PATTERNS)
def test_exact_inputs_sum_exactly_in_fp32(pattern):
    """The precondition of the bitwise GPU comparison: sum |terms| < 2^24 * 2^-3 for every code and column, the fp64 model
    equals integer arithmetic, and the patterns are what their names say."""
    for H, M, K, D in td.ACC_SHAPES:
        x, idx = td.exact_inputs(H, M, K, D, td.acc_seed(H, M, K, D), pattern)
        assert tuple(x.shape) == (H, M, D) and tuple(idx.shape) == (H, M) and idx.dtype == torch.int64
        xi = np.rint(x.numpy().astype(np.float64) * 8).astype(np.int64)
        assert np.array_equal(xi.astype(np.float32) * np.float32(0.125), x.numpy()) and (M == 0 or np.abs(xi).max() <= 15)
        counts, sums, abs_sums = td.accumulate_model(x, idx, None, K)
        assert (abs_sums.max() if abs_sums.size else 0.0) < 2.0 ** 24 * 2.0 ** -3
        assert int(counts.sum()) == H * M
        want = np.zeros((H, K, D), dtype=np.int64)
        for h in range(H):
            np.add.at(want[h], idx[h].numpy(), xi[h])
        assert np.array_equal(sums * 8, want)
        assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums)
        i = idx.numpy()
        if pattern == "one_code":
            assert not i.any()
        elif pattern == "last_code":
            assert (i == K - 1).all()
        elif pattern == "half_empty":
            assert not (i % 2).any() and not counts[:, 1::2].any()
        elif pattern == "runs" and M >= 128:
            g = i[:, :M // 64 * 64].reshape(H, -1, 64)
            assert (g == g[..., :1]).all() and (K == 1 or (g[:, 1:, 0] != g[:, :-1, 0]).any())
        elif pattern == "uniform" and M >= 8 * K:
            assert (counts > 0).all()


@pytest.mark.parametrize("shape", td.ACC_SHAPES, ids=str)
def test_fp32_summation_orders_stay_within_the_bound(shape):
    """np.add.at in fp32 in three shuffled row orders, and the owner kernel's blocked order, against the fp64 model."""
    H, M, K, D = shape
    x, idx = td.float_inputs(H, M, K, D, td.acc_seed(*shape))
    mask = td.acc_mask(H, M, td.acc_seed(*shape)) if shape in td.ACC_MASK_SHAPES else None
    counts, sums, abs_sums = td.accumulate_model(x, idx, mask, K)
    tol = td.residual_sums_bound(counts, abs_sums)
    xn, im = x.numpy(), idx.numpy()
    keep = _keep(im, None if mask is None else mask.numpy(), K)
    rng = np.random.default_rng(3)
    worst = 0.0
    for h in range(H):
        evals = [_fp32_scatter(xn[h], im[h], keep[h], K, rng.permutation(M)) for _ in range(3)]
        evals.append(_fp32_blocked(xn[h], im[h], keep[h], K))
        for got in evals:
            worst = max(worst, td.error_ratio(got, sums[h], tol[h]))
    print(f"accumulate fp32 orders {shape}: error / bound = {worst:.3f}")
    assert worst <= 1.0
    if M >= 8 * K and K > 1 and mask is None:  # the cancelling pairs are there: a quarter of the codes sum to far less than sum |terms|
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(sums) / abs_sums
        assert np.nanmedian(rel[:, 1::4]) < 2e-2 * np.nanmedian(rel[:, 0::4])
    if M:
        col = np.abs(xn).reshape(-1, D).max(0)
        assert col.min() < 2.0 ** -15 or D < 2
        assert col.max() > 2.0 ** 18 or D < 2


def _caught(x, idx, mask, K, mutant, exact):
    """The model of a wrong kernel (`mutant`: inputs -> the inputs whose right result is the wrong kernel's result) against
    the model: on exact data -> True if counts or sums differ in a bit; on float data -> error / bound (inf if the counts
    differ)."""
    counts, sums, abs_sums = td.accumulate_model(x, idx, mask, K)
    x2, idx2, mask2 = mutant(x.clone(), idx.clone(), None if mask is None else mask.clone())
    c2, s2, _ = td.accumulate_model(x2, idx2, mask2, K)
    if exact:
        return not (np.array_equal(c2, counts) and np.array_equal(_f32_bits(s2), _f32_bits(sums)))
    if not np.array_equal(c2, counts):
        return np.inf
    return td.error_ratio(s2, sums, td.residual_sums_bound(counts, abs_sums))


def _first_row(x, idx, mask, K):
    """(head, row) of the first row that contributes and is not all zero."""
    keep = _keep(idx.numpy(), None if mask is None else mask.numpy(), K) & (x.numpy() != 0).any(-1)
    h, m = np.argwhere(keep)[0]
    return int(h), int(m)


def _all_true(idx):
    return torch.ones(idx.shape, dtype=torch.bool)


def _drop_row(K):
    def mutant(x, idx, mask):
        h, m = _first_row(x, idx, mask, K)
        mask = _all_true(idx) if mask is None else mask
        mask[h, m] = False
        return x, idx, mask
    return mutant


def _neighbour(K):
    def mutant(x, idx, mask):
        h, m = _first_row(x, idx, mask, K)
        k = int(idx[h, m])
        idx[h, m] = k + 1 if k + 1 < K else k - 1
        return x, idx, mask
    return mutant


def _last_column(x, idx, mask):
    x[..., -1] = 0
    return x, idx, mask


def _block0(x, idx, mask):
    mask = _all_true(idx) if mask is None else mask
    mask[:, :td.ACC_ROWS_PER_BLOCK] = False
    return x, idx, mask


def _both_inputs(shape):
    seed = td.acc_seed(*shape)
    yield True, td.exact_inputs(*shape, seed, "uniform")
    yield True, td.exact_inputs(*shape, seed, "runs")
    yield False, td.float_inputs(*shape, seed)


@pytest.mark.parametrize("shape", [s for s in td.ACC_SHAPES if s[1] > 0], ids=str)
def test_wrong_accumulate_models_are_caught_on_the_gpu_tests_inputs(shape):
    """One row dropped, one row credited to the neighbouring code, the last column of a D % 4 != 0 shape dropped, row
    block 0 left out of the merge.  The exact data catch every one of them at every shape.  The float data catch the
    gross ones everywhere and the single-row ones where the row's code has at most 1024 rows: the bound is then at most
    n_k 2^-23 sum |terms| <= 2^-13 n_k mean |terms| <= mean |terms| / 8 per column, and a row has an entry above an eighth
    of its column's mean in some column (with n_k = 5000 the bound exceeds the row itself)."""
    H, M, K, D = shape
    for exact, (x, idx) in _both_inputs(shape):
        counts = td.accumulate_model(x, idx, None, K)[0]
        h, m = _first_row(x, idx, None, K)
        small = int(counts[h, int(idx[h, m])]) <= 1024
        got = _caught(x, idx, None, K, _drop_row(K), exact)
        assert got is True if exact else (got > 1.0 or not small)
        if K > 1:
            got = _caught(x, idx, None, K, _neighbour(K), exact)
            assert got is True if exact else (got > 1.0 or not small)
        if D % 4 and M >= 8:
            got = _caught(x, idx, None, K, _last_column, exact)
            assert got is True if exact else got > 1.0
        if M > td.ACC_ROWS_PER_BLOCK:
            got = _caught(x, idx, None, K, _block0, exact)
            assert got is True if exact else got > 1.0


@pytest.mark.parametrize("shape", td.ACC_MASK_SHAPES, ids=str)
def test_an_inverted_mask_is_caught(shape):
    H, M, K, D = shape
    mask = td.acc_mask(H, M, td.acc_seed(*shape))
    assert 0.65 < float(mask.float().mean()) < 0.75
    for exact, (x, idx) in _both_inputs(shape):
        got = _caught(x, idx, mask, K, lambda x, idx, mask: (x, idx, ~mask), exact)
        assert got is True if exact else got > 1.0
        # a row that is dropped from the sums only (its count stays): the sums alone show it
        counts, sums, abs_sums = td.accumulate_model(x, idx, mask, K)
        s2 = td.accumulate_model(*_drop_row(K)(x.clone(), idx.clone(), mask.clone()), K)[1]
        assert not np.array_equal(_f32_bits(s2), _f32_bits(sums)) if exact else \
            td.error_ratio(s2, sums, td.residual_sums_bound(counts, abs_sums)) > 1.0


@pytest.mark.parametrize("shape", td.ACC_RANGE_SHAPES, ids=str)
def test_clamped_out_of_range_indices_are_caught(shape):
    H, M, K, D = shape
    for exact, (x, idx) in _both_inputs(shape):
        idx, hit = td.out_of_range_indices(idx, K, td.acc_seed(*shape))
        bad = idx[hit].numpy()
        assert 0.07 * H * M < bad.size < 0.13 * H * M
        assert set(np.unique(bad).tolist()) == {-2 ** 63, -1, K, K + 63, 2 ** 40}
        assert int(td.accumulate_model(x, idx, None, K)[0].sum()) == H * M - bad.size
        got = _caught(x, idx, None, K, lambda x, idx, mask: (x, idx.clamp(0, K - 1), mask), exact)
        assert got is True if exact else got > 1.0
        # (the truncation of an index to 32 bits: 2^40 -> 0, -2^63 -> 0)
        got = _caught(x, idx, None, K, lambda x, idx, mask: (x, idx.to(torch.int32).to(torch.int64), mask), exact)
        assert got is True if exact else got > 1.0


@pytest.mark.parametrize("shape", td.ACC_NONFINITE_SHAPES, ids=str)
def test_nonfinite_inputs_have_the_classes_their_docstring_names(shape):
    H, M, K, D = shape
    x, idx, (a, b, c) = td.nonfinite_inputs(H, M, K, D, td.acc_seed(*shape))
    ka, kb = int(idx[-1, a]), int(idx[-1, b])
    assert ka != kb and int(idx[-1, c]) == kb
    counts, sums, abs_sums = td.accumulate_model(x, idx, None, K)
    s = sums[-1]
    assert np.isnan(s[ka, 0]) and np.isnan(s[kb, 1]) and s[kb, 2] == np.inf and s[kb, 0] == -np.inf
    assert int((~np.isfinite(sums)).sum()) == 4 and int(counts.sum()) == H * M
    if M > td.ACC_ROWS_PER_BLOCK:  # +inf and -inf meet only when the row blocks are merged
        assert b < td.ACC_ROWS_PER_BLOCK <= c


def test_empty_inputs_pass_the_binding_stride_check():
    """torch.from_numpy of an array without elements has all-zero strides (and is contiguous): the M = 0 case of the GPU
    tests reaches native.ema_accumulate with such a tensor, whose strides nothing reads."""
    from vector_quantization import native

    x, idx = td.exact_inputs(1, 0, 4, 8, td.acc_seed(1, 0, 4, 8), "uniform")
    assert x.is_contiguous() and x.stride(-1) != 1
    assert native._row_strides(x) == (int(x.stride(1)), int(x.stride(0)))
    with pytest.raises(AssertionError, match="last dim must be contiguous"):
        native._row_strides(torch.zeros((1, 3, 8)).transpose(1, 2))
