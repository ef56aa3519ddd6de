"""CPU checks of tests/train_dense.py: the models are right (fp64 autograd, the reference's own fp32 torch ops), the
reference alone stays within the derived bounds, and the bounds bite: deliberately wrong models fall outside them on the
very inputs the GPU tests use (tests/test_gpu_quantize_backward.py, tests/test_gpu_ema_update.py)."""
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
