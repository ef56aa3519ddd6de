"""Host: the rule of the masked residual stack (tests/residual_mask_rule.py) against the fixtures captured from the reference
(tests/golden/make_golden_rvq_mask.py), the two new symbols in the binding and the header, and the modules' fused masked route
driven on the CPU by a backend whose mask pass IS the rule (the search is the oracle's)."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

import residual_mask_rule as rule
from helpers import OracleBackend, checksum_close, load_golden
from rvq_mask_run import (BY_NAME, CASES, DIM, GROUPS, Q, case_inputs, check_against_fixture, dropout_cut, grad_close, q_weights,
                          rel_close, run_case, same)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vq_residual_mask_f32", "vq_residual_mask_backward_f32")


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_rule_reproduces_the_reference(c):
    arrays, meta = load_golden(c["name"])
    x, cbs, mask = case_inputs(c)
    assert checksum_close(x.nan_to_num(0.0, 0.0, 0.0), meta["x_checksum"])[0], "the seeded inputs drifted"
    G = cbs.shape[0]
    run = dropout_cut(c) + 1
    rows = x.shape[0] * x.shape[1]
    m = mask.reshape(rows).numpy()
    kept = int(m.sum())
    weights = q_weights(x.shape).reshape(rows, G, DIM).numpy()
    for g in range(G):
        xg = x.reshape(rows, G, DIM)[:, g].numpy()
        want_idx = arrays["idx"][g] if c["kind"] == "grvq" else arrays["idx"]
        want_idx = want_idx.reshape(rows, Q)
        stage0 = np.where(np.isfinite(xg).all(1), -1, want_idx[:, 0])  # (a non-finite row's stage 0 is the search's answer)
        f = rule.search_chain(xg, cbs[g, :run].numpy(), m, train=c["training"], stage0=stage0)
        assert np.array_equal(f["idx"], want_idx[:, :run]) and bool((want_idx[:, run:] == -1).all())
        want_q = arrays["q_full"].reshape(rows, G, DIM)[:, g]
        assert same(f["out"], want_q)
        assert same(f["out"][~m & np.isfinite(xg).all(1)], xg[~m & np.isfinite(xg).all(1)]), "out == x on masked-out rows"
        want_loss = (arrays["loss"][g] if c["kind"] == "grvq" else arrays["loss"]).reshape(Q)
        if c["training"]:
            assert rel_close(f["sq_err"] / (kept * DIM), want_loss[:run]) and not want_loss[run:].any()
        else:
            assert not want_loss.any()
        if c["grad"]:
            gx, _ = rule.backward(f, m, weights[:, g], np.full(run, 1.0 / (kept * DIM)), train=True)
            want_g = arrays["g_full"].reshape(rows, G, DIM)[:, g].astype(np.float64)
            assert grad_close(gx, want_g)
            # masked-out rows: d out / d x = I per stage that ran, and no loss term
            assert same(gx[~m], run * weights[:, g][~m].astype(np.float64))


def test_fixtures_hold_the_cases_they_are_for():
    arrays, _ = load_golden("rvq_mask_nonfinite")
    x, _, mask = case_inputs(BY_NAME["rvq_mask_nonfinite"])
    rows = x.reshape(-1, DIM)
    bad = ~torch.isfinite(rows).all(1)
    assert bad.sum() == 2 and not bool(mask.reshape(-1)[bad].any()), "the non-finite rows are masked-out rows"
    idx, q = arrays["idx"].reshape(-1, Q), arrays["q_full"].reshape(-1, DIM)
    assert not idx[bad.numpy(), 1:].any() and np.isnan(q[bad.numpy()]).sum() == 2  # code 0, NaN in exactly those elements
    finite_out = ~mask.reshape(-1).numpy() & ~bad.numpy()
    assert len(np.unique(idx[finite_out, 1:], axis=0)) == 1, "one answer per stage for every finite masked-out row"
    d = load_golden("rvq_mask_dropout")[0]["idx"]
    assert (d[..., -1] == -1).all() and (d[..., 0] >= 0).all(), "the fixed seed drops at least the last stage"


def test_symbols_are_bound_and_declared():
    from vector_quantization import native

    header = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTED_SYMBOLS and name in native._SIGNATURES
        assert re.search(rf"\bint\s+{name}\s*\(", header), f"{name} is not declared in the header"
    assert callable(native.residual_mask) and callable(native.residual_mask_backward)


# ------------------------------------------------------------------------------------ the modules' fused route on the CPU
class RuleBackend(OracleBackend):
    """The oracle's search plus a mask pass that is the numpy rule: what the native backend gives the modules, on the CPU."""

    name = "cpu-oracle + mask rule (tests only)"
    calls = []

    @staticmethod
    def residual_mask(x, cb, idx, mask, zero_idx, *, train, want_sq_err, per_group=False, out=None):
        G, M, D = x.shape
        Qr = idx.shape[-1]
        RuleBackend.calls.append((G, M, Qr))
        res = torch.empty((G, M, D)) if out is None else out
        err = np.zeros((G, Qr))
        m = mask.reshape(-1, M)
        for g in range(G):
            f = rule.forward(x[g].detach().numpy(), cb[g].numpy(), idx[g].numpy(), m[g if m.shape[0] > 1 else 0].numpy(),
                             zero_idx[g].numpy(), train=train)
            res[g].copy_(torch.from_numpy(f["out"]))
            idx[g].copy_(torch.from_numpy(f["idx"]))
            err[g] = f["sq_err"]
        if not want_sq_err:
            return res, None
        return res, torch.from_numpy(err if per_group else err.sum(0))

    @staticmethod
    def ema_accumulate_residual(x, cb, idx, *, ste, share):
        """The native kernel's rule: an index outside [0, K) ends a row's chain (the oracle's version has no such rows)."""
        h, m, d = x.shape
        stages, k = idx.shape[-1], cb.shape[2]
        hits, sums = torch.zeros((h, stages, k)), torch.zeros((h, stages, k, d))
        r, live = x, torch.ones((h, m), dtype=torch.bool)
        harange = torch.arange(h)[:, None]
        for q in range(stages):
            live = live & (idx[..., q] >= 0) & (idx[..., q] < k)
            safe = idx[..., q].clamp(0, k - 1)
            hits[:, q], sums[:, q] = OracleBackend.ema_accumulate(r, safe, k, live)
            c = cb[:, 0 if share else q][harange, safe]
            r = r - (r + (c - r) if ste else c)
        return hits, sums

    @staticmethod
    def residual_mask_backward(x, cb, idx, mask, grad_out, grad_sq_err, *, train, per_group=False):
        G, M, D = x.shape
        gx = torch.empty((G, M, D))
        m = mask.reshape(-1, M)
        for g in range(G):
            mg = m[g if m.shape[0] > 1 else 0].numpy()
            f = rule.forward(x[g].numpy(), cb[g].numpy(), idx[g].numpy(), mg, idx[g, 0].numpy() * 0, train=train)
            ge = None if grad_sq_err is None else (grad_sq_err[g] if per_group else grad_sq_err).numpy()
            gx[g] = torch.from_numpy(rule.backward(f, mg, None if grad_out is None else grad_out[g].numpy(), ge, train=train)[0]).float()
        return gx


@pytest.fixture
def rule_backend():
    from vector_quantization import search

    RuleBackend.calls = []
    search.set_backend(RuleBackend)
    try:
        yield RuleBackend
    finally:
        search.set_backend(None)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_fused_route_reproduces_the_reference(c, rule_backend):
    """The host side of the fused masked forward (views, strides, denominators, EMA masking, dropout cut, groups) with the
    rule standing in for the kernel; grouped stacks draw a seed of their own for the (inactive) dropout, nothing else."""
    out = run_case(c)
    assert len(rule_backend.calls) == 1, "one mask pass per forward"
    assert rule_backend.calls[0][0] == (GROUPS if c["kind"] == "grvq" else 1)
    check_against_fixture(c, *out)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_switch_restores_the_layered_route(c, rule_backend, monkeypatch):
    monkeypatch.setenv("VQ_RVQ_NO_FUSED_MASK", "1")
    out = run_case(c)
    assert rule_backend.calls == []
    check_against_fixture(c, *out)
