"""GPU: the mask pass of a residual stack (vq_residual_mask_f32 / vq_residual_mask_backward_f32) against the numpy statement
of its rule (tests/residual_mask_rule.py) at every shape edge of its lane mapping, and the fused masked / quantize-dropout
forwards of ResidualVQ and GroupedResidualVQ against the layer-by-layer route (VQ_RVQ_NO_FUSED_MASK=1) and against the
fixtures captured from the reference (tests/golden/make_golden_rvq_mask.py).

The case of the two entry points in the table of native calls (tests/native_cases.py) shares this module's inputs
(native_cases.residual_mask_inputs), so that the poison suites run them like every other one and find their kernels launched."""
from __future__ import annotations

import copy
import random

import numpy as np
import pytest
import torch

import residual_mask_rule as rule
import train_dense as td
from native_cases import DEV, RESIDUAL_MASK_K as K_DIRECT, residual_mask_inputs as _inputs
from rvq_mask_run import (BY_NAME, CASES, DIM, Q, build_module, case_inputs, check_against_fixture, ema_state, forward_backward,
                          grad_close, rel_close, run_case, same)

pytestmark = pytest.mark.gpu

MASKS = ("all", "none", "alternating", "boundary", "nonfinite")


def _native():
    from vector_quantization import native

    native.load()
    return native


def _strided(t, pad, fill):
    """``t`` [G, M, W] as a view of a [G, M, W + pad] tensor filled with ``fill`` (the view starts at element 0 of a row)."""
    wide = torch.full((*t.shape[:-1], t.shape[-1] + pad), fill, dtype=t.dtype, device=DEV)
    wide[..., : t.shape[-1]] = t.to(DEV)
    return wide, wide[..., : t.shape[-1]]


def sq_err_bound(D):
    """Relative bound against the fp64 sum of the fp32 squares, the form of helpers.finalize_sq_err_bound, (L R + 9) 2^-24: a
    lane adds L = 4 ceil(D / 256) squares per row for the R = 2 rows it holds, then six butterfly additions; the rest is fp64."""
    return (4 * -(-D // 256) * 2 + 9) * 2.0 ** -24


@pytest.mark.parametrize("M", [1, 33, 257])
@pytest.mark.parametrize("D", [1, 4, 5, 64, 257, 512])
def test_kernels_against_the_rule(D, M):
    native = _native()
    combos = [(Qn, G) for Qn in (1, 3, 8) for G in (1, 2)]
    worst_e = worst_g = 0.0
    for n, (Qn, G) in enumerate(combos):
        for k, kind in enumerate(MASKS):
            share = (n + k) % 2 == 1 and Qn > 1
            train = (n + k) % 3 != 0
            pad = (0, 4, 1)[(n + k) % 3]  # dense / strided rows that keep 16-byte accesses / rows off the 16-byte grid
            x, cb, idx, zero_idx, mask = _inputs(G, M, D, Qn, share, kind, 1000 * D + 10 * M + n * 7 + k)
            per_group = G > 1 and k % 2 == 0
            _, xv = _strided(torch.from_numpy(x), pad, float("nan"))
            out_wide, out_v = _strided(torch.zeros((G, M, D)), pad, 7.0)
            idx_wide, idx_v = _strided(torch.from_numpy(idx), 2, -5)
            mask_t = torch.from_numpy(mask).to(DEV)
            out, sq_err = native.residual_mask(xv, torch.from_numpy(cb).to(DEV), idx_v, mask_t, torch.from_numpy(zero_idx).to(DEV),
                                               train=train, want_sq_err=True, sq_err_per_group=per_group, out=out_v)
            go = torch.randn((G, M, D), generator=torch.Generator().manual_seed(n + k))
            ge = torch.linspace(-1.0, 1.0, G * Qn if per_group else Qn, dtype=torch.float64)
            _, go_v = _strided(go, pad, float("nan"))
            gx = native.residual_mask_backward(xv, torch.from_numpy(cb).to(DEV), idx_v, mask_t, go_v, ge.to(DEV), train=train,
                                               sq_err_per_group=per_group)
            torch.cuda.synchronize()
            what = f"D={D} M={M} Q={Qn} G={G} share={share} train={train} pad={pad} mask={kind}"
            assert bool((out_wide[..., D:] == 7.0).all()) and bool((idx_wide[..., Qn:] == -5).all()), what + ": pads written"
            want_err = np.zeros((G, Qn))
            for g in range(G):
                f = rule.forward(x[g], cb[g], idx[g], mask, zero_idx[g], train=train)
                assert np.array_equal(idx_v[g].cpu().numpy(), f["idx"]), what + ": idx"
                assert same(out[g].cpu().numpy(), f["out"]), what + ": out"
                want_err[g] = f["sq_err"]
                g_ref, S = rule.backward(f, mask, go[g].numpy(), (ge.reshape(G, Qn)[g] if per_group else ge).numpy(), train=train)
                got = gx[g].cpu().numpy().astype(np.float64)
                ok = np.isfinite(g_ref)
                assert np.array_equal(np.isfinite(got), ok), what + ": non-finite gradient elements"
                worst_g = max(worst_g, td.error_ratio(got[ok], g_ref[ok], td.quantize_backward_bound(S[ok], Qn)))
            got_err = sq_err.cpu().numpy().reshape(-1, Qn)
            want = want_err if per_group else want_err.sum(0, keepdims=True)
            if kind == "none":
                assert not got_err.any(), what + ": no kept row, the sums are 0"
            if kind in ("all", "none", "alternating", "boundary"):
                assert not np.isnan(out.cpu().numpy()).any(), what
            rel = np.abs(got_err - want) / np.maximum(want, 1e-300)
            worst_e = max(worst_e, float(rel[want > 0].max()) if (want > 0).any() else 0.0)
            assert np.array_equal(got_err == 0, want == 0), what
    print(f"D = {D}, M = {M}: sq_err worst relative error {worst_e:.3e} (bound {sq_err_bound(D):.3e}); "
          f"backward worst error / bound {worst_g:.3f}")
    assert worst_e <= sq_err_bound(D)
    assert worst_g <= 1.0


def test_rows_beyond_one_grid_pass_and_bad_arguments():
    """More units than the grid holds waves (the unit loop strides), indices outside [0, K) read as code 0, M == 0, and the
    argument checks."""
    native = _native()
    lib = native.load()
    cus = int(native.device_info().split()[-2])
    G, D, Qn = 1, 256, 2
    M = 8 * cus * 4 * 2 + 3  # units = ceil(M / 2) > 8 * CUs blocks x 4 waves
    x, cb, idx, zero_idx, mask = _inputs(G, M, D, Qn, False, "alternating", 5)
    idx[0, 4, 1] = K_DIRECT + 3  # (rows 4 and 6 are kept rows)
    idx[0, 6, 0] = -2
    t = [torch.from_numpy(a).to(DEV) for a in (x, cb, idx, mask, zero_idx)]
    out, sq_err = native.residual_mask(*t, train=True, want_sq_err=True)
    idx_fixed = idx.copy()
    idx_fixed[0, 4, 1] = 0
    idx_fixed[0, 6, 0] = 0
    f = rule.forward(x[0], cb[0], idx_fixed[0], mask, zero_idx[0], train=True)
    assert same(out[0].cpu().numpy(), f["out"])
    assert rel_close(sq_err.cpu().numpy(), f["sq_err"], sq_err_bound(D))
    empty = [torch.empty((1, 0, D), device=DEV), t[1], torch.empty((1, 0, Qn), dtype=torch.int64, device=DEV),
             torch.empty((0,), dtype=torch.bool, device=DEV), t[4]]
    out0, err0 = native.residual_mask(*empty, train=True, want_sq_err=True)
    assert out0.shape == (1, 0, D) and err0.tolist() == [0.0, 0.0]
    ws = torch.empty(1024, device=DEV)
    m8 = t[3].view(torch.uint8)

    def fwd(D=D, M=8, x=t[0].data_ptr(), ws_bytes=4096, zero=t[4].data_ptr()):
        return lib.vq_residual_mask_f32(x, M * D, D, t[1].data_ptr(), Qn * K_DIRECT * D, K_DIRECT * D, t[2].data_ptr(), M * Qn, Qn, 1,
                                        m8.data_ptr(), 0, zero, 1, M, Qn, K_DIRECT, D, 1, out.data_ptr(), M * D, D,
                                        sq_err.data_ptr(), 0, ws.data_ptr(), ws_bytes, None)

    assert fwd() == 0
    assert fwd(D=513) == -1 and fwd(D=0) == -1 and fwd(M=-1) == -1
    assert fwd(x=None) == -1 and fwd(zero=None) == -1
    assert fwd(ws_bytes=8) == -1 and b"workspace" in lib.vq_last_error()
    assert lib.vq_residual_mask_backward_f32(t[0].data_ptr(), 8 * D, D, t[1].data_ptr(), Qn * K_DIRECT * D, K_DIRECT * D,
                                             t[2].data_ptr(), 8 * Qn, Qn, 1, m8.data_ptr(), 0, 1, 8, Qn, K_DIRECT, D, 1, None, 0, 0,
                                             None, 0, None, 8 * D, D, None) == -1
    torch.cuda.synchronize()


def test_custom_op_gives_the_wrappers_result():
    native = _native()
    import vector_quantization  # noqa: F401  (registers the ops)

    x, cb, idx, zero_idx, mask = _inputs(2, 70, 20, 3, False, "boundary", 9)
    a = [torch.from_numpy(v).to(DEV) for v in (x, cb, idx, mask, zero_idx)]
    b = [v.clone() for v in a]
    out, sq_err = native.residual_mask(*a, train=True, want_sq_err=True, sq_err_per_group=True)
    out_b = torch.empty_like(out)
    got = torch.ops.vq_mi355x.residual_mask(*b, out_b, True, True, True)
    assert torch.equal(got, sq_err) and torch.equal(out_b, out) and torch.equal(a[2], b[2])
    torch.library.opcheck(torch.ops.vq_mi355x.residual_mask.default, (*[v.clone() for v in b], torch.empty_like(out), True, True, True),
                          test_utils=("test_schema", "test_faketensor"))


# ------------------------------------------------------------------------------------------------------------- the modules
@pytest.fixture(scope="module")
def layered():
    """The layer-by-layer results of every fixture case, computed once: (module state after the step, q, idx, losses, grad)."""
    import os

    os.environ["VQ_RVQ_NO_FUSED_MASK"] = "1"
    try:
        return {c["name"]: run_case(c, DEV) for c in CASES}
    finally:
        del os.environ["VQ_RVQ_NO_FUSED_MASK"]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_fused_equals_layered_and_the_reference(c, layered):
    mod, q, idx, losses, grad = run_case(c, DEV)
    _, q_l, idx_l, losses_l, grad_l = layered[c["name"]]
    assert torch.equal(idx, idx_l), "indices: fused against layered"
    assert same(q.cpu().numpy(), q_l.cpu().numpy()), "output: fused against layered"
    assert losses.shape == losses_l.shape and rel_close(losses.cpu().numpy(), losses_l.cpu().numpy())
    if c["grad"]:
        assert grad_close(grad.cpu().numpy(), grad_l.cpu().numpy())
    check_against_fixture(c, mod, q, idx, losses, grad)


def _grid_case(**kw):
    c = dict(BY_NAME["rvq_mask_ema"])
    c.update(kw)
    return c


def _grid_inputs(G=1, groups_dim=1):
    """Grid-valued rows and codes (multiples of 1/8 in [-2, 2]): every EMA sum is exact in any order."""
    from gen import CB_SEED, make_rvq_codebooks, make_x
    from rvq_mask_cases import K, X_SHAPE, make_mask

    cbs = torch.stack([make_rvq_codebooks(Q, K, DIM, "G", seed=CB_SEED + 100 * g) for g in range(G)])
    return make_x((*X_SHAPE[:-1], G * DIM), "G"), cbs, make_mask()


@pytest.mark.parametrize("kind", ["rvq", "grvq"])
@pytest.mark.parametrize("threshold", [0, 2], ids=["no-expiry", "expiry"])
def test_ema_buffers_equal_the_layered_route(kind, threshold, monkeypatch):
    """One EMA step on grid-valued inputs: the three buffers of every layer are equal bit for bit, with the dead codes
    (threshold 2: most of the 64 codes see fewer than two of the 58 kept rows) re-seeded from the same pool by the same draws."""
    c = _grid_case(kind=kind, cb_extra=dict(threshold_ema_dead_code=threshold))
    x, cbs, mask = _grid_inputs(2 if kind == "grvq" else 1)
    states = []
    for switch in ("0", "1"):
        monkeypatch.setenv("VQ_RVQ_NO_FUSED_MASK", switch)
        mod = build_module(c, cbs, DEV)
        before = ema_state(mod)
        torch.manual_seed(77)
        q, idx, losses, _ = forward_backward(mod, c, x.to(DEV), mask.to(DEV))
        states.append((ema_state(mod), q, idx, losses))
    (fused, q, idx, losses), (lay, q_l, idx_l, losses_l) = states
    assert torch.equal(idx, idx_l) and torch.equal(q, q_l) and rel_close(losses.cpu().numpy(), losses_l.cpu().numpy())
    for attr in fused:
        assert torch.equal(fused[attr], lay[attr]), attr
    assert not torch.equal(fused["embeddings"], before["embeddings"])
    if threshold:
        rows = x.reshape(-1, x.shape[-1])[:, :DIM]
        # a re-seeded code: cluster_size = the reset value and embed_avg = the picked row times it, exactly
        reseeded = ((fused["cluster_size"] == 2.0) & (fused["embed_avg"] == fused["embeddings"] * 2.0).all(-1)).reshape(-1, cbs.shape[-2])
        assert int(reseeded[0].sum()) > 8, "the case is about a stage-0 codebook in which codes expire"
        picked = fused["embeddings"].reshape(-1, cbs.shape[-2], DIM)[0][reseeded[0]]
        assert bool((picked[:, None, :] == rows[None]).all(-1).any(-1).all()), "stage 0 re-seeds from the rows of x"
        late = fused["embeddings"].reshape(-1, cbs.shape[-2], DIM)[1][reseeded[1]]
        assert bool((late == 0).all(-1).any()), "stage 1 draws from a pool that holds the masked-out rows' zero residual"


def _seed_for_cut(cut, cutoff=0):
    return next(s for s in range(200) if random.Random(s).randrange(cutoff, Q) == cut)


@pytest.mark.parametrize("cut", range(Q))
@pytest.mark.parametrize("masked", [False, True], ids=["dropout", "dropout+mask"])
def test_quantize_dropout_every_cut(cut, masked, monkeypatch):
    c = dict(BY_NAME["rvq_mask_dropout"])
    x, cbs, mask = case_inputs(c)
    seed = _seed_for_cut(cut)
    runs = []
    for switch in ("0", "1"):
        monkeypatch.setenv("VQ_RVQ_NO_FUSED_MASK", switch)
        mod = build_module(c, cbs, DEV)
        runs.append(forward_backward(mod, c, x.to(DEV), mask.to(DEV) if masked else None,
                                     fwd_extra=dict(rand_quantize_dropout_fixed_seed=seed)))
    (q, idx, losses, grad), (q_l, idx_l, losses_l, grad_l) = runs
    assert bool((idx[..., cut + 1:] == -1).all()) and bool((idx[..., : cut + 1] >= 0).all())
    assert torch.equal(idx, idx_l) and torch.equal(q, q_l)
    assert losses.shape == losses_l.shape and losses.dtype == losses_l.dtype and rel_close(losses.cpu().numpy(), losses_l.cpu().numpy())
    assert not bool(losses[..., cut + 1:].any())
    assert grad_close(grad.cpu().numpy(), grad_l.cpu().numpy())


def test_grouped_dropout_fuses_inside_the_group_loop(monkeypatch):
    """Active dropout keeps the loop over the groups (each draws its own cut from the shared stream); every group fuses on
    its own: one mask pass per group, the results those of the layered route."""
    native = _native()
    c = dict(BY_NAME["rvq_mask_grouped"])
    c["rvq_extra"] = dict(quantize_dropout=True)
    x, cbs, mask = case_inputs(c)
    calls = []
    real = native.residual_mask
    monkeypatch.setattr(native, "residual_mask", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    runs = []
    for switch in ("0", "1"):
        monkeypatch.setenv("VQ_RVQ_NO_FUSED_MASK", switch)
        random.seed(5)
        mod = build_module(c, cbs, DEV)
        runs.append(forward_backward(mod, c, x.to(DEV), mask.to(DEV)))
    assert [tuple(s) for s in calls] == [(1, 120, DIM)] * cbs.shape[0]
    (q, idx, losses, grad), (q_l, idx_l, losses_l, grad_l) = runs
    assert torch.equal(idx, idx_l) and torch.equal(q, q_l) and rel_close(losses.cpu().numpy(), losses_l.cpu().numpy())
    assert grad_close(grad.cpu().numpy(), grad_l.cpu().numpy())


def test_no_kept_row_gives_nan_losses_and_nothing_else():
    c = BY_NAME["rvq_mask_train"]
    x, cbs, mask = case_inputs(c)
    mod = build_module(c, cbs, DEV)
    q, idx, losses, grad = forward_backward(mod, c, x.to(DEV), torch.zeros_like(mask).to(DEV))
    assert bool(torch.isnan(losses).all()), "the reference's mean over no rows"
    assert torch.equal(q, x.to(DEV)) and bool((idx >= 0).all())
    assert bool((idx[..., 1:].reshape(-1, Q - 1) == idx[0, 0, 1:]).all())


def test_one_masked_forward_is_one_mask_pass_and_no_layer_loop(monkeypatch):
    """A masked forward of a Q = 8 stack: native.residual_mask once, ResidualVQ._forward_layers never."""
    import vector_quantization as vq
    from gen import make_rvq_codebooks

    native = _native()
    c = dict(BY_NAME["rvq_mask_train"])
    cbs = make_rvq_codebooks(8, 64, DIM, "S")[None]
    x, _, mask = case_inputs(c)
    mod = build_module(c, cbs, DEV)
    calls = {"mask_pass": 0, "layers": 0}
    real = native.residual_mask

    def counted(*a, **k):
        calls["mask_pass"] += 1
        return real(*a, **k)

    def layers(self, *a, **k):
        calls["layers"] += 1
        raise AssertionError("the masked forward walked its layers")

    monkeypatch.setattr(native, "residual_mask", counted)
    monkeypatch.setattr(vq.ResidualVQ, "_forward_layers", layers)
    q, idx, losses, grad = forward_backward(mod, c, x.to(DEV), mask.to(DEV))
    assert calls == {"mask_pass": 1, "layers": 0}
    assert idx.shape == (*x.shape[:2], 8) and losses.shape == (1, 8) and grad is not None


def test_masked_forward_and_backward_under_one_graph():
    c = BY_NAME["rvq_mask_train"]
    x, cbs, mask = case_inputs(c)
    mod = build_module(c, cbs, DEV)
    xd, md = x.to(DEV).requires_grad_(True), mask.to(DEV)
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    kept = {}

    def step(mod, x):
        q, idx, losses = mod(x, mask=md, freeze_codebook=True)
        ((q * w).sum() + losses.sum()).backward()
        return q.detach(), idx, losses.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(mod, xd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    xd.grad = None
    twin, tx = copy.deepcopy(mod), xd.detach().clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kept["out"] = step(mod, xd)
    graph.replay()
    want = step(twin, tx)
    torch.cuda.synchronize()
    for got, ref in zip(kept["out"], want):
        assert torch.equal(got, ref)
    assert xd.grad is not None and bool(xd.grad.any()) and torch.equal(xd.grad, tx.grad)
