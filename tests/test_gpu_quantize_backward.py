"""vq_quantize_backward_kernel through direct native.quantize_backward calls.

Compared with tests/train_dense.py's fp64 model under the derived bound |got - g| <= (Q + 5) 2^-23 S (see that module's
docstring; tests/test_train_dense_host.py shows the bound rejects a factor 1 instead of 2, ge[0] for every stage and head
0's g_err row for every head on these very inputs), and bit for bit wherever the result is exactly determined: no g_err,
a single non-zero g_err entry of 0.5 (gx is then the fp32 residual chain's r_q - c_q itself), layouts, the scalar fallback,
a shared codebook, per-head g_err rows, the grid-stride row loop.  Indices come from torch.randint: the kernel does not
care whether they are winners.  Every case is small; the largest tensor is about 1 MB."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import train_dense as td

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {"ratio": 0.0}


def _native():
    from vector_quantization import native

    return native


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _call(x, cb, idx, go, ge, *, ste, share=False, per_head=False):
    return _native().quantize_backward(x, cb, idx, go, ge, ste=ste, stages_share_codebook=share, sq_err_per_head=per_head)


# ------------------------------------------------------------------------------------------------
# the fp64 model and the derived bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", td.backward_cases(), ids=lambda c: f"D{c[0]}-Q{c[1]}-H{c[2]}-ste{int(c[3])}")
def test_backward_within_derived_bound_of_fp64_model(case):
    D, Q, H, ste, per_head = case
    x, cb, idx, go, ge = td.backward_case_inputs(*case)
    got = _call(*_dev(x, cb, idx, go, ge), ste=ste, per_head=per_head)
    assert got.shape == (H, td.BWD_M, D) and got.is_contiguous()
    g, S = td.quantize_backward_model(x, cb, idx, go, ge, ste=ste, share=False, per_head=per_head)
    ratio = td.error_ratio(got.cpu().numpy(), g, td.quantize_backward_bound(S, Q))
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"quantize_backward D={D} Q={Q} H={H} ste={ste}: error / bound = {ratio:.3f} (worst so far {WORST['ratio']:.3f})")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------
EXACT_DIMS = (3, 64, 260)


@pytest.mark.parametrize("Q", [3, 5])
@pytest.mark.parametrize("D", EXACT_DIMS)
def test_without_g_err_the_gradient_is_q_times_grad_out_bitwise(D, Q):
    x, cb, idx, go, _ = td.backward_inputs(2, 37, D, Q, 11, 300 + D + Q)
    got = _call(*_dev(x, cb, idx, go), None, ste=True)
    assert _same(got, go * np.float32(Q))


@pytest.mark.parametrize("D", EXACT_DIMS)
def test_nothing_to_propagate_gives_all_zero_bits(D):
    x, cb, idx, go, ge = td.backward_inputs(2, 37, D, 3, 11, 310 + D)
    xd, cd, idd, god = _dev(x, cb, idx, go)
    zero_ge = torch.zeros(3, dtype=torch.float64, device=DEV)
    for got in (_call(xd, cd, idd, god, None, ste=False), _call(xd, cd, idd, None, zero_ge, ste=True),
                _call(xd, cd, idd, None, zero_ge, ste=False), _call(xd, cd, idd, None, None, ste=True)):
        assert got.shape == x.shape and not _bits(got).any()


@pytest.mark.parametrize("ste", [True, False])
@pytest.mark.parametrize("stage", [0, 2, 4])
@pytest.mark.parametrize("D", EXACT_DIMS)
def test_single_g_err_entry_returns_the_fp32_chain_bitwise(D, stage, ste):
    """g_err = 0.5 at one stage, 0 elsewhere: coef is 1.0f there, every other term +-0, so gx = 0 + (r_q - c_q) exactly, fma
    or not.  Pins the in-kernel residual chain (with and without the straight-through rule) against the CPU fp32 chain.
    (The two rules give the same residuals: r - (r + (c - r)) is -fl(c - r) = fl(r - c), see test_train_dense_host.py.)"""
    Q = 5
    x, cb, idx, _go, _ = td.backward_inputs(2, 37, D, Q, 11, 320 + D)
    ge = torch.zeros(Q, dtype=torch.float64)
    ge[stage] = 0.5
    got = _call(*_dev(x, cb, idx), None, ge.to(DEV), ste=ste)
    r, c, _live = td.residual_chain(x, cb, idx, ste=ste, share=False)[stage]
    want = np.float32(0) + (r - c)
    assert np.array_equal(_bits(got), want.view(np.int32))
    if stage > 0:  # the chain matters: stage 0's difference is something else
        r0, c0, _ = td.residual_chain(x, cb, idx, ste=ste, share=False)[0]
        assert not np.array_equal(want, r0 - c0)


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 64])
def test_permuted_views_and_strided_indices_equal_the_contiguous_call_bitwise(D):
    H, M, Q = 3, 37, 3
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, M, D, Q, 11, 400 + D))
    want = _call(x, cb, idx, go, ge, ste=True)

    def rows_view(t):  # [H, M, D] view of [M, H * D] storage
        v = t.permute(1, 0, 2).contiguous().view(M, H * D).view(M, H, D).permute(1, 0, 2)
        assert v.stride() == (D, H * D, 1) and torch.equal(v, t)
        return v

    idx_mhq = idx.permute(1, 0, 2).contiguous().permute(1, 0, 2)  # [M, H, Q] storage
    idx_qhm = idx.permute(2, 0, 1).contiguous().permute(1, 2, 0)  # [Q, H, M] storage
    assert idx_mhq.stride() == (Q, H * Q, 1) and idx_qhm.stride() == (M, 1, H * M)
    assert _same(_call(rows_view(x), cb, idx, rows_view(go), ge, ste=True), want)
    assert _same(_call(x, cb, idx_mhq, go, ge, ste=True), want)
    assert _same(_call(rows_view(x), cb, idx_qhm, rows_view(go), ge, ste=True), want)


def test_misaligned_x_takes_the_scalar_path_and_equals_the_aligned_call_bitwise():
    H, M, D, Q = 2, 37, 64, 3
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, M, D, Q, 11, 410))
    want = _call(x, cb, idx, go, ge, ste=True)
    buf = torch.empty(H * M * D + 1, device=DEV)
    off = buf[1:].view(H, M, D)
    off.copy_(x)
    assert x.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    assert _same(_call(off, cb, idx, go, ge, ste=True), want)
    gbuf = torch.empty(H * M * D + 1, device=DEV)
    goff = gbuf[1:].view(H, M, D)
    goff.copy_(go)
    assert _same(_call(x, cb, idx, goff, ge, ste=True), want)


def test_grad_out_with_a_non_unit_last_stride_is_copied():
    H, M, D, Q = 2, 37, 12, 2
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, M, D, Q, 11, 420))
    wide = torch.zeros((H, M, 2 * D), device=DEV)
    wide[..., ::2] = go
    wide[..., 1::2] = 99.0
    view = wide[..., ::2]
    assert view.stride(-1) == 2
    assert _same(_call(x, cb, idx, view, ge, ste=True), _call(x, cb, idx, go, ge, ste=True))


# ------------------------------------------------------------------------------------------------
# codebook and head handling
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 64])
def test_shared_codebook_equals_the_repeated_codebook_bitwise(D):
    H, M, Q = 2, 37, 4
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, M, D, Q, 11, 500 + D, share=True))
    assert cb.shape[1] == 1
    got = _call(x, cb, idx, go, ge, ste=True, share=True)
    want = _call(x, cb.repeat(1, Q, 1, 1).contiguous(), idx, go, ge, ste=True)
    assert _same(got, want)
    g, S = td.quantize_backward_model(*(t.cpu() for t in (x, cb, idx, go, ge)), ste=True, share=True, per_head=False)
    assert td.error_ratio(got.cpu().numpy(), g, td.quantize_backward_bound(S, Q)) <= 1.0


@pytest.mark.parametrize("D", [5, 64])
def test_per_head_g_err_rows_equal_single_head_calls_bitwise(D):
    H, M, Q = 3, 37, 3
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, M, D, Q, 11, 510 + D, per_head=True))
    assert ge.shape == (H, Q) and not torch.equal(ge[0], ge[1]) and not torch.equal(ge[0], ge[2])
    got = _call(x, cb, idx, go, ge, ste=True, per_head=True)
    for h in range(H):
        one = _call(x[h:h + 1], cb[h:h + 1], idx[h:h + 1], go[h:h + 1], ge[h], ste=True)
        assert _same(got[h:h + 1], one), h
    row0 = _call(x, cb, idx, go, ge[0], ste=True)
    assert _same(row0[0], got[0]) and not _same(row0[1], got[1]) and not _same(row0[2], got[2])


# ------------------------------------------------------------------------------------------------
# grid-stride loop and small edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 3])
def test_more_rows_than_the_grid_holds(D):
    """M = 4 * 8192 + 5: the grid is capped at 8192 workgroups of 4 rows, so rows 32768 .. 32772 are a wave's second trip."""
    M, Q = 4 * 8192 + 5, 1
    x, cb, idx, go, ge = td.backward_inputs(1, M, D, Q, 11, 600 + D)
    got = _call(*_dev(x, cb, idx, go, ge), ste=True).cpu().numpy()
    g, S = td.quantize_backward_model(x, cb, idx, go, ge, ste=True, share=False, per_head=False)
    tol = td.quantize_backward_bound(S, Q)
    assert np.abs(g[0, 32768:]).min() > 0
    assert td.error_ratio(got[0, 32768:], g[0, 32768:], tol[0, 32768:]) <= 1.0  # rows 32768 .. 32772, the last rows
    assert td.error_ratio(got[0, 32760:32768], g[0, 32760:32768], tol[0, 32760:32768]) <= 1.0
    assert td.error_ratio(got, g, tol) <= 1.0


@pytest.mark.parametrize("D", [3, 64])
def test_one_row_and_no_rows(D):
    Q = 2
    x, cb, idx, go, ge = td.backward_inputs(2, 1, D, Q, 11, 610 + D)
    got = _call(*_dev(x, cb, idx, go, ge), ste=True)
    g, S = td.quantize_backward_model(x, cb, idx, go, ge, ste=True, share=False, per_head=False)
    assert td.error_ratio(got.cpu().numpy(), g, td.quantize_backward_bound(S, Q)) <= 1.0
    xd, cd, idd, god, ged = _dev(x, cb, idx, go, ge)
    empty = _call(xd[:, :0], cd, idd[:, :0], god[:, :0], ged, ste=True)
    assert empty.shape == (2, 0, D) and empty.dtype == torch.float32
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# input safety
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 64])
def test_inputs_are_left_unchanged(D):
    x, cb, idx, go, ge = _dev(*td.backward_inputs(2, 37, D, 3, 11, 700 + D))
    keep = [t.clone() for t in (x, cb, idx, go, ge)]
    _call(x, cb, idx, go, ge, ste=True)
    _call(x, cb, idx, go, ge, ste=False)
    torch.cuda.synchronize()
    for t, k in zip((x, cb, idx, go, ge), keep):
        assert torch.equal(t, k)
