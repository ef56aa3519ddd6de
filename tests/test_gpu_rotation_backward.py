"""vq_rotate_backward_kernel through direct native.rotate_backward calls.

Compared with tests/rotation_dense.py's fp64 model under its derived bound (that module's docstring; tests/test_rotation_host.py
shows the model is the fp64 autograd of the literal composition and that the bound rejects a model without the 2 (g.qh) u term
and one with lam = 1).  Every case prints error / bound.  M = 37, K = 11: ten workgroups of four rows, the last one ragged;
D runs over train_dense.BWD_DIMS up to 1024, so every register variant (f32x4 x 1 / 2 / 4, float x 1 / 2 / 4 / 8 / 16), the vector
and the scalar path run, and 252 / 260 straddle the first variant boundary.  Indices come from torch.randint: the kernel does not
care whether they are winners.  Worst error / bound seen on an MI355X: profiles/rotation_trick.md.

The wrapper's case in the table of native calls (tests/native_cases.py) lets the poison suites run it on poisoned allocations,
on inputs embedded in poisoned buffers and on far operands."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import rotation_dense as rd
import train_dense as td

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {"ratio": 0.0}
# (510 and 1022: the two widest scalar variants, which no dim of BWD_DIMS below 1024 reaches; 1024: the widest vector one)
DIMS = tuple(d for d in td.BWD_DIMS if d <= 1024) + (510, 1022, 1024)


def _native():
    from vector_quantization import native

    return native


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _call(x, cb, idx, go, ge, *, share=False, per_head=False, ste=True):
    return _native().rotate_backward(x, cb, idx, go, ge, ste=ste, stages_share_codebook=share, sq_err_per_head=per_head)


def _ratio(got, x, cb, idx, go, ge, *, share=False, per_head=False, what=""):
    g, tol = rd.rotate_backward_model(x, cb, idx, go, ge, share=share, per_head=per_head)
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    ratio = td.error_ratio(got, g, tol)
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"rotate_backward {what}: error / bound = {ratio:.3f} (worst so far {WORST['ratio']:.3f})")
    return ratio


# ------------------------------------------------------------------------------------------------
# the fp64 model and the derived bound
# ------------------------------------------------------------------------------------------------
def _cases():
    cases = []
    for i, D in enumerate(DIMS):
        for j, Q in enumerate(td.BWD_STAGES):
            for H in (1, 3):
                if H == 3 and (i + j) % 2:
                    continue
                cases.append((D, Q, H, H == 3 and Q != 2))
    return cases


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"D{c[0]}-Q{c[1]}-H{c[2]}")
def test_backward_within_derived_bound_of_fp64_model(case):
    D, Q, H, per_head = case
    x, cb, idx, go, ge = td.backward_inputs(H, td.BWD_M, D, Q, td.BWD_K, 2000 + D * 16 + Q * 4 + H, per_head=per_head)
    got = _call(*_dev(x, cb, idx, go, ge), per_head=per_head)
    assert got.shape == (H, td.BWD_M, D) and got.is_contiguous()
    assert _ratio(got, x, cb, idx, go, ge, per_head=per_head, what=f"D={D} Q={Q} H={H}") <= 1.0


@pytest.mark.parametrize("D", [3, 64, 260, 1024])
def test_grad_out_only_and_grad_sq_err_only(D):
    Q = 3
    x, cb, idx, go, ge = td.backward_inputs(2, td.BWD_M, D, Q, td.BWD_K, 2100 + D)
    xd, cd, idd, god, ged = _dev(x, cb, idx, go, ge)
    assert _ratio(_call(xd, cd, idd, god, None), x, cb, idx, go, None, what=f"D={D} grad_out only") <= 1.0
    loss_only = _call(xd, cd, idd, None, ged)
    assert _ratio(loss_only, x, cb, idx, None, ge, what=f"D={D} grad_sq_err only") <= 1.0
    # the loss term alone is what the existing backward computes without its straight-through term
    other = _native().quantize_backward(xd, cd, idd, None, ged, ste=False)
    g, tol = rd.rotate_backward_model(x, cb, idx, None, ge, share=False, per_head=False)
    g_q, S = td.quantize_backward_model(x, cb, idx, None, ge, ste=False, share=False, per_head=False)
    assert np.array_equal(g, g_q)  # (the two rules of the chain give the same residuals: tests/test_train_dense_host.py)
    both = tol + td.quantize_backward_bound(S, Q)
    assert td.error_ratio(loss_only.cpu().numpy(), other.cpu().numpy(), both) <= 1.0
    neither = _call(xd, cd, idd, None, None)
    assert neither.shape == x.shape and not neither.cpu().numpy().any()


@pytest.mark.parametrize("D", [5, 64, 520])
def test_shared_codebook_equals_the_repeated_codebook_bitwise(D):
    H, M, Q = 2, td.BWD_M, 4
    x, cb, idx, go, ge = td.backward_inputs(H, M, D, Q, td.BWD_K, 2200 + D, share=True)
    xd, cd, idd, god, ged = _dev(x, cb, idx, go, ge)
    got = _call(xd, cd, idd, god, ged, share=True)
    assert _same(got, _call(xd, cd.repeat(1, Q, 1, 1).contiguous(), idd, god, ged))
    assert _ratio(got, x, cb, idx, go, ge, share=True, what=f"D={D} shared") <= 1.0


@pytest.mark.parametrize("D", [5, 64])
def test_per_head_g_err_rows_equal_single_head_calls_bitwise(D):
    H, Q = 3, 3
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, td.BWD_M, D, Q, td.BWD_K, 2300 + D, per_head=True))
    got = _call(x, cb, idx, go, ge, per_head=True)
    for h in range(H):
        assert _same(got[h:h + 1], _call(x[h:h + 1], cb[h:h + 1], idx[h:h + 1], go[h:h + 1], ge[h])), h
    row0 = _call(x, cb, idx, go, ge[0])
    assert _same(row0[0], got[0]) and not _same(row0[1], got[1])


def test_more_stages_than_one_wave_of_lanes_holds():
    """Q = 70: the indices and loss coefficients are kept one per lane, stages 64 .. 69 are the second batch."""
    H, D, Q = 1, 12, 70
    x, cb, idx, go, ge = td.backward_inputs(H, td.BWD_M, D, Q, td.BWD_K, 2400)
    cb = cb * 0.2  # (a long random chain: keep the residuals of order 1)
    got = _call(*_dev(x, cb, idx, go, ge))
    assert _ratio(got, x, cb, idx, go, ge, what="Q=70") <= 1.0


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 64, 300])
def test_embedded_rows_strided_indices_and_strided_grad_out_equal_the_contiguous_call_bitwise(D):
    H, M, Q = 3, td.BWD_M, 3
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, M, D, Q, td.BWD_K, 2500 + D))
    want = _call(x, cb, idx, go, ge)
    pad = 8  # (keeps 16-byte alignment at D = 64, so the vector path runs on strided rows)

    def embedded(t):  # [H, M, D] view with a row stride > D and a head stride, inside a larger NaN-filled buffer
        buf = torch.full((M, H, D + pad), float("nan"), device=DEV)
        v = buf[:, :, :D].permute(1, 0, 2)
        v.copy_(t)
        assert v.stride() == (D + pad, H * (D + pad), 1)
        return v

    idx_mhq = idx.permute(1, 0, 2).contiguous().permute(1, 0, 2)  # [M, H, Q] storage
    idx_qhm = idx.permute(2, 0, 1).contiguous().permute(1, 2, 0)  # [Q, H, M] storage
    assert not idx_mhq.is_contiguous() and not idx_qhm.is_contiguous()
    assert _same(_call(embedded(x), cb, idx, go, ge), want)
    assert _same(_call(x, cb, idx_mhq, embedded(go), ge), want)
    assert _same(_call(embedded(x), cb, idx_qhm, embedded(go), ge), want)


def test_misaligned_rows_take_the_scalar_path_within_the_bound():
    H, M, D, Q = 2, td.BWD_M, 64, 3
    x, cb, idx, go, ge = td.backward_inputs(H, M, D, Q, td.BWD_K, 2600)
    xd, cd, idd, god, ged = _dev(x, cb, idx, go, ge)
    buf = torch.empty(H * M * D + 1, device=DEV)
    off = buf[1:].view(H, M, D)
    off.copy_(xd)
    assert xd.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    got = _call(off, cd, idd, god, ged)
    assert _ratio(got, x, cb, idx, go, ge, what="misaligned x") <= 1.0
    # the scalar variant sums in another order: the same result up to rounding, not a copy of the vector variant's
    assert _ratio(_call(xd, cd, idd, god, ged), x, cb, idx, go, ge, what="aligned x") <= 1.0


@pytest.mark.parametrize("D", [4, 3])
def test_more_rows_than_the_grid_holds(D):
    """M = 4 * 8192 + 5: the grid is capped at 8192 workgroups of 4 rows, so rows 32768 .. 32772 are a wave's second trip."""
    M, Q = 4 * 8192 + 5, 1
    x, cb, idx, go, ge = td.backward_inputs(1, M, D, Q, td.BWD_K, 2700 + D)
    got = _call(*_dev(x, cb, idx, go, ge)).cpu().numpy()
    g, tol = rd.rotate_backward_model(x, cb, idx, go, ge, share=False, per_head=False)
    assert np.abs(g[0, 32768:]).min() > 0
    assert td.error_ratio(got[0, 32768:], g[0, 32768:], tol[0, 32768:]) <= 1.0
    assert td.error_ratio(got, g, tol) <= 1.0


@pytest.mark.parametrize("D", [3, 64])
def test_one_row_and_no_rows(D):
    Q = 2
    x, cb, idx, go, ge = td.backward_inputs(2, 1, D, Q, td.BWD_K, 2800 + D)
    xd, cd, idd, god, ged = _dev(x, cb, idx, go, ge)
    assert _ratio(_call(xd, cd, idd, god, ged), x, cb, idx, go, ge, what=f"D={D} one row") <= 1.0
    empty = _call(xd[:, :0], cd, idd[:, :0], god[:, :0], ged)
    assert empty.shape == (2, 0, D) and empty.dtype == torch.float32
    torch.cuda.synchronize()


def test_rows_wider_than_the_kernel_holds_are_refused():
    x, cb, idx, go, ge = _dev(*td.backward_inputs(1, 5, 1028, 1, td.BWD_K, 2900))
    with pytest.raises(AssertionError):
        _call(x, cb, idx, go, ge)


# ------------------------------------------------------------------------------------------------
# exact and degenerate rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 64, 260, 1024])
def test_degenerate_rows_are_finite_and_within_the_bound(D):
    """c = -r, c = r (the next stage's residual is exactly 0), an all-zero x row and a zero code, inside a random batch."""
    Q = 2
    x, cb, idx, go, ge, rows = rd.degenerate_inputs(2, td.BWD_M, D, Q, td.BWD_K, 3000 + D)
    got = _call(*_dev(x, cb, idx, go, ge))
    assert torch.isfinite(got).all()
    assert _ratio(got, x, cb, idx, go, ge, what=f"D={D} degenerate rows") <= 1.0
    g, tol = rd.rotate_backward_model(x, cb, idx, go, ge, share=False, per_head=False)
    for row in rows:
        assert td.error_ratio(got[-1, row].cpu().numpy(), g[-1, row], tol[-1, row]) <= 1.0, row


def test_exact_rows():
    """Stage count 1, no loss term.  c = r: the rotation is the identity, and a zero code gives exactly no gradient."""
    D = 64
    x, cb, idx, go, _ge, (_anti, same, _zero_x, zero_c) = rd.degenerate_inputs(1, td.BWD_M, D, 1, td.BWD_K, 3100)
    got = _call(*_dev(x, cb, idx, go), None).cpu().numpy()
    assert not got[0, zero_c].any()
    assert np.abs(got[0, same] - go[0, same].numpy()).max() <= 1e-5 * np.abs(go[0, same].numpy()).max()


# ------------------------------------------------------------------------------------------------
# non-finite isolation, input safety
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 64])
def test_a_nan_row_changes_no_other_row(D):
    H, M, Q = 2, td.BWD_M, 3
    x, cb, idx, go, ge = _dev(*td.backward_inputs(H, M, D, Q, td.BWD_K, 3200 + D))
    want = _call(x, cb, idx, go, ge)
    for where in ("x", "go"):
        xn, gn = x.clone(), go.clone()
        (xn if where == "x" else gn)[1, 17, D // 2] = float("nan")
        got = _call(xn, cb, idx, gn, ge)
        keep = torch.ones((H, M), dtype=torch.bool, device=DEV)
        keep[1, 17] = False
        assert _same(got[keep], want[keep]), where
        assert torch.isnan(got[1, 17]).any()


@pytest.mark.parametrize("D", [5, 64])
def test_inputs_are_left_unchanged(D):
    x, cb, idx, go, ge = _dev(*td.backward_inputs(2, td.BWD_M, D, 3, td.BWD_K, 3300 + D))
    keep = [t.clone() for t in (x, cb, idx, go, ge)]
    _call(x, cb, idx, go, ge)
    torch.cuda.synchronize()
    for t, k in zip((x, cb, idx, go, ge), keep):
        assert torch.equal(t, k)
