"""vq_ema_accumulate_kernel, vq_ema_accumulate_owner_kernel and vq_ema_reduce_parts_kernel, the project's scatter-add,
through native.ema_accumulate (deterministic=False / True) and the raw C entry points.

Two references (tests/train_dense.py; its docstring has the derivations, tests/test_train_dense_host.py shows on the CPU
that fp32 summation in any order stays within the bound and that a dropped row, a row credited to the neighbouring code,
a dropped last column, a row block left out of the merge, an inverted mask and a clamped index are caught on these very
inputs):
  exact data   rows of integers in [-15, 15] times 2^-3: every fp32 addition is exact in any order, so counts and sums
               must equal the integer model BIT FOR BIT on every path
  float data   randn rows with column scales 2^-20 .. 2^20 and cancelling pairs: counts exact, sums within the order-free
               bound n_k 2^-23 sum |terms| of the fp64 model

The shapes (td.ACC_SHAPES, H M K D) and the branch of the owner kernel's launch plan each one takes:
  1 1024 8 32, 1 1023 8 32   the two sides of the owner / atomic boundary M / owners == 1024, one owner
  1 5000 3 4                 cw = K = 3, three row blocks, the last one 904 rows: 14 full groups of 64 and 8 rows
  2 4500 70 20               two heads, cw = 64, the second owner has kvalid = 6, waves 2 and 3 return early, float4 loads
  1 3000 40 5                D % 4 != 0: scalar loads, D4 = 8
  1 2048 1 64                K = 1
  1 2100 2 256 / 257 / 260 / 512   one 256-dim pass exactly / a second pass with one scalar lane / with one float4 lane /
                             two full passes
  1 3100 7 600               cw = 3, three owners, kvalid = 1 in the last, three passes
  1 2100 2 2048              cw = 1, eight passes
  1 2100 2 2052              no owner plan: atomic kernel, deterministic=True raises, the workspace sizer answers 0
  1 37 5 3, 2 1000 256 64, 1 300 8192 16   atomic kernel, codes that no row hits
  1 1 4 8, 1 0 4 8           one row; no rows (zeros back)
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import train_dense as td

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {"ratio": 0.0}
BADARG = -1  # VQ_E_BADARG
ENTRIES = (False, True)  # native.ema_accumulate(.., deterministic=)


def _native():
    from vector_quantization import native

    native.load()
    return native


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _cw_owners(K, D):
    D4 = (D + 3) & ~3
    cw = min(64, 2048 // D4, K)
    return cw, -(-K // cw)


def _takes_owner_kernel(H, M, K, D):
    """Which kernel vq_ema_accumulate_f32 launches.  Mirrors the device-independent half of ema_owner_plan and the
    condition in vq_ema_accumulate_f32 (csrc/vq_kernels.hip): the choice is not observable from outside."""
    if D > 2048:
        return False
    _cw, owners = _cw_owners(K, D)
    return M // owners >= 1024


def _row_blocks(H, M, K, D):
    with torch.cuda.device(DEV):
        nbytes = int(_native().load().vq_ema_det_workspace_bytes(H, M, K, D))
    assert nbytes > 256 and (nbytes - 256) % (H * K * (D + 1) * 4) == 0
    return (nbytes - 256) // (H * K * (D + 1) * 4)


def _run(x, idx, K, mask, deterministic):
    counts, sums = _native().ema_accumulate(x.to(DEV), idx.to(DEV), K, None if mask is None else mask.to(DEV),
                                            deterministic=deterministic)
    torch.cuda.synchronize()
    return counts, sums


@functools.lru_cache(maxsize=None)
def _exact(shape, pattern):
    """(x, idx, model counts, model sums) of one exact case, computed once and shared (nobody writes to them)."""
    x, idx = td.exact_inputs(*shape, td.acc_seed(*shape), pattern)
    counts, sums, _ = td.accumulate_model(x, idx, None, shape[2])
    return x, idx, counts, sums


@functools.lru_cache(maxsize=None)
def _float(shape):
    x, idx = td.float_inputs(*shape, td.acc_seed(*shape))
    return (x, idx) + td.accumulate_model(x, idx, None, shape[2])


def _assert_exact(got, want_c, want_s, what):
    counts, sums = got
    assert tuple(counts.shape) == want_c.shape and tuple(sums.shape) == want_s.shape
    cb, sb = _bits(counts), _bits(sums)
    assert np.array_equal(cb, _bits(want_c)), f"{what}: counts differ"
    bad = np.argwhere(sb != _bits(want_s))
    assert bad.size == 0, f"{what}: {len(bad)} sums differ, the first at (head, code, column) {tuple(bad[0])}"
    assert not sb[want_c == 0].any(), f"{what}: a code without rows does not hold +0.0"


def _assert_within_bound(got, want_c, want_s, abs_s, what, where=None):
    counts, sums = got
    assert np.array_equal(_bits(counts), _bits(want_c)), f"{what}: counts differ"
    s, tol = sums.cpu().numpy(), td.residual_sums_bound(want_c, abs_s)
    if where is not None:
        s, want_s, tol = s[where], want_s[where], tol[where]
    ratio = td.error_ratio(s, want_s, tol)
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"ema_accumulate {what}: error / bound = {ratio:.3f} (worst so far {WORST['ratio']:.3f})")
    assert ratio <= 1.0, what
    return ratio


def _ids(shape):
    return "H%d-M%d-K%d-D%d" % shape


# ------------------------------------------------------------------------------------------------
# the shape table
# ------------------------------------------------------------------------------------------------
def test_shape_table_has_both_kernels_and_the_plan_edges_it_names():
    owner = [s for s in td.ACC_SHAPES if _takes_owner_kernel(*s)]
    atomic = [s for s in td.ACC_SHAPES if not _takes_owner_kernel(*s)]
    assert (1, 1024, 8, 32) in owner and (1, 1023, 8, 32) in atomic
    assert {(1, 2100, 2, 2052), (1, 37, 5, 3), (2, 1000, 256, 64), (1, 300, 8192, 16), (1, 1, 4, 8), (1, 0, 4, 8)} <= set(atomic)
    assert len(owner) == 11 and len(atomic) == 7
    assert _cw_owners(3, 4) == (3, 1) and _cw_owners(70, 20) == (64, 2) and _cw_owners(40, 5) == (40, 1)
    assert _cw_owners(7, 600) == (3, 3) and _cw_owners(2, 2048) == (1, 2) and _cw_owners(2, 512) == (2, 1)
    # more than one row block where the table says so (the deterministic entry takes the owner kernel at every M)
    assert _row_blocks(1, 5000, 3, 4) == 3 and _row_blocks(2, 4500, 70, 20) == 3
    for shape in td.ACC_SHAPES:
        H, M, K, D = shape
        if M > td.ACC_ROWS_PER_BLOCK and D <= 2048:
            assert _row_blocks(*shape) == -(-M // td.ACC_ROWS_PER_BLOCK) >= 2, shape
        elif M > 0 and D <= 2048:
            assert _row_blocks(*shape) == 1, shape
    assert {s for s in td.ACC_MASK_SHAPES + td.ACC_RANGE_SHAPES + td.ACC_NONFINITE_SHAPES} <= set(td.ACC_SHAPES)
    # the out-of-range cases: owner path, atomic path, cw = 64 with K inside the last owner's range
    assert [_takes_owner_kernel(*s) for s in td.ACC_RANGE_SHAPES] == [True, False, True]
    cw, owners = _cw_owners(70, 20)
    assert (owners - 1) * cw <= 70 < owners * cw
    assert [_takes_owner_kernel(*s) for s in td.ACC_NONFINITE_SHAPES] == [True, False]


# ------------------------------------------------------------------------------------------------
# exact data: bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", td.ACC_PATTERNS)
@pytest.mark.parametrize("shape", td.ACC_SHAPES, ids=_ids)
def test_exact_data_equals_the_integer_model_bit_for_bit(shape, pattern):
    H, M, K, D = shape
    x, idx, want_c, want_s = _exact(shape, pattern)
    for deterministic in ENTRIES:
        if deterministic and D > 2048:
            with torch.cuda.device(DEV):
                assert _native().load().vq_ema_det_workspace_bytes(H, M, K, D) == 0
            with pytest.raises(RuntimeError, match="D <= 2048"):
                _run(x, idx, K, None, True)
            continue
        _assert_exact(_run(x, idx, K, None, deterministic), want_c, want_s, f"{shape} {pattern} deterministic={deterministic}")
    if pattern in ("one_code", "last_code", "half_empty") and K > 1 and M > 0:
        assert (want_c == 0).any()
    if M == 0:
        assert not want_c.any() and not want_s.any()


# ------------------------------------------------------------------------------------------------
# float data: the derived bound, and run-to-run identity of the deterministic entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", td.ACC_SHAPES, ids=_ids)
def test_float_data_within_the_bound_and_reproducible(shape):
    H, M, K, D = shape
    x, idx, want_c, want_s, abs_s = _float(shape)
    _assert_within_bound(_run(x, idx, K, None, False), want_c, want_s, abs_s, f"{shape} deterministic=False")
    if D > 2048:
        return
    first = _run(x, idx, K, None, True)
    _assert_within_bound(first, want_c, want_s, abs_s, f"{shape} deterministic=True")
    if M == 0:
        return
    with torch.cuda.device(DEV):
        nbytes = int(_native().load().vq_ema_det_workspace_bytes(H, M, K, D))
    for _ in range(2):
        # an unrelated tensor of the workspace's size takes the block the last run freed and lives through the next run:
        # the workspace moves
        other = torch.full(((nbytes + 15) // 16 * 2,), 3.0, dtype=torch.float64, device=DEV)
        again = _run(x, idx, K, None, True)
        del other
        assert np.array_equal(_bits(again[0]), _bits(first[0])) and np.array_equal(_bits(again[1]), _bits(first[1]))


# ------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", ENTRIES)
@pytest.mark.parametrize("shape", td.ACC_MASK_SHAPES, ids=_ids)
def test_random_mask_against_the_model(shape, deterministic):
    H, M, K, D = shape
    mask = td.acc_mask(H, M, td.acc_seed(*shape))
    x, idx, _, _ = _exact(shape, "uniform")
    want_c, want_s, _ = td.accumulate_model(x, idx, mask, K)
    assert 0.65 * H * M < int(want_c.sum()) < 0.75 * H * M
    _assert_exact(_run(x, idx, K, mask, deterministic), want_c, want_s, f"{shape} masked exact deterministic={deterministic}")
    x, idx = _float(shape)[:2]
    want_c, want_s, abs_s = td.accumulate_model(x, idx, mask, K)
    _assert_within_bound(_run(x, idx, K, mask, deterministic), want_c, want_s, abs_s,
                         f"{shape} masked deterministic={deterministic}")


@pytest.mark.parametrize("shape", td.ACC_MASK_SHAPES, ids=_ids)
def test_all_true_all_false_and_non_contiguous_masks(shape):
    H, M, K, D = shape
    x, idx = _float(shape)[:2]
    plain = _run(x, idx, K, None, True)
    ones = _run(x, idx, K, torch.ones((H, M), dtype=torch.bool), True)
    assert np.array_equal(_bits(ones[0]), _bits(plain[0])) and np.array_equal(_bits(ones[1]), _bits(plain[1]))
    for deterministic in ENTRIES:
        c, s = _run(x, idx, K, torch.zeros((H, M), dtype=torch.bool), deterministic)
        assert not _bits(c).any() and not _bits(s).any()
    # a bool mask as a transposed view of an [M, H] tensor
    mask = td.acc_mask(H, M, td.acc_seed(*shape))
    view = mask.t().contiguous().to(DEV).t()
    assert tuple(view.shape) == (H, M) and torch.equal(view.cpu(), mask) and (H == 1 or not view.is_contiguous())
    if H == 1:  # (a [1, M] transpose is contiguous: a strided slice of an [M, 3] tensor instead)
        wide = torch.zeros((M, 3), dtype=torch.bool)
        wide[:, 1] = mask[0]
        view = wide.to(DEV)[:, 1][None]
        assert not view.is_contiguous() and torch.equal(view.cpu(), mask)
    a = _run(x, idx, K, view, True)
    b = _run(x, idx, K, mask.contiguous(), True)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    want_c = td.accumulate_model(x, idx, mask, K)[0]
    assert np.array_equal(_bits(a[0]), _bits(want_c))
    x, idx, _, _ = _exact(shape, "uniform")
    want_c, want_s, _ = td.accumulate_model(x, idx, mask, K)
    _assert_exact(_run(x, idx, K, view, False), want_c, want_s, f"{shape} non-contiguous mask")


# ------------------------------------------------------------------------------------------------
# indices outside [0, K)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", td.ACC_RANGE_SHAPES, ids=_ids)
def test_rows_with_an_index_outside_the_codebook_are_skipped(shape):
    H, M, K, D = shape
    seed = td.acc_seed(*shape)
    for exact in (True, False):
        x, idx = _exact(shape, "uniform")[:2] if exact else _float(shape)[:2]
        idx, hit = td.out_of_range_indices(idx, K, seed)
        assert 0.07 * H * M < int(hit.sum()) < 0.13 * H * M
        want_c, want_s, abs_s = td.accumulate_model(x, idx, None, K)
        assert int(want_c.sum()) == H * M - int(hit.sum())
        poisoned = torch.where(hit[..., None], torch.full_like(x, 1e30), x)
        for deterministic in ENTRIES:
            what = f"{shape} out-of-range {'exact' if exact else 'float'} deterministic={deterministic}"
            got = _run(x, idx, K, None, deterministic)
            if exact:
                _assert_exact(got, want_c, want_s, what)
            else:
                _assert_within_bound(got, want_c, want_s, abs_s, what)
            if exact or deterministic:  # (float atomics: only exact data are bit-identical from run to run)
                again = _run(poisoned, idx, K, None, deterministic)
                assert np.array_equal(_bits(again[0]), _bits(got[0])) and np.array_equal(_bits(again[1]), _bits(got[1])), what
            else:
                _assert_within_bound(_run(poisoned, idx, K, None, False), want_c, want_s, abs_s, what + " poisoned")


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
def _layout(kind, x, idx):
    """-> (x view, idx view) on the device, equal in value to (x, idx)."""
    H, M, D = x.shape
    xd, idd = x.to(DEV), idx.to(DEV)
    if kind == "rows_of_a_wider_tensor":  # [M, H, D + 8][..., :D].permute(1, 0, 2)
        buf = torch.full((M, H, D + 8), 7.5, device=DEV)
        buf[..., :D] = xd.permute(1, 0, 2)
        xv = buf[..., :D].permute(1, 0, 2)
        assert xv.stride() == (D + 8, H * (D + 8), 1)
    elif kind == "one_float_into_the_buffer":  # the base pointer is 4-byte aligned only: no float4 loads
        buf = torch.full((H * M * D + 1,), 7.5, device=DEV)
        buf[1:] = xd.reshape(-1)
        xv = buf[1:].view(H, M, D)
        assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    elif kind == "odd_row_stride":
        rs = D + 1 if D % 2 == 0 else D + 2
        buf = torch.full((H, M, rs), 7.5, device=DEV)
        buf[..., :D] = xd
        xv = buf[..., :D]
        assert xv.stride(1) % 2 == 1
    elif kind == "strided_indices":  # a slice of an [M, H, 3] tensor
        wide = torch.full((M, H, 3), -5, dtype=torch.int64, device=DEV)
        wide[..., 1] = idd.t()
        idd = wide[..., 1].permute(1, 0)
        assert idd.stride() == (3, 3 * H)
        xv = xd
    else:
        raise ValueError(kind)
    assert torch.equal(xv, xd) and torch.equal(idd.cpu(), idx)
    return xv, idd


@pytest.mark.parametrize("kind", ["rows_of_a_wider_tensor", "one_float_into_the_buffer", "odd_row_stride", "strided_indices"])
@pytest.mark.parametrize("shape", [(2, 4500, 70, 20), (1, 3000, 40, 5), (1, 2100, 2, 260), (2, 1000, 256, 64)], ids=_ids)
def test_layouts_equal_the_contiguous_call(shape, kind):
    H, M, K, D = shape
    native = _native()
    x, idx = _float(shape)[:2]
    xv, iv = _layout(kind, x, idx)
    a = native.ema_accumulate(xv, iv, K, None, deterministic=True)
    b = native.ema_accumulate(x.to(DEV), idx.to(DEV), K, None, deterministic=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    x, idx, want_c, want_s = _exact(shape, "uniform")
    xv, iv = _layout(kind, x, idx)
    got = native.ema_accumulate(xv, iv, K, None, deterministic=False)
    torch.cuda.synchronize()
    _assert_exact(got, want_c, want_s, f"{shape} {kind}")


# ------------------------------------------------------------------------------------------------
# the C entry points: += into what is there, inputs untouched, bad arguments
# ------------------------------------------------------------------------------------------------
def _raw(det, x, idx, mask, K, counts, sums, ws=None, ws_ptr=None, ws_bytes=None, shape=None):
    """vq_ema_accumulate_f32 / vq_ema_accumulate_det_f32 on contiguous device tensors, on the default stream -> rc."""
    lib = _native().load()
    H, M, D = shape if shape is not None else tuple(x.shape)
    args = (x.data_ptr(), D, M * D, idx.data_ptr(), 1, M, None if mask is None else mask.data_ptr(), H, M, K, D,
            None if counts is None else counts.data_ptr(), sums.data_ptr())
    with torch.cuda.device(DEV):
        if not det:
            return lib.vq_ema_accumulate_f32(*args, None)
        ptr = ws.data_ptr() if ws_ptr is None else ws_ptr
        return lib.vq_ema_accumulate_det_f32(*args, ptr, ws.numel() * 8 if ws_bytes is None else ws_bytes, None)


def _workspace(H, M, K, D, extra=0):
    with torch.cuda.device(DEV):
        need = int(_native().load().vq_ema_det_workspace_bytes(H, M, K, D))
    assert need > 0
    ws = torch.empty(((need + 15) // 16 * 2 + extra,), dtype=torch.float64, device=DEV)
    assert ws.data_ptr() % 16 == 0
    return ws, need


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("shape", [(2, 4500, 70, 20), (2, 1000, 256, 64)], ids=_ids)
def test_both_entry_points_add_into_the_existing_contents(shape, det):
    H, M, K, D = shape
    assert _takes_owner_kernel(*shape) == (M == 4500)
    x, idx = _exact(shape, "half_empty")[:2]
    mask = td.acc_mask(H, M, td.acc_seed(*shape)).to(torch.uint8)
    want_c, want_s, _ = td.accumulate_model(x, idx, mask, K)
    assert (want_c == 0).any()
    rng = np.random.default_rng(17)
    pre_c = rng.integers(0, 8, (H, K)).astype(np.float32)
    pre_s = rng.integers(0, 8, (H, K, D)).astype(np.float32) * np.float32(0.125)
    xd, idd, md = x.to(DEV), idx.to(DEV), mask.to(DEV)
    counts, sums = torch.from_numpy(pre_c).to(DEV), torch.from_numpy(pre_s).to(DEV)
    ws = _workspace(H, M, K, D)[0] if det else None
    for n in (1, 2):
        assert _raw(det, xd, idd, md, K, counts, sums, ws) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(counts), _bits(pre_c.astype(np.float64) + n * want_c))
        bad = np.argwhere(_bits(sums) != _bits(pre_s.astype(np.float64) + n * want_s))
        assert bad.size == 0, f"call {n}: {len(bad)} sums differ, the first at (head, code, column) {tuple(bad[0])}"
    assert torch.equal(xd.cpu(), x) and torch.equal(idd.cpu(), idx) and torch.equal(md.cpu(), mask)


def test_bad_arguments_are_refused_without_a_launch():
    lib = _native().load()
    H, M, K, D = 1, 3000, 40, 5
    x, idx = (t.to(DEV) for t in _exact((H, M, K, D), "uniform")[:2])
    counts = torch.full((H, K), 2.0, device=DEV)
    sums = torch.full((H, K, D), 2.0, device=DEV)
    ws, need = _workspace(H, M, K, D, extra=2)
    for det in (False, True):
        name = b"vq_ema_accumulate_det" if det else b"vq_ema_accumulate"
        for bad in ((H, M, D, 0), (H, M, 0, K), (0, M, D, K)):
            assert _raw(det, x, idx, None, bad[3], counts, sums, ws, shape=bad[:3]) == BADARG
            assert name in lib.vq_last_error()
        assert _raw(det, x, idx, None, K, None, sums, ws) == BADARG and name in lib.vq_last_error()
        # no rows: nothing to do, whatever the pointers
        assert _raw(det, x, idx, None, K, counts, sums, ws, shape=(H, 0, D)) == 0
    # the deterministic entry's workspace: one byte short, and 8-byte-misaligned with room to spare
    assert _raw(True, x, idx, None, K, counts, sums, ws, ws_bytes=need - 1) == BADARG
    assert b"vq_ema_det_workspace_bytes" in lib.vq_last_error()
    assert _raw(True, x, idx, None, K, counts, sums, ws, ws_ptr=ws.data_ptr() + 8, ws_bytes=need) == BADARG
    assert b"vq_ema_det_workspace_bytes" in lib.vq_last_error()
    torch.cuda.synchronize()
    assert bool((counts == 2.0).all()) and bool((sums == 2.0).all())
    # exactly the bytes the sizer names are enough
    assert _raw(True, x, idx, None, K, counts, sums, ws, ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert float(counts.sum()) == 2.0 * H * K + H * M


# ------------------------------------------------------------------------------------------------
# non-finite rows
# ------------------------------------------------------------------------------------------------
def _klass(a):
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 2, np.where(a == -np.inf, 1, 0)))


@pytest.mark.parametrize("deterministic", ENTRIES)
@pytest.mark.parametrize("shape", td.ACC_NONFINITE_SHAPES, ids=_ids)
def test_nonfinite_rows_reach_their_own_code_and_column_only(shape, deterministic):
    H, M, K, D = shape
    x, idx, _rows = td.nonfinite_inputs(H, M, K, D, td.acc_seed(*shape))
    want_c, want_s, abs_s = td.accumulate_model(x, idx, None, K)
    assert sorted(_klass(want_s)[~np.isfinite(want_s)].tolist()) == [1, 2, 3, 3]
    got = _run(x, idx, K, None, deterministic)
    assert np.array_equal(_klass(got[1].cpu().numpy()), _klass(want_s))
    _assert_within_bound(got, want_c, want_s, abs_s, f"{shape} non-finite deterministic={deterministic}",
                         where=np.isfinite(want_s))
