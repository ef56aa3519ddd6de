"""lq_quantize_kernel<D> at every D = 1 .. 16 (and lq_backward_kernel at every width C * d), through native.lq_quantize /
native.lq_backward and through the module, with the levels, tables and inputs of tests/lq_dense.py (levels_for,
default_tables / learned_tables, sweep_input; tests/test_lq_host.py checks that recipe on the CPU).

What is compared with what:
  * out and idx with the numpy fp32 model (lq_dense.quantize_np / indices_np), bit for bit on every row at every d: the
    model is the kernel's specification, the d >= 8 sum order t0, t4 .. t(d-1), t1, t2, t3 included.
  * out with fp64 on the rows whose two nearest table values differ by at least 1e-6 in distance: the selected value is the
    fp64 nearest and |out - q| <= 2^-23 max(|z|, |q|) (out = z + (q - z): two rounded operations, so out == q is not
    expected).  The share of rows left out is printed and capped at 1 %.
  * out with the torch fallback on the GPU, bitwise on every row; idx with the fallback on every row for d <= 7 and on the
    order-free rows (every term a whole number, codebook <= 2^24) for d >= 8, where torch's sum order is not pinned.  (At
    d = 6, C = 3, B = 3 with learned tables this comparison found the fallback, not the kernel, off the reference's CPU
    values on 4 of 20 007 rows: torch's GPU sum picks its order by shape and strides, so the module's codes_to_indices
    now adds the d <= 7 terms in the CPU order explicitly.)  With
    default tables at least 99 % of the rows must be order-free.  With learned tables no row is order-free (a CPU
    measurement, printed by the host test), so at d >= 8 their idx is compared with the fp32 model only and their out
    with the fallback.

No case's sub-row count is a multiple of 256 (the last workgroup is ragged), every case but the `small` one (201 sub-rows)
has 79 workgroups."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from lq_dense import (default_tables, indices_np, learned_tables, levels_for, nearest64, order_free, quantize_np, restate64,
                      smallest_gap, sweep_input)
from test_gpu_lq import count_native, fallback

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT32_MIN = -(2**31)
CANARY = -77.25
DIMS = list(range(1, 17))
LAYOUTS = ("cfirst", "clast_padded", "contig")
# (B, C) -> positions: B * P * C is 20011, 20013, 20013, 20007 sub-rows
POSITIONS = {(1, 1): 20011, (3, 1): 6671, (1, 3): 6671, (3, 3): 2223}


def _tables(d, variant):
    levels = levels_for(d)
    return default_tables(levels) if variant == "default" else learned_tables(levels, 100 + d)


def _flat(tabs):
    return torch.from_numpy(np.concatenate(tabs)).to(DEV)


def _same_bits(a, b):
    """Bitwise equality of two fp32 arrays, a NaN matching any NaN (the payload of a generated NaN is the machine's)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(np.uint32),
                                                                           np.where(nb, 0, b).view(np.uint32))


def _place(zc, layout, want_out=True):
    """zc [B, P, W] numpy -> (z on the GPU in `layout`, out view or None, the buffer that holds out or None)."""
    B, P, W = zc.shape
    zt = torch.from_numpy(zc).to(DEV)
    if layout == "cfirst":  # [B, W, P] seen as [B, P, W]: ps = 1, cs = P; out freshly allocated by the call
        z = zt.transpose(1, 2).contiguous().transpose(1, 2)
        assert W == 1 or z.stride() == (W * P, 1, P)
        return z, None, None
    if layout == "clast_padded":  # a slice of a padded buffer, out a slice of a second one filled with a canary
        buf = torch.full((B, P, W + 5), 3.0, device=DEV)
        buf[:, :, 3:3 + W] = zt
        obuf = torch.full((B, P, W + 5), CANARY, device=DEV)
        return buf[:, :, 3:3 + W], (obuf[:, :, 3:3 + W] if want_out else None), obuf
    obuf = torch.full((B, W, P), CANARY, device=DEV)  # contiguous z, the caller's channel-first view as out
    return zt, (obuf.transpose(1, 2) if want_out else None), obuf


def _canary_intact(obuf, W):
    if obuf is None or obuf.shape[-1] != W + 5:
        return True
    return bool((obuf[:, :, :3] == CANARY).all()) and bool((obuf[:, :, 3 + W:] == CANARY).all())


def _order_free_or_nan(codes, levels):
    return order_free(codes, levels) | np.isnan(codes).any(axis=-1)


_MODULE = {}


def _module(d, C, tabs):
    """LatentQuantize(levels_for(d), dim = C * d, num_codebooks = C) on the GPU with `tabs` as its tables (one module is
    kept: the codebook of d = 16 has two million rows)."""
    from vector_quantization import LatentQuantize

    if _MODULE.get("key") != (d, C):
        _MODULE.clear()
        _MODULE.update(key=(d, C), mod=LatentQuantize(levels=levels_for(d), dim=C * d, num_codebooks=C).to(DEV))
    mod = _MODULE["mod"]
    with torch.no_grad():
        for p, t in zip(mod.values_per_latent, tabs):
            p.copy_(torch.from_numpy(np.asarray(t)))
        mod.commitment_loss_weight.fill_(0.1)
        mod.quantization_loss_weight.fill_(0.1)
    return mod.eval()


def _check_fp64(z4, tabs, got4, sel, what):
    """z4, got4 [..., d]: on the rows that clear every tie by 1e-6 the selected value is the fp64 nearest and out is within
    two roundings of it."""
    gap = smallest_gap(z4, [np.unique(t) for t in tabs])
    rows = gap >= 1e-6
    left_out = 1.0 - float(rows.mean())
    print(f"{what}: {left_out:.4%} of rows within 1e-6 of a tie")
    assert left_out <= 0.01
    q64 = nearest64(z4, tabs)
    picked = np.stack([np.asarray(t, dtype=np.float64)[sel[..., i]] for i, t in enumerate(tabs)], axis=-1)
    assert np.array_equal(picked[rows], q64[rows]), "the selected value is not the fp64 nearest"
    err = np.abs(got4.astype(np.float64) - q64)[rows]
    bound = 2.0**-23 * np.maximum(np.abs(z4.astype(np.float64)), np.abs(q64))[rows]
    print(f"{what}: largest |out - q64| / bound = {float((err / np.maximum(bound, 1e-300)).max(initial=0.0)):.3f}")
    assert (err <= bound).all()


_NATIVE_CASES = [(d, layout, C, B, variant, False) for d in DIMS for layout in LAYOUTS for C in (1, 3) for B in (1, 3)
                 for variant in ("default", "learned")] + [(d, "clast_padded", 3, 1, "learned", True) for d in DIMS]


def _case_id(c):
    d, layout, C, B, variant, small = c
    return f"d{d}-{layout}-C{C}-B{B}-{variant}" + ("-small" if small else "")


@pytest.mark.parametrize("case", _NATIVE_CASES, ids=_case_id)
def test_native_against_fp32_model_and_fp64(case):
    from vector_quantization import native

    d, layout, C, B, variant, small = case
    levels = levels_for(d)
    tabs = _tables(d, variant)
    P = 67 if small else POSITIONS[(B, C)]
    N = B * P * C
    assert N % 256 != 0 and (small and N < 256 or N > 3 * 256)
    W = C * d
    zc = sweep_input(B * P, W, 1000 * d + 10 * C + B).reshape(B, P, W)
    z, out, obuf = _place(zc, layout)
    got, idx, loss = native.lq_quantize(z, levels, _flat(tabs), C, out=out)
    assert loss is None and idx.shape == (B, P, C) and idx.dtype == torch.int32 and got.shape == (B, P, W)
    if out is not None:
        assert got.data_ptr() == out.data_ptr() and got.stride() == out.stride()
    assert _canary_intact(obuf, W)
    z4 = zc.reshape(B, P, C, d)
    codes, sel = quantize_np(z4, tabs)
    got4 = got.cpu().numpy().reshape(B, P, C, d)
    assert np.array_equal(got4.view(np.uint32), codes.view(np.uint32)), "out differs from the fp32 model"
    assert np.array_equal(idx.cpu().numpy(), indices_np(codes, levels)), "idx differs from the fp32 model"
    _check_fp64(z4, tabs, got4, sel, _case_id(case))


@pytest.mark.parametrize("case", [(d, C, B, variant) for d in DIMS for C in (1, 3) for B in (1, 3)
                                  for variant in ("default", "learned")], ids=lambda c: f"d{c[0]}-C{c[1]}-B{c[2]}-{c[3]}")
def test_module_against_fallback(case):
    d, C, B, variant = case
    levels = levels_for(d)
    tabs = _tables(d, variant)
    P = POSITIONS[(B, C)]
    W = C * d
    zc = sweep_input(B * P, W, 1000 * d + 10 * C + B).reshape(B, P, W)
    x = torch.from_numpy(zc).to(DEV).transpose(1, 2).contiguous()  # [B, C * d, P], as the module takes it
    mod = _module(d, C, tabs)
    with torch.no_grad():
        with count_native() as calls:
            out, idx, loss = mod(x)
        assert len(calls["lq_quantize"]) == 1
        with fallback(), count_native() as calls:
            want, want_idx, _ = mod(x)
        assert "lq_quantize" not in calls
    assert out.shape == x.shape and idx.shape == want_idx.shape and idx.dtype == want_idx.dtype == torch.int32
    assert float(loss) == 0.0
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "out differs from the fallback"
    codes, _ = quantize_np(zc.reshape(B, P, C, d), tabs)
    gi, wi = idx.cpu().numpy().reshape(B, P, C), want_idx.cpu().numpy().reshape(B, P, C)
    assert np.array_equal(gi, indices_np(codes, levels)), "idx differs from the fp32 model"
    keep = np.ones((B, P, C), dtype=bool) if d <= 7 else order_free(codes, levels)
    print(f"d{d} C{C} B{B} {variant}: {int((gi != wi).sum())} of {gi.size} indices differ from the fallback, "
          f"{1 - keep.mean():.4%} of rows not compared")
    if variant == "default":
        assert keep.mean() >= 0.99
    assert np.array_equal(gi[keep], wi[keep]), "idx differs from the fallback"


def _edge_rows(d, tabs, seed):
    """[P, d]: in dimension 0 and in dimension d - 1, one row on every table value and one on the midpoint of every pair of
    values adjacent in sorted order, the other dimensions random; then NaN, +inf, -inf each alone in dimension d - 1.
    -> (z, the (row, dim, value a, value b) of the midpoint rows)."""
    rows, mids = [], []
    base = sweep_input(4 * sum(len(t) for t in tabs) + 16, d, seed)
    n = 0
    for dim in sorted({0, d - 1}):
        tab = np.asarray(tabs[dim], dtype=np.float32)
        for v in tab:
            r = base[n].copy()
            r[dim] = v
            rows.append(r)
            n += 1
        s = np.unique(tab)
        for a, b in zip(s[:-1], s[1:]):
            r = base[n].copy()
            r[dim] = np.float32((np.float64(a) + np.float64(b)) / 2)
            mids.append((n, dim, a, b))
            rows.append(r)
            n += 1
    for v in (np.nan, np.inf, -np.inf):
        r = base[n].copy()
        r[d - 1] = v
        rows.append(r)
        n += 1
    return np.stack(rows).astype(np.float32), mids


@pytest.mark.parametrize("variant", ["default", "learned", "nan_in_last_table"])
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_ties_table_values_and_nonfinite(d, variant):
    """Inputs exactly on every table value and on every midpoint, in the first and in the last dimension, and NaN / +inf /
    -inf in the last dimension, against the fp32 model and the fallback; where the two fp32 distances of a midpoint are
    equal, the value that comes first in table order wins.  nan_in_last_table: a NaN distance is the minimum, so every
    row's last value is NaN and every index INT32_MIN."""
    from vector_quantization import native

    levels = levels_for(d)
    tabs = _tables(d, "default" if variant == "default" else "learned")
    if variant == "nan_in_last_table":
        tabs[-1][min(1, len(tabs[-1]) - 1)] = np.nan
    clean = [t[~np.isnan(t)] for t in tabs]
    ze, mids = _edge_rows(d, clean, 7000 + d)
    P = ze.shape[0]
    zc = ze[None]
    codes, sel = quantize_np(zc, tabs)
    want_idx = indices_np(codes, levels)
    for layout in ("cfirst", "clast_padded"):
        z, out, obuf = _place(zc, layout)
        got, idx, _ = native.lq_quantize(z, levels, _flat(tabs), 1, out=out)
        assert _same_bits(got.cpu().numpy(), codes), f"{layout}: out differs from the fp32 model"
        assert np.array_equal(idx.cpu().numpy()[..., 0], want_idx), f"{layout}: idx differs from the fp32 model"
        assert _canary_intact(obuf, d)
    g = got.cpu().numpy()[0]
    # the rows on a table value return it exactly (q - z = 0)
    n = 0
    for dim in sorted({0, d - 1}):
        if not (variant == "nan_in_last_table" and dim == d - 1):
            for v in clean[dim]:
                assert g[n, dim] == v
                n += 1
            n += len(np.unique(clean[dim])) - 1
    ties = 0
    for row, dim, a, b in mids:
        if variant == "nan_in_last_table" and dim == d - 1:
            continue
        zv = ze[row, dim]
        if np.abs(np.float32(zv - a)) == np.abs(np.float32(zv - b)):
            tab = list(tabs[dim])
            first = a if tab.index(a) < tab.index(b) else b
            assert g[row, dim] == np.float32(zv + np.float32(first - zv)), (row, dim, a, b)
            ties += 1
    print(f"d{d} {variant}: {ties} of {len(mids)} midpoints are exact fp32 ties")
    if variant == "default" and d >= 8:
        assert ties == len(mids)  # dyadic tables: every midpoint is exact
    nan_rows = np.isnan(codes[0]).any(axis=-1)
    assert nan_rows[-3:].all() and (want_idx[0][nan_rows] == INT32_MIN).all()
    if variant == "nan_in_last_table":
        assert nan_rows.all() and np.isnan(g[:, d - 1]).all()
    # the module against the fallback
    mod = _module(d, 1, tabs)
    x = torch.from_numpy(zc).to(DEV).transpose(1, 2).contiguous()
    with torch.no_grad():
        out, idx, _ = mod(x)
        with fallback():
            want, widx, _ = mod(x)
    assert _same_bits(out.cpu().numpy(), want.cpu().numpy()), "out differs from the fallback"
    gi, wi = idx.cpu().numpy()[0], widx.cpu().numpy()[0]
    assert np.array_equal(gi, want_idx[0])
    if d <= 7:
        keep = np.ones(P, dtype=bool)
    elif variant == "default":
        keep = _order_free_or_nan(codes[0], levels)
        assert keep.mean() >= 0.99
    else:
        keep = nan_rows  # learned tables at d >= 8: only the NaN rows' index is independent of the sum order
    assert np.array_equal(gi[keep], wi[keep]), "idx differs from the fallback"


@pytest.mark.parametrize("levels", [[4096], [2048, 2048], [4092, 2, 2]], ids=lambda v: "x".join(map(str, v)))
def test_table_cap_is_fused(levels):
    """sum(levels) = 4096 floats, the LDS table's cap, takes the fused path; inputs lie on every table value, so the last
    float of the staged tables is selected."""
    from vector_quantization import LatentQuantize, native

    d = len(levels)
    assert sum(levels) == 4096
    tabs = default_tables(levels)
    P = max(levels) + 37
    zc = sweep_input(P, d, 31 + d)[None].copy()
    for i, t in enumerate(tabs):
        zc[0, :len(t), i] = t
    codes, sel = quantize_np(zc, tabs)
    assert (sel[..., d - 1] == levels[-1] - 1).any() and (sel[..., 0] == levels[0] - 1).any()
    z, out, obuf = _place(zc, "clast_padded")
    got, idx, _ = native.lq_quantize(z, levels, _flat(tabs), 1, out=out)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), codes.view(np.uint32)) and _canary_intact(obuf, d)
    assert np.array_equal(idx.cpu().numpy()[..., 0], indices_np(codes, levels))
    mod = LatentQuantize(levels=levels, dim=d).to(DEV).eval()
    x = torch.from_numpy(zc).to(DEV).transpose(1, 2).contiguous()
    with torch.no_grad():
        with count_native() as calls:
            o, i, _ = mod(x)
        assert len(calls["lq_quantize"]) == 1
        with fallback():
            want, widx, _ = mod(x)
    assert torch.equal(o.view(torch.int32), want.view(torch.int32)) and torch.equal(i, widx)


def test_table_above_the_cap_takes_the_fallback():
    from vector_quantization import LatentQuantize, native

    levels = [4097]
    tabs = default_tables(levels)
    zc = sweep_input(4097 + 36, 1, 5)[None].copy()
    zc[0, :4097, 0] = tabs[0]
    mod = LatentQuantize(levels=levels, dim=1).to(DEV).eval()
    x = torch.from_numpy(zc).to(DEV).transpose(1, 2).contiguous()
    with torch.no_grad(), count_native() as calls:
        out, idx, _ = mod(x)
    assert "lq_quantize" not in calls
    codes, _ = quantize_np(zc, tabs)
    assert np.array_equal(out.cpu().numpy()[0, 0].view(np.uint32), codes[0, :, 0].view(np.uint32))
    assert np.array_equal(idx.cpu().numpy()[0], indices_np(codes, levels)[0])
    with pytest.raises(RuntimeError, match="4096"):
        native.lq_quantize(torch.from_numpy(zc).to(DEV), levels, _flat(tabs))


def _loss_want(w_c, w_q, m):
    """loss[0] from the kernel's own mean m, formed in fp32: a zero weight multiplies 0, not m."""
    w_c, w_q, m = np.float32(w_c), np.float32(w_q), np.float32(m)
    with np.errstate(invalid="ignore", over="ignore"):
        lc = np.float32(w_c * (m if w_c != 0 else np.float32(0)))
        lq = np.float32(w_q * (m if w_q != 0 else np.float32(0)))
        return np.float32(lc + lq)


def _with_last(zc, value):
    """zc [B, P, W] with its very last element replaced, on the GPU as a channel-first view."""
    zb = zc.copy()
    zb[-1, -1, -1] = value
    return _place(zb, "cfirst")[0]


@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_loss_partials_with_a_ragged_last_block(d):
    """79 per-workgroup partials, the last workgroup holding 45 sub-rows: loss[1] against the fp64 mean of (c - z)^2 over
    the fp32 model's c, within the 2^-18 relative bound test_gpu_lq.py::test_fixture derives for this reduction; loss[0]
    equal to w_c * m + w_q * m formed in fp32; with one weight zero and a non-finite mean, the zero weight multiplies 0."""
    from vector_quantization import native

    levels = levels_for(d)
    tabs = _tables(d, "learned")
    B, C, P = 1, 3, POSITIONS[(1, 3)]
    W = C * d
    zc = sweep_input(P, W, 500 + d).reshape(B, P, W)
    z, _, _ = _place(zc, "cfirst")
    got, idx, loss = native.lq_quantize(z, levels, _flat(tabs), C, loss_weights=(0.25, 0.1))
    codes, _ = quantize_np(zc.reshape(B, P, C, d), tabs)
    assert np.array_equal(got.cpu().numpy().reshape(codes.shape).view(np.uint32), codes.view(np.uint32))
    m64 = float(((codes.astype(np.float64) - zc.reshape(codes.shape).astype(np.float64)) ** 2).mean())
    l0, m = (np.float32(v) for v in loss.cpu().numpy())
    print(f"d{d}: loss[1] {float(m)!r} fp64 {m64!r} relative distance {abs(float(m) - m64) / m64:.3e} (bound {2.0**-18:.3e})")
    assert abs(float(m) - m64) <= 2.0**-18 * m64
    assert l0 == _loss_want(0.25, 0.1, m) and np.isfinite(l0)
    # a non-finite mean: an inf input makes it NaN, an input of 1e30 makes it +inf (c = 0, (c - z)^2 overflows)
    for bad, mean_is in ((np.inf, np.isnan), (1e30, np.isposinf)):
        zt = _with_last(zc, bad)
        for w_c, w_q in ((0.0, 0.1), (0.25, 0.0), (0.0, 0.0)):
            _, _, loss = native.lq_quantize(zt, levels, _flat(tabs), C, loss_weights=(w_c, w_q))
            l0, m = (np.float32(v) for v in loss.cpu().numpy())
            assert mean_is(m), (bad, m)
            want = _loss_want(w_c, w_q, m)
            assert (np.isnan(l0) and np.isnan(want)) or l0 == want, (bad, w_c, w_q, l0, want)
            if bad == 1e30:
                assert l0 == (0.0 if w_c == w_q == 0.0 else np.inf)  # 0 * inf would have been NaN
    # the module's fused loss follows the fallback's on the +inf mean
    mod = _module(d, C, tabs).train()
    try:
        with torch.no_grad():
            mod.commitment_loss_weight.fill_(0.0)
            x = _with_last(zc, 1e30).transpose(1, 2)
            _, _, lf = mod(x)
            with fallback():
                _, _, lw = mod(x)
        assert float(lf) == float(lw) == float("inf")
    finally:
        mod.eval()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64], ids=["bf16", "fp16", "fp64"])
@pytest.mark.parametrize("d", [6, 7], ids=lambda d: f"d{d}")
def test_fallback_indices_of_other_dtypes_keep_torch_sum(d, dtype):
    """codes_to_indices pins the order of the sum for fp32 terms only.  torch.sum accumulates bf16 / fp16 terms in fp32 and
    rounds once, so a chain of half-precision additions would leave the reference's values; fp64 keeps torch.sum as well.
    Learned fp32 tables cast to `dtype`, three codebooks on channel-first rows: the index is that of torch.sum on every
    row."""
    levels = levels_for(d)
    tabs = _tables(d, "learned")
    mod = _module(d, 3, tabs)
    B, C, P = 3, 3, POSITIONS[(3, 3)]
    z, _, _ = _place(sweep_input(B * P, C * d, 950 + d).reshape(B, P, C * d), "cfirst")
    codes, _ = quantize_np(z.cpu().numpy().reshape(B, P, C, d), tabs)
    zhat = torch.from_numpy(codes).to(DEV).to(dtype).transpose(1, 2).contiguous().transpose(1, 2)
    with count_native() as calls:
        got = mod.codes_to_indices(zhat)
    assert not calls
    index = (mod._scale_and_shift(zhat) * mod._basis).sum(dim=-1)
    assert index.dtype == dtype and got.dtype == torch.int32
    assert torch.equal(got, index.to(torch.int32))


def _strided3(a, kind):
    """a [B, P, W] numpy -> the same values on the GPU in one of three layouts."""
    z, _, _ = _place(a, kind)
    return z


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_backward_native(d, C):
    """lq_backward_kernel at W = C * d with three differently strided operands, bit for bit the fp32 restatement
    gv + (g_loss * coef) * (ov - xv) (three rounded operations after the product k = g_loss * coef), and within
    2^-22 |want| + 2^-22 max|k (ov - xv)| of fp64."""
    from vector_quantization import native

    B, P, W = 3, 1777, C * d
    x = sweep_input(B * P, W, 900 + d).reshape(B, P, W)
    ov = sweep_input(B * P, W, 901 + d).reshape(B, P, W)
    gv = sweep_input(B * P, W, 902 + d).reshape(B, P, W)
    g_loss, coef = np.float32(1.7), 0.37
    gbuf = torch.full((B, P, W + 5), CANARY, device=DEV)
    got = native.lq_backward(_strided3(x, "cfirst"), _strided3(ov, "clast_padded"), _strided3(gv, "contig"),
                             torch.tensor(g_loss, device=DEV), coef, grad_x=gbuf[:, :, 3:3 + W])
    assert _canary_intact(gbuf, W) and got.data_ptr() == gbuf[:, :, 3:3 + W].data_ptr()
    k = np.float32(g_loss * np.float32(coef))
    want = (gv + (k * (ov - x).astype(np.float32)).astype(np.float32)).astype(np.float32)
    g = got.cpu().numpy()
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
    k64 = float(g_loss) * float(np.float32(coef))
    t64 = k64 * (ov.astype(np.float64) - x.astype(np.float64))
    w64 = gv.astype(np.float64) + t64
    assert (np.abs(g - w64) <= 2.0**-22 * np.abs(w64) + 2.0**-22 * np.abs(t64).max()).all()
    # grad_x left to the call: laid out as x
    got2 = native.lq_backward(_strided3(x, "cfirst"), _strided3(ov, "contig"), _strided3(gv, "clast_padded"),
                              torch.tensor(g_loss, device=DEV), coef)
    assert (W == 1 or got2.stride() == (W * P, 1, P)) and torch.equal(got2, got)


@pytest.mark.parametrize("d", [2, 9, 16], ids=lambda d: f"d{d}")
def test_module_backward_with_unequal_weights(d):
    """Weights 0.25 / 0.1, so that lq_backward_kernel launches, against the fp64 restatement's gradient (rtol 1e-5, atol
    1e-6, the bound of test_gpu_lq.py::test_fused_equals_fallback)."""
    levels = levels_for(d)
    tabs = _tables(d, "learned")
    B, C, P = 3, 1, 2223
    x0 = sweep_input(B * d, P, 40 + d).reshape(B, d, P)
    r = sweep_input(B * d, P, 41 + d).reshape(B, d, P)
    mod = _module(d, C, tabs).train()
    try:
        with torch.no_grad():
            mod.commitment_loss_weight.fill_(0.25)
        x = torch.from_numpy(x0).to(DEV).requires_grad_(True)
        with count_native() as calls:
            out, idx, loss = mod(x)
            ((out * torch.from_numpy(r).to(DEV)).sum() + loss).backward()
        assert len(calls["lq_quantize"]) == 1 and len(calls["lq_backward"]) == 1
    finally:
        mod.eval()
    kw = dict(levels=levels, dim=d, commitment_loss_weight=0.25, quantization_loss_weight=0.1)
    st = restate64(kw, {}, x0, r, True, tabs)
    np.testing.assert_allclose(x.grad.cpu().numpy(), st["grad"].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(loss.detach()), float(st["loss"]), rtol=1e-5)


def test_two_d13_training_steps_bitwise_equal():
    d = 13
    mod = _module(d, 1, _tables(d, "learned")).train()
    try:
        with torch.no_grad():
            mod.commitment_loss_weight.fill_(0.25)
        x0 = torch.from_numpy(sweep_input(3 * d, 20011, 77).reshape(3, d, 20011)).to(DEV)
        res = []
        for _ in range(2):
            x = x0.clone().requires_grad_(True)
            with count_native() as calls:
                out, idx, loss = mod(x)
                ((out * out).sum() + loss).backward()
            assert len(calls["lq_backward"]) == 1
            res.append((out.detach(), idx, loss.detach(), x.grad))
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        mod.eval()
