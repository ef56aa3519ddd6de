"""GPU: vq_finalize_kernel (csrc/vq_finalize_ema.inc) alone, fed with keys packed on the host, against an exact reference.

The kernel ends every K-split quantize, every sharded step and the replicated gather: per row the MIN over the candidate key
planes, the decode into (value, index), the gather of the code row, optionally the straight-through value x + (c - x), and the
squared error that vq_loss_reduce_kernel sums in double.  Here the keys come from oracle.pack_key, so no search kernel is
involved, and the reference is helpers.finalize_reference:

    key  = planes.min(axis=0)                      # int64, signed
    idx  = key & 0xFFFFFFFF ; best = unpack_key(key, metric)[0]
    q    = cb[h, idx]                              # exact gather
    out  = x + (q - x) in float32 if ste else q    # one rounding each
    sq   = sum((q.astype(f64) - x.astype(f64))**2) # over all heads

idx, best and out (with and without straight-through) are compared bit for bit (NaN positions as masks, the sign of zero
included: nothing in the kernel's straight-through path can be contracted into an FMA); sq_err within
helpers.finalize_sq_err_bound, (L R + 9) 2^-24 relative, which is derived from the kernel's arithmetic and not measured.
Every key carries an index < K and every row has at least one real key: the kernel gathers whatever index wins.

Which branch each group pins:

1. test_plane_min_and_key_decode -- the planes loop `for (cnd = lane; cnd < nparts; cnd += 64)` with fewer than, exactly and more
   than 64 planes, the 64-lane butterfly on long long, the `nparts == 1` branch that reads plane 0 directly ([H, M] and
   [1, H, M] keys), key_value for both metrics (NaN, infinities, signed zeros, a subnormal), the low-32-bit index above 65535,
   the signed MIN order against the init plane value, lowest GLOBAL index on equal values.  The winner sits in plane 0, 63, 64,
   P - 1 or a random one by construction.
2. test_gather_ste_and_squared_error -- the scalar loop (`p.vec == 0`, 64-lane stride) and the float4 loop (256-element
   stride) with and without `need_x`: gather, `quant = r + diff`, the fmaf chain of the squared error, `out` null (loss only).
3. test_views_strides_and_alignment, test_sharded_overlap_calling_convention -- run_finalize's `vec` decision (D, strides, base
   alignment of cb / out, and of x only when x is read), out / x / idx / best as views of larger buffers (row stride of idx
   and best other than 1), nothing written outside a view; the sharded step's overlap branch called the way sharded.py calls it.
4. test_row_cap_and_loss_partials, test_no_rows -- more rows than 2048 workgroups x 4 waves (each wave strides over 2 or 3
   rows, its squared-error chain running on), the loss partials filling H x 8192 floats of the workspace, and M = 0.
5. test_finalize_rejects_bad_arguments -- the argument checks of vq_finalize_key_planes_f32, which launch nothing.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from helpers import finalize_reference, finalize_rows_per_wave, finalize_sq_err_bound, same_values

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EUCLID, DOT = 0, 1
KEY_INIT = np.int64(0x7FFFFFFFFFFFFFFF)  # what vq_keys_init writes: worse than every real key
SENT, ISENT = 7777.0, -7                 # what destination buffers hold before a call
NAN, INF = float("nan"), float("inf")
# best -> worst.  Euclid: NaN beats 0, +inf beats the init value.  Dot: NaN beats +inf, +0.0 beats -0.0, -inf beats the init value.
VALUES = {EUCLID: np.array([NAN, 0.0, 1e-40, 1.5, INF], dtype=np.float32),
          DOT: np.array([NAN, INF, 2.0, 0.0, -0.0, -1.0, -INF], dtype=np.float32)}
WORST = dict(scalar=0.0, vector=0.0)


def _native():
    from vector_quantization import native

    native.load()
    return native


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _finalize(native, x, cb, keys, **kw):
    r = native.finalize_keys(x, cb, keys, **kw)
    torch.cuda.synchronize()
    return r


def _assert_idx_best(label, idx, best, want_idx, want_best):
    assert np.array_equal(idx.cpu().numpy(), want_idx), f"{label}: idx"
    assert same_values(best.cpu().numpy(), want_best), f"{label}: best"


def _vec4(t: torch.Tensor, *strides) -> bool:
    return t.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in strides)


def _expect_vec(D, cb, out, x, need_x) -> bool:
    """The path run_finalize must choose: float4 accesses need D % 4 == 0 and, for cb, out and -- only when it is read -- x,
    a 16-byte aligned base and row / head strides that are multiples of 4 floats."""
    ok = D % 4 == 0 and _vec4(cb, cb.stride(0))
    if out is not None:
        ok = ok and _vec4(out, out.stride(1), out.stride(0))
    if need_x:
        ok = ok and _vec4(x, x.stride(1), x.stride(0))
    return ok


def _sq_ratio(label, got: float, want: float, D: int, M: int, vec: bool) -> float:
    """error / bound of a finite squared-error sum (asserted <= 1); non-finite: the same NaN / inf class as the fp64 sum."""
    if not math.isfinite(want):
        assert math.isnan(got) == math.isnan(want) and math.isinf(got) == math.isinf(want), f"{label}: sq_err {got} vs {want}"
        assert not math.isinf(want) or got > 0, f"{label}: sq_err {got} vs {want}"
        return 0.0
    assert want > 0.0 and math.isfinite(got), f"{label}: sq_err {got} vs {want}"
    ratio = abs(got - want) / want / finalize_sq_err_bound(D, M, vec)
    path = "vector" if vec else "scalar"
    WORST[path] = max(WORST[path], ratio)
    assert ratio <= 1.0, f"{label}: sq_err {got!r} vs {want!r}: error / bound = {ratio:.3f} on the {path} path"
    return ratio


def _report(label, ratios):
    """ratios: (vec, ratio) pairs of one test case"""
    parts = []
    for vec, path in ((False, "scalar"), (True, "vector")):
        mine = [r for v, r in ratios if v == vec]
        if mine:
            parts.append(f"{path} path (L = {'4 ceil(D/256)' if vec else 'ceil(D/64)'}) worst of {len(mine)}: {max(mine):.3f}")
    print(f"finalize sq_err {label}: error / bound " + "; ".join(parts)
          + f" (worst so far scalar {WORST['scalar']:.3f} vector {WORST['vector']:.3f})")


# ------------------------------------------------------------------------------------------------ 1. plane MIN and key decode
@functools.lru_cache(maxsize=None)
def _codes(H: int, K: int, D: int, seed: int = 5):
    cb = np.random.default_rng(seed + H).standard_normal((H, K, D)).astype(np.float32)
    return cb, _dev(cb)


def _plane_case(oracle, metric, H, M, P, K, seed):
    """-> planes [P, H, M], and per row the winner's index and value.  By construction: the winner of a row sits in plane 0, 63,
    64, P - 1 (where they exist) or a random plane; a third of the rows carry the winner's VALUE a second time with a HIGHER
    index, in an earlier plane wherever there is one; every other plane holds a strictly worse value with any index (lower
    ones included) or the init value."""
    g = np.random.default_rng(seed)
    vals = VALUES[metric]
    nv, n = len(vals), H * M
    cols = np.arange(n)
    r = cols + seed  # rotates the scenarios, so that the few rows of a small M differ from case to case
    slots = np.array(list(dict.fromkeys(p for p in (0, 63, 64, P - 1) if p < P)))
    sel = r % (len(slots) + 1)
    w = np.where(sel < len(slots), slots[np.minimum(sel, len(slots) - 1)], g.integers(0, P, n))
    v = (r // (len(slots) + 1)) % nv
    wi = np.where(r % 2 == 0, g.integers(65536, K - 1, n), g.integers(0, K - 1, n))  # <= K - 2: room for a higher index
    wi[r % 11 == 0] = 0
    worse = v[None, :] + 1 + g.integers(0, nv, (P, n))
    empty = (worse >= nv) | (g.random((P, n)) < 0.4)
    planes = np.where(empty, KEY_INIT, oracle.pack_key(vals[np.minimum(worse, nv - 1)], g.integers(0, K, (P, n)), metric))
    if P > 1:
        tie = r % 3 == 0
        t = np.where(w > 0, g.integers(0, np.maximum(w, 1)), g.integers(1, P, n))
        ti = wi + 1 + g.integers(0, K - 1 - wi)
        planes[t[tie], cols[tie]] = oracle.pack_key(vals[v], ti, metric)[tie]
        # a winner in plane 64 or beyond always has a real, losing key among the first 64 planes (a worse value; for the worst
        # value the same one with a higher index): a kernel that lost the late planes would be wrong, and still gather in bounds
        guard = w >= 64
        gk = oracle.pack_key(vals[np.minimum(v + 1, nv - 1)], np.where(v + 1 < nv, g.integers(0, K, n), ti), metric)
        planes[g.integers(0, 64, n)[guard], cols[guard]] = gk[guard]
    planes[w, cols] = oracle.pack_key(vals[v], wi, metric)
    assert int((planes & np.int64(0xFFFFFFFF))[planes != KEY_INIT].max()) < K
    return planes.reshape(P, H, M), wi.reshape(H, M), vals[v].reshape(H, M)


@pytest.mark.parametrize("P", [1, 2, 3, 63, 64, 65, 128, 130, 200])
@pytest.mark.parametrize("metric", [EUCLID, DOT])
def test_plane_min_and_key_decode(oracle, metric, P):
    native = _native()
    K, D = 70000, 4
    for H in (1, 3):
        cb_np, cb = _codes(H, K, D)
        for M in (1, 3, 4, 5, 261):
            label = f"metric={metric} P={P} H={H} M={M}"
            planes, wi, wv = _plane_case(oracle, metric, H, M, P, K, seed=1000 * P + 10 * M + H)
            x_np = np.full((H, M, D), NAN, dtype=np.float32)  # neither flag reads x
            want_idx, want_best, want_out, _ = finalize_reference(planes, cb_np, x_np, metric, False)
            assert np.array_equal(want_idx, wi) and same_values(want_best, wv), f"{label}: the planes are not what they claim"
            x = _dev(x_np)
            for keys in ([planes] if P > 1 else [planes, planes[0]]):  # [P, H, M]; one plane also as [H, M]
                r = _finalize(native, x, cb, _dev(keys), metric=metric)
                _assert_idx_best(f"{label} keys{list(keys.shape)}", r["idx"], r["best"], want_idx, want_best)
                assert same_values(r["out"].cpu().numpy(), want_out), f"{label}: out"


# ------------------------------------------------------------------------- 2. gather, straight-through, squared error, both paths
FLAGS = [(False, False, True), (True, False, True), (False, True, True), (True, True, True), (False, True, False)]


_ARITH = {}


def _arith_data(oracle, D: int, finite: bool, H: int = 2, M: int = 7, K: int = 9):
    """Generated once per (D, half) and reused for every flag combination.  Rows 0, 2, 4, 6 have |x| ~ 1e4 against |c| ~ 1e-3, so
    x + (c - x) != c; codes 2 and 5 contain -0.0; the non-finite half has a NaN in one row of x and a +inf in one code."""
    if (D, finite) in _ARITH:
        return _ARITH[D, finite]
    g = np.random.default_rng(31 * D + (0 if finite else 7919))
    x = g.standard_normal((H, M, D)).astype(np.float32)
    x[:, ::2] *= np.float32(1e4)
    cb = (g.standard_normal((H, K, D)) * 1e-3).astype(np.float32)
    cb[:, [2, 5], ::3] = -0.0
    if not finite:
        x[0, 3, D // 2] = NAN
        cb[1, 4, D - 1] = INF
    metric = D % 2
    idx = (np.arange(M)[None, :] + 2 * np.arange(H)[:, None] + 1) % K  # head 0: codes 1..7, head 1: codes 3..8, 0
    key = oracle.pack_key(np.abs(g.standard_normal((H, M))).astype(np.float32), idx, metric)
    if D % 2:  # odd D: two planes, the real key of a row in either
        first = (np.arange(M)[None, :] + np.arange(H)[:, None]) % 2 == 0
        planes = np.stack([np.where(first, key, KEY_INIT), np.where(first, KEY_INIT, key)])
    else:
        planes = key[None]
    _ARITH[D, finite] = (x, cb, planes, metric)
    return _ARITH[D, finite]


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 63, 64, 65, 100, 255, 256, 257, 260, 1024, 1028, 1030])
def test_gather_ste_and_squared_error(oracle, D):
    native = _native()
    ratios = []
    for finite in (True, False):
        x_np, cb_np, planes, metric = _arith_data(oracle, D, finite)
        H, M, _ = x_np.shape
        x, cb = _dev(x_np), _dev(cb_np)
        keys = _dev(planes if planes.shape[0] > 1 else planes[0])
        refs = {ste: finalize_reference(planes, cb_np, x_np, metric, ste) for ste in (False, True)}
        # a condition on the DATA: straight-through must be distinguishable from the plain gather
        differ = refs[True][2].view(np.uint32) != refs[False][2].view(np.uint32)
        assert differ.mean() >= 0.25, differ.mean()
        assert np.signbit(refs[False][2][refs[False][2] == 0.0]).any(), "no -0.0 reaches the output"
        for ste, want_sq, want_out in FLAGS:
            label = f"D={D} finite={finite} ste={ste} sq_err={want_sq} out={want_out}"
            want_idx, want_best, want, sq64 = refs[ste]
            r = _finalize(native, x, cb, keys, metric=metric, ste=ste, want_sq_err=want_sq, want_out=want_out)
            _assert_idx_best(label, r["idx"], r["best"], want_idx, want_best)
            if want_out:
                assert same_values(r["out"].cpu().numpy(), want), f"{label}: out"
            else:
                assert r["out"] is None
            if want_sq:
                vec = _expect_vec(D, cb, r["out"], x, True)
                assert vec == (D % 4 == 0)  # dense tensors: the path depends on D alone
                assert math.isfinite(sq64) == finite
                ratio = _sq_ratio(label, float(r["sq_err"][0]), sq64, D, M, vec)
                if finite:
                    ratios.append((vec, ratio))
            else:
                assert r["sq_err"] is None
    _report(f"D={D} H=2 M=7 (R = {finalize_rows_per_wave(7)})", ratios)


# ------------------------------------------------------------------------------ 3. views, strides, alignment: the `vec` decision
def _view_data(oracle, D, H=2, M=37, K=11, P=3, seed=0):
    g = np.random.default_rng(4000 + D + seed)
    x = g.standard_normal((H, M, D)).astype(np.float32)
    x[:, ::3] *= np.float32(1e4)
    cb = (g.standard_normal((H, K, D)) * 1e-3).astype(np.float32)
    metric = (D // 2) % 2
    key = oracle.pack_key(np.abs(g.standard_normal((H, M))).astype(np.float32), g.integers(0, K, (H, M)), metric)
    home = g.integers(0, P, (H, M))
    planes = np.stack([np.where(home == p, key, KEY_INIT) for p in range(P)])
    return x, cb, planes, metric


def _x_views(x_np):
    """x dense, as rows of a wider buffer (row stride D + 1 and D + 4), and starting one float into its storage; NaN around it"""
    H, M, D = x_np.shape
    src = torch.from_numpy(x_np)
    yield "x dense", src.to(DEV)
    for pad in (1, 4):
        wide = torch.full((H, M, D + pad), NAN)
        wide[..., :D] = src
        yield f"x row stride D+{pad}", wide.to(DEV)[..., :D]
    flat = torch.full((H * M * D + 1,), NAN)
    flat[1:] = src.reshape(-1)
    yield "x one float into its storage", flat.to(DEV)[1:].view(H, M, D)


def _idx_best_views(H, M):
    """-> label, the shape of the idx / best buffers, and the function that cuts the [H, M] view out of either"""
    yield "idx dense", (H, M), lambda t: t
    yield "idx big[:, :, 1]", (H, M, 3), lambda t: t[:, :, 1]
    yield "idx wide[:, 2:2+M]", (H, M + 5), lambda t: t[:, 2:2 + M]


@pytest.mark.parametrize("ste,want_sq", [(True, True), (False, False)])
@pytest.mark.parametrize("D", [6, 8, 260])
def test_views_strides_and_alignment(oracle, D, ste, want_sq):
    native = _native()
    x_np, cb_np, planes, metric = _view_data(oracle, D)
    H, M, _ = x_np.shape
    cb, keys = _dev(cb_np), _dev(planes)
    want_idx, want_best, want_out, sq64 = finalize_reference(planes, cb_np, x_np, metric, ste)
    ratios, paths = [], set()
    for xl, x in _x_views(x_np):
        for o in (0, 1, 4):
            for il, shape, cut in _idx_best_views(H, M):
                label = f"D={D} ste={ste}: {xl}, out = buf[:, :, {o}:{o}+D], {il}"
                buf = torch.full((H, M, D + 8), SENT, device=DEV)
                ibuf = torch.full(shape, ISENT, dtype=torch.int64, device=DEV)
                bbuf = torch.full(shape, SENT, device=DEV)
                out, idx, best = buf[:, :, o:o + D], cut(ibuf), cut(bbuf)
                r = _finalize(native, x, cb, keys, metric=metric, ste=ste, want_sq_err=want_sq, out=out, idx=idx, best=best)
                # x misaligned or oddly strided changes the path only when x is read; the values never
                _assert_idx_best(label, idx, best, want_idx, want_best)
                assert same_values(out.cpu().numpy(), want_out), f"{label}: out"
                out.fill_(SENT), idx.fill_(ISENT), best.fill_(SENT)
                assert bool((buf == SENT).all()), f"{label}: wrote outside the out view"
                assert bool((ibuf == ISENT).all()) and bool((bbuf == SENT).all()), f"{label}: wrote outside the idx / best view"
                vec = _expect_vec(D, cb, out, x, ste or want_sq)
                paths.add(vec)
                if want_sq:
                    ratios.append((vec, _sq_ratio(label + (" [vector]" if vec else " [scalar]"), float(r["sq_err"][0]), sq64, D, M, vec)))
    assert paths == ({False} if D % 4 else {False, True})  # D = 8, 260: both paths among the views
    if want_sq:
        _report(f"views D={D} H={H} M={M} (R = {finalize_rows_per_wave(M)})", ratios)


@pytest.mark.parametrize("ste", [False, True])
@pytest.mark.parametrize("D", [6, 8, 260])
def test_sharded_overlap_calling_convention(oracle, D, ste):
    """sharded.py's overlap branch (world > 1 only) hands x[a:b], out[a:b], idx[a:b], best[a:b] of whole-batch buffers to the
    finalize, half by half.  With D = 6 the second `out` of the cut at 257 does not start on 16 bytes."""
    from vector_quantization.sharded import _NativeShardOps

    x_np, cb_np, planes_np, metric = _view_data(oracle, D, H=1, M=600, K=33, P=3, seed=1)
    M = 600
    x, table, planes = _dev(x_np[0]), _dev(cb_np[0]), _dev(planes_np[:, 0])
    want_idx, want_best, want_out, _ = finalize_reference(planes_np, cb_np, x_np, metric, ste)
    single = _NativeShardOps.finalize(x, table, planes, metric, ste, False)
    torch.cuda.synchronize()
    assert single[3] is None
    _assert_idx_best(f"D={D} single call", single[1], single[2], want_idx[0], want_best[0])
    assert same_values(single[0].cpu().numpy(), want_out[0])
    for cuts in (((0, 256), (256, M)), ((0, 257), (257, M))):
        out = torch.full((M, D), SENT, device=DEV)
        idx = torch.full((M,), ISENT, dtype=torch.int64, device=DEV)
        best = torch.full((M,), SENT, device=DEV)
        for a, b in cuts:
            _NativeShardOps.finalize(x[a:b], table, planes[:, a:b].contiguous(), metric, ste, False,
                                     out=out[a:b], idx=idx[a:b], best=best[a:b])
            torch.cuda.synchronize()
            if a == 0:  # the first half leaves the second alone
                assert bool((out[b:] == SENT).all()) and bool((idx[b:] == ISENT).all()) and bool((best[b:] == SENT).all())
        label = f"D={D} ste={ste} cuts={cuts}"
        _assert_idx_best(label, idx, best, want_idx[0], want_best[0])
        assert same_values(out.cpu().numpy(), want_out[0]), f"{label}: out"
        assert torch.equal(idx, single[1]) and torch.equal(out.view(torch.int32), single[0].view(torch.int32))
        assert torch.equal(best.view(torch.int32), single[2].view(torch.int32))


# ------------------------------------------------------------------------------- 4. more than 8192 rows, loss partials at capacity
@pytest.mark.parametrize("D", [4, 6])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("M", [8191, 8192, 8193, 16389, 20000])
def test_row_cap_and_loss_partials(oracle, M, H, D):
    native = _native()
    K = 16
    g = np.random.default_rng(M + 7 * H + D)
    x_np = g.standard_normal((H, M, D)).astype(np.float32)
    x_np[:, ::5] *= np.float32(1e3)
    cb_np = g.standard_normal((H, K, D)).astype(np.float32)
    value = np.abs(g.standard_normal((H, M))).astype(np.float32)
    win = oracle.pack_key(value, g.integers(0, K, (H, M)), EUCLID)
    lose = np.where(g.random((H, M)) < 0.5, KEY_INIT, oracle.pack_key(value + np.float32(1.0), g.integers(0, K, (H, M)), EUCLID))
    first = g.random((H, M)) < 0.5
    planes = np.stack([np.where(first, win, lose), np.where(first, lose, win)])
    want_idx, want_best, want_out, sq64 = finalize_reference(planes, cb_np, x_np, EUCLID, True)
    x, cb = _dev(x_np), _dev(cb_np)
    r = _finalize(native, x, cb, _dev(planes), metric=EUCLID, ste=True, want_sq_err=True)
    label = f"M={M} H={H} D={D}"
    _assert_idx_best(label, r["idx"], r["best"], want_idx, want_best)
    assert same_values(r["out"].cpu().numpy(), want_out), f"{label}: out"
    vec = _expect_vec(D, cb, r["out"], x, True)
    assert vec == (D % 4 == 0)
    R = finalize_rows_per_wave(M)
    assert R == {8191: 1, 8192: 1, 8193: 2, 16389: 3, 20000: 3}[M]
    ratio = _sq_ratio(label, float(r["sq_err"][0]), sq64, D, M, vec)
    _report(f"{label} (R = {R})", [(vec, ratio)])


def test_no_rows(oracle):
    native = _native()
    for H, D in ((1, 4), (3, 6)):
        cb = _dev(np.ones((H, 16, D), dtype=np.float32))
        x = torch.empty((H, 0, D), device=DEV)
        for shape in ((H, 0), (2, H, 0)):
            r = _finalize(native, x, cb, torch.empty(shape, dtype=torch.int64, device=DEV), ste=True, want_sq_err=True)
            assert r["out"].shape == (H, 0, D) and r["idx"].shape == (H, 0) and r["best"].shape == (H, 0)
            assert r["sq_err"].shape == (1,) and float(r["sq_err"][0]) == 0.0


# ----------------------------------------------------------------------------------------------------------- 5. argument errors
def test_finalize_rejects_bad_arguments(oracle):
    """vq_finalize_key_planes_f32 answers a bad argument with VQ_E_BADARG and a message that names it -- and launches nothing."""
    native = _native()
    lib = native.load()
    H, M, K, D = 1, 8, 4, 4
    g = np.random.default_rng(3)
    x_np = g.standard_normal((H, M, D)).astype(np.float32)
    cb_np = g.standard_normal((H, K, D)).astype(np.float32)
    planes = oracle.pack_key(np.abs(g.standard_normal((1, H, M))).astype(np.float32), g.integers(0, K, (1, H, M)), EUCLID)
    x, cb, keys = _dev(x_np), _dev(cb_np), _dev(planes)
    out = torch.full((H, M, D), SENT, device=DEV)
    idx = torch.full((H, M), ISENT, dtype=torch.int64, device=DEV)
    best = torch.full((H, M), SENT, device=DEV)
    sq = torch.full((1,), SENT, dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.vq_workspace_bytes(H, M, 1)) // 8 + 2, dtype=torch.float64, device=DEV)

    def args(**over):
        a = native.VqArgs()
        a.H, a.Q, a.M, a.K, a.D, a.metric, a.flags = H, 1, M, K, D, EUCLID, native.F_STE
        a.x, a.x_rs, a.x_hs = x.data_ptr(), D, M * D
        a.cb, a.cb_hs, a.cb_qs = cb.data_ptr(), K * D, 0
        a.out, a.out_rs, a.out_hs = out.data_ptr(), D, M * D
        a.idx, a.idx_rs, a.idx_hs, a.idx_qs = idx.data_ptr(), 1, M, 0
        a.best = best.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    BADARG = -1
    with_sq = dict(sq_err=sq.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 8)
    for over, keys_ptr, n_planes, cause in ((dict(), keys.data_ptr(), 0, "n_planes"),
                                            (dict(Q=2), keys.data_ptr(), 1, "Q must be 1"),
                                            (dict(), None, 1, "is null"),
                                            (dict(with_sq, workspace=None, workspace_bytes=0), keys.data_ptr(), 1, "workspace")):
        rc = lib.vq_finalize_key_planes_f32(ctypes.byref(args(**over)), keys_ptr, n_planes, stream)
        assert rc == BADARG, (cause, rc)
        assert cause in lib.vq_last_error().decode(), (cause, lib.vq_last_error())
    assert lib.vq_finalize_keys_f32(ctypes.byref(args()), None, stream) == BADARG  # the one-plane entry: same checks
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((idx == ISENT).all()) and bool((best == SENT).all()) and float(sq[0]) == SENT
    # the same arguments, well formed, through both entries
    want_idx, want_best, want_out, sq64 = finalize_reference(planes, cb_np, x_np, EUCLID, True)
    for call in (lambda a: lib.vq_finalize_key_planes_f32(ctypes.byref(a), keys.data_ptr(), 1, stream),
                 lambda a: lib.vq_finalize_keys_f32(ctypes.byref(a), keys.data_ptr(), stream)):
        out.fill_(SENT), sq.fill_(SENT)
        assert call(args(**with_sq)) == 0
        torch.cuda.synchronize()
        _assert_idx_best("raw call", idx, best, want_idx, want_best)
        assert same_values(out.cpu().numpy(), want_out)
        _sq_ratio("raw call", float(sq[0]), sq64, D, M, True)
