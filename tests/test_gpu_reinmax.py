"""GPU suite of the fused reinmax Gumbel backward (vq_gumbel_reinmax_stats_f32, vq_gumbel_reinmax_columns_f32,
vq_gumbel_reinmax_backward_x_f32, vq_gumbel_reinmax_backward_codes_f32) against the fp64 closed form on the CPU.

Tolerances are the project's rules:
* gradients, e and delta0: assert_grad_close with atol = max(2e-5, 4 x the error of the reference's own fp32 op sequence)
  of the largest fp64 entry, rtol = 2e-4 (the rule of test_gpu_gumbel.py::test_reinmax_against_fp64);
* log-sum-exps: the LSE_ATOL / LSE_RTOL rule of test_gpu_gumbel_edges.py;
* col: entry by entry and RELATIVE, |got - want| <= max(2e-4, 4 x the fp32 sequence's worst relative error) x want -- a
  tolerance scaled by the largest column would hide a padding row counted into a small (all-clamped) column.
Every measured reference error and kernel error is printed."""
from __future__ import annotations

import functools

import pytest
import torch

from gen import make_codebook, make_x
from gumbel_run import GRAD_ATOL_OF_MAX, GRAD_RTOL, assert_grad_close, closed_form64, similarities64

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
LSE_ATOL, LSE_RTOL = 2e-5, 2e-6
PACK_SLACK = 2048  # floats behind every packed image (vq_packed_floats)
GRADS = ("delta0", "e", "gx", "gc_sim", "gc")
ALL = GRADS + ("col", "lse_tau", "lse_one")


# ------------------------------------------------------------------------------------------------ inputs and references
def _metric(metric):
    from vector_quantization import search

    return search.DOT if metric == "dot" else search.EUCLID


@functools.lru_cache(maxsize=4)
def _inputs(shape, metric):
    """(x, c, g, ind) on the CPU, as tests/test_gpu_gumbel_edges.py::_inputs: ind is the fp64 argmax."""
    h, m, k, d = shape
    x = make_x((h, m, d), "S") * (0.25 if metric == "dot" else 1.0)
    c = make_codebook(h, k, d, "S")
    g = torch.randn((h, m, d), generator=torch.Generator().manual_seed(2024))
    return x, c, g, similarities64(x.double(), c.double(), metric == "dot").argmax(-1)


def _dense(x, c, g, ind, tau, dot, dtype):
    """Dense reinmax statistics in ``dtype``: col [H, K], e [H, K], both natural-log log-sum-exps [H, M], p1 [H, M, K]."""
    x, c, g = x.to(dtype), c.to(dtype), g.to(dtype)
    s = similarities64(x, c, dot)
    a = g @ c.transpose(-1, -2)
    onehot = torch.nn.functional.one_hot(ind.clamp(0, c.shape[1] - 1), c.shape[1]).to(dtype)
    onehot = onehot * ((ind >= 0) & (ind < c.shape[1]))[..., None]
    p1 = ((onehot + (s * tau).softmax(-1)) / 2).clamp(min=1e-5)
    col = p1.sum(dim=1)
    return dict(col=col, e=(p1 * a).sum(dim=1) / col, lse_tau=(s * tau).logsumexp(-1), lse_one=s.logsumexp(-1), p1=p1)


def _reference(x, c, g, ind, tau, dot):
    """fp64 closed form and the reference's fp32 op sequence: two dicts of ALL (+ p1)."""
    out = []
    for dtype in (torch.float64, torch.float32):
        ref = dict(zip(("delta0", "gx", "gc_sim", "gc"), closed_form64(x, c, g, ind, tau, dot, reinmax=True, dtype=dtype)))
        ref.update(_dense(x, c, g, ind, tau, dot, dtype))
        out.append(ref)
    return out


@functools.lru_cache(maxsize=4)
def _suite_reference(shape, metric, tau):
    return _reference(*_inputs(shape, metric), tau, metric == "dot")


def _native(x, c, g, ind, mt, tau, xd=None, gd=None, gx_out=None):
    """The four sweeps and the deterministic scatter -> dict of ALL on the GPU."""
    from vector_quantization import native

    xd = x.cuda() if xd is None else xd
    gd = g.cuda() if gd is None else gd
    cd, indd = c.cuda(), ind.cuda()
    m, k = x.shape[1], c.shape[1]
    packed = native.pack_codebooks(cd, mt)
    stats = native.gumbel_reinmax_stats(xd, cd, gd, metric=mt, tau=tau, packed=packed)
    col, e, ws = native.gumbel_reinmax_columns(xd, cd, gd, stats[0], indd, metric=mt, tau=tau)
    gx = native.gumbel_reinmax_backward_x(xd, cd, gd, stats, indd, col, e, metric=mt, tau=tau, packed=packed, out=gx_out)
    gc_sim = native.gumbel_reinmax_backward_codes(xd, cd, gd, stats, col, e, ws, metric=mt, tau=tau)
    scatter = native.ema_accumulate(gd.contiguous(), indd.clamp(0, k - 1), k, deterministic=True)[1]
    return dict(lse_tau=stats[0][:, :m].double() / LOG2E, lse_one=stats[1][:, :m].double() / LOG2E, delta0=stats[2][:, :m],
                col=col[:, :k], e=e[:, :k], gx=gx, gc_sim=gc_sim, gc=gc_sim + scatter)


def _compare(case, got, ref64, ref32, names=ALL, rows=None, codes=None):
    """``rows`` / ``codes``: index lists the comparison is restricted to (per-row and per-code outputs respectively)."""
    def cut(name, t):
        t = torch.as_tensor(t).detach().double().cpu()
        if rows is not None and name in ("delta0", "gx", "lse_tau", "lse_one"):
            t = t[:, rows]
        if codes is not None and name in ("gc_sim", "gc", "col", "e"):
            t = t[:, codes]
        return t

    for name in names:
        want, r32, have = cut(name, ref64[name]), cut(name, ref32[name]), cut(name, got[name])
        assert have.shape == want.shape and bool(torch.isfinite(have).all()), (case, name)
        if name.startswith("lse"):
            ref_err = float((r32 - want).abs().max())
            atol = max(LSE_ATOL, 4 * ref_err)
            err = (have - want).abs()
            print(f"{case} {name}: the reference's fp32 sequence is {ref_err:.3e} off fp64 | kernel max err {float(err.max()):.3e} "
                  f"(atol {atol:.3e})")
            assert float((err - LSE_RTOL * want.abs()).max()) <= atol, (case, name, float(err.max()), atol)
        elif name == "col":
            ref_rel = float(((r32 - want).abs() / want).max())
            rtol = max(GRAD_RTOL, 4 * ref_rel)
            rel = (have - want).abs() / want
            print(f"{case} col: the reference's fp32 sequence is {ref_rel:.2e} (worst relative) off fp64 | kernel worst relative "
                  f"err {float(rel.max()):.3e} (rtol {rtol:.3e})")
            assert float(rel.max()) <= rtol, (case, name, float(rel.max()), rtol)
        else:
            ref_err = float((r32 - want).abs().max() / want.abs().max())
            print(f"{case} {name}: the reference's fp32 sequence is {ref_err:.2e} of the largest entry off fp64")
            assert_grad_close(have, want, f"{case} {name}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * ref_err))


def _run_suite_case(shape, metric, tau, names=ALL):
    x, c, g, ind = _inputs(shape, metric)
    ref64, ref32 = _suite_reference(shape, metric, tau)
    got = _native(x, c, g, ind, _metric(metric), tau)
    _compare(f"{'x'.join(map(str, shape))} {metric} tau={tau:g}", got, ref64, ref32, names)
    return got, ref64


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ------------------------------------------------------------------------------------------------ 1. the project's shapes
SHAPES = [(1, 300, 256, 64), (4, 130, 520, 64), (1, 111, 301, 100), (2, 33, 7, 5), (1, 40, 1, 16), (1, 70, 1000, 128),
          (1, 96, 512, 256)]


@pytest.mark.parametrize("temperature", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_closed_form_at_the_project_shapes(shape, metric, temperature):
    """(K = 1 is no zero-gradient case under reinmax: w = (2 / M)(a - mean a).)"""
    _run_suite_case(shape, metric, 1.0 / temperature)


# ------------------------------------------------------------------------------------------------ 2. the clamp and the padding
@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("shape,tau", [((2, 133, 70, 48), 20.0), ((1, 300, 520, 64), 8.0)], ids=["133-rows", "300-rows"])
def test_all_clamped_columns_do_not_see_padding_rows(shape, tau, metric):
    """Saturated softmax: most of p1 is the clamp's 1e-5, whole columns are M x 1e-5.  A padding row of the packed image that
    is not masked adds another 1e-5 to every such column (0.75 % at M = 133, with 123 padding rows in the tile)."""
    ref64, _ = _suite_reference(shape, metric, tau)
    m = shape[1]
    clamped = ref64["p1"] == 1e-5
    all_clamped = int(clamped.all(dim=1).sum())
    print(f"{shape} {metric}: {all_clamped} all-clamped columns of {clamped.shape[0] * clamped.shape[2]}, "
          f"{float(clamped.double().mean()):.1%} of the entries clamped")
    assert all_clamped >= 1 and float(clamped.double().mean()) > 0.9
    assert bool((ref64["col"][clamped.all(dim=1)] - m * 1e-5).abs().max() < 1e-12)
    _run_suite_case(shape, metric, tau)


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_flat_temperature(metric):
    _run_suite_case((2, 133, 70, 48), metric, 1e-3)


# ------------------------------------------------------------------------------------------------ 3. tiling boundaries
@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("d", [48, 256])
@pytest.mark.parametrize("m", [1, 31, 33, 129, 257])
def test_row_counts_on_the_tiling_boundaries(m, d, metric):
    got, ref64 = _run_suite_case((1, m, 70, d), metric, 2.0)
    if m == 1 and metric == "dot" and d == 48:
        n = int((ref64["col"] == 1e-5).sum())
        print(f"M = 1, dot: {n} all-clamped columns")
        assert n == 5, "the M = 1 case no longer has its all-clamped columns"


@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("d", [48, 256])
@pytest.mark.parametrize("k", [2, 31, 33, 129, 257])
def test_code_counts_on_the_tiling_boundaries(k, d, metric):
    _run_suite_case((1, 133, k, d), metric, 2.0)


# ------------------------------------------------------------------------------------------------ 4. ind is really used
IND_SHAPE = (2, 133, 70, 48)


def _selection(kind, metric):
    x, c, g, ind = _inputs(IND_SHAPE, metric)
    if kind == "random":
        ind = torch.randint(0, IND_SHAPE[2], ind.shape, generator=torch.Generator().manual_seed(7))
    elif kind == "constant":
        ind = torch.full_like(ind, 5)
    return x, c, g, ind


@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("kind", ["random", "constant", "argmax"])
def test_every_selection_matches_its_own_closed_form(kind, metric):
    x, c, g, ind = _selection(kind, metric)
    ref64, ref32 = _reference(x, c, g, ind, 2.0, metric == "dot")
    got = _native(x, c, g, ind, _metric(metric), 2.0)
    _compare(f"ind {kind} {metric}", got, ref64, ref32)


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_a_different_selection_gives_a_different_gradient(metric):
    """Guards against a kernel that ignores ind: the gx of a random selection and of the argmax differ by far more than the
    tolerance either is held to."""
    outs = {}
    for kind in ("random", "argmax"):
        x, c, g, ind = _selection(kind, metric)
        outs[kind] = _native(x, c, g, ind, _metric(metric), 2.0)["gx"].double().cpu()
    want = closed_form64(*_selection("argmax", metric), 2.0, metric == "dot", reinmax=True)[1]
    gap = float((outs["random"] - outs["argmax"]).abs().max())
    atol = GRAD_ATOL_OF_MAX * float(want.abs().max())
    print(f"{metric}: gx of the two selections differ by {gap:.3e} (tolerance {atol:.3e})")
    assert gap > 100 * atol


def test_a_selection_outside_the_codebook_selects_nothing():
    """ind is compared, never an address: -1, K and 2^40 give the closed form with an all-zero one-hot for those rows."""
    x, c, g, ind = (t.clone() for t in _inputs(IND_SHAPE, "euclid"))
    ind[0, 3], ind[1, 130], ind[1, 7] = -1, IND_SHAPE[2], 2 ** 40
    from vector_quantization import native

    mt = _metric("euclid")
    xd, cd, gd, indd = x.cuda(), c.cuda(), g.cuda(), ind.cuda()
    stats = native.gumbel_reinmax_stats(xd, cd, gd, metric=mt, tau=2.0)
    col, e, ws = native.gumbel_reinmax_columns(xd, cd, gd, stats[0], indd, metric=mt, tau=2.0)
    gx = native.gumbel_reinmax_backward_x(xd, cd, gd, stats, indd, col, e, metric=mt, tau=2.0)
    gc = native.gumbel_reinmax_backward_codes(xd, cd, gd, stats, col, e, ws, metric=mt, tau=2.0)
    want = _dense(x, c, g, ind, 2.0, False, torch.float64)
    k = IND_SHAPE[2]
    assert float(((col[:, :k].double().cpu() - want["col"]).abs() / want["col"]).max()) <= GRAD_RTOL
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gc).all())


# ------------------------------------------------------------------------------------------------ 5. several tiles per split
MULTI_TILE = [(1, 2130, 130, 200), (1, 4150, 130, 256), (1, 16600, 40, 64), (4, 2565, 1030, 64)]


def _padded_dim(d):
    return next(p for p in (32, 64, 128, 256) if d <= p)


def _plan(shape):
    """(ntiles, tiles_per_split, splits) of the column sweep and the codes sweep (one plan), from the sizes the library reports
    and the documented workspace layout: two images, the int32 selection, the col / e partials of every split, and the
    [H, K, D] partial of every split when there is more than one."""
    from vector_quantization import native

    h, m, k, d = shape
    dp = _padded_dim(d)
    tile = 32 * max(1, 256 // dp)
    ntiles = -(-m // tile)
    img_floats = native.packed_floats(m, d)
    assert img_floats == ntiles * tile * (dp + 4) + PACK_SLACK, (shape, img_floats)
    lib = native.load()
    rs_m, rs_k = int(lib.vq_gumbel_row_stride(m)), int(lib.vq_gumbel_row_stride(k))
    nbytes = int(lib.vq_gumbel_reinmax_workspace_bytes(h, m, k, d))
    assert nbytes > 0 and nbytes % 4 == 0
    rest = nbytes // 4 - 2 * h * img_floats - h * rs_m
    if rest == 2 * h * rs_k:
        splits = 1
    else:
        assert rest > 0 and rest % (2 * h * rs_k + h * k * d) == 0, (shape, nbytes)
        splits = rest // (2 * h * rs_k + h * k * d)
        assert splits > 1
    return ntiles, -(-ntiles // splits), splits


@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("shape", MULTI_TILE, ids=_ids(MULTI_TILE))
def test_sweeps_with_several_tiles_per_split(shape, metric):
    ntiles, tiles_per_split, splits = _plan(shape)
    print(f"plan of {shape}: ntiles {ntiles}, tiles_per_split {tiles_per_split}, splits {splits}")
    assert tiles_per_split >= 2, "the shape no longer stages a second tile in any split: the LDS ring is not exercised"
    if shape != MULTI_TILE[0]:
        assert tiles_per_split % 2 == 1, "the shape no longer starts a split on an odd tile"
    _run_suite_case(shape, metric, 2.0)


# ------------------------------------------------------------------------------------------------ 6. reruns
@pytest.mark.parametrize("shape", [(4, 130, 520, 64), (1, 4150, 130, 256)], ids=_ids([(4, 130, 520, 64), (1, 4150, 130, 256)]))
def test_two_runs_are_bit_identical(shape):
    x, c, g, ind = _inputs(shape, "euclid")
    one = _native(x, c, g, ind, _metric("euclid"), 2.0)
    two = _native(x, c, g, ind, _metric("euclid"), 2.0)
    for name in ALL:
        assert torch.equal(one[name], two[name]), name


# ------------------------------------------------------------------------------------------------ 7. a row equal to a code
def test_row_equal_to_a_code_gives_finite_gradients():
    """Euclid, s == 0 for (row 57, code 9): everything must be finite; the row and the code of the pair are left out of the
    comparison, as in test_gpu_gumbel.py::test_row_equal_to_a_code_gives_finite_gradients -- the gradient is singular there."""
    shape, row, code = (1, 300, 256, 64), 57, 9
    x, c, g, ind = (t.clone() for t in _inputs(shape, "euclid"))
    x[0, row] = c[0, code]
    ind[0, row] = code
    ref64, ref32 = _reference(x, c, g, ind, 1.0, False)
    got = _native(x, c, g, ind, _metric("euclid"), 1.0)
    for name in ALL:
        assert bool(torch.isfinite(got[name]).all()), name
    _compare("coinciding pair", got, ref64, ref32, rows=[r for r in range(shape[1]) if r != row],
             codes=[k for k in range(shape[2]) if k != code])


# ------------------------------------------------------------------------------------------------ 8. layout
@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_strided_rows_and_rows_one_float_into_a_buffer(metric):
    """D = 64 with x rows of stride 80 and g starting 4 bytes into its buffer (16-byte loads off for g, strided for x), then
    x shifted and g strided."""
    shape = (2, 133, 70, 64)
    h, m, _, d = shape
    x, c, g, ind = _inputs(shape, metric)
    ref64, ref32 = _suite_reference(shape, metric, 2.0)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return view

    def strided(t):
        view = torch.full((h, m, d + 16), 555.0, device="cuda")[:, :, 8:8 + d]
        view.copy_(t)
        assert view.stride(1) == d + 16
        return view

    for xd, gd, what in ((strided(x), shifted(g), "strided x, shifted g"), (shifted(x), strided(g), "shifted x, strided g")):
        got = _native(x, c, g, ind, _metric(metric), 2.0, xd=xd, gd=gd)
        _compare(f"{what} {metric}", got, ref64, ref32)


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_destination_view_at_a_padded_width(metric):
    """gx at D = 200 (Dp = 256) written into an unaligned view of a larger buffer; the bytes around it stay untouched."""
    shape = (2, 133, 70, 200)
    h, m, _, d = shape
    x, c, g, ind = _inputs(shape, metric)
    ref64, ref32 = _suite_reference(shape, metric, 2.0)
    big = torch.full((h, m + 2, d + 7), 777.0, device="cuda")
    out = big[:, 1:m + 1, 3:d + 3]
    got = _native(x, c, g, ind, _metric(metric), 2.0, gx_out=out)
    assert got["gx"].data_ptr() == out.data_ptr()
    _compare(f"destination view {metric}", got, ref64, ref32, names=("gx",))
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:, 1:m + 1, 3:d + 3] = False
    assert bool((big[keep] == 777.0).all()), "bytes around the destination view were written"


# ------------------------------------------------------------------------------------------------ 9. dispatch
DISPATCH = (1, 300, 256, 64)


def _relaxed_grads(x, c, g, ind, mt, tau, live=None):
    from vector_quantization import gumbel

    xr, cr = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    out = gumbel.relaxed_gather(xr, cr, ind.cuda(), mt, 1.0 / tau, reinmax=True, live_codes=live)
    (out * g.cuda()).sum().backward()
    return dict(gx=xr.grad, gc=cr.grad)


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_relaxed_gather_takes_the_fused_path(metric, monkeypatch):
    from vector_quantization import gumbel

    x, c, g, ind = _inputs(DISPATCH, metric)
    ref64, ref32 = _suite_reference(DISPATCH, metric, 2.0)
    chunked = _relaxed_grads_chunked(x, c, g, ind, _metric(metric), 2.0)

    def boom(*args, **kwargs):
        raise AssertionError("the chunked path was taken")

    monkeypatch.setattr(gumbel, "_chunked_backward", boom)
    fused = _relaxed_grads(x, c, g, ind, _metric(metric), 2.0)
    _compare(f"fused relaxed_gather {metric}", fused, ref64, ref32, names=("gx", "gc"))
    _compare(f"chunked relaxed_gather {metric}", chunked, ref64, ref32, names=("gx", "gc"))
    for name in ("gx", "gc"):  # the two paths against each other: each is within the tolerance of fp64, so twice that apart
        ref_err = float((ref32[name].double() - ref64[name]).abs().max() / ref64[name].abs().max())
        assert_grad_close(fused[name], chunked[name].double().cpu(), f"fused against chunked {metric} {name}",
                          atol_of_max=2 * max(GRAD_ATOL_OF_MAX, 4 * ref_err), rtol=2 * GRAD_RTOL)


def _relaxed_grads_chunked(x, c, g, ind, mt, tau):
    """The chunked path on the same inputs: a backend without reinmax_backward falls through to it."""
    from vector_quantization import search

    class NoReinmax:
        pass

    native_backend = search.get_backend()
    for name in ("similarities", "ema_accumulate"):
        setattr(NoReinmax, name, staticmethod(getattr(native_backend, name)))
    search.set_backend(NoReinmax)
    try:
        return _relaxed_grads(x, c, g, ind, mt, tau)
    finally:
        search.set_backend(None)


def test_wide_rows_and_live_codes_stay_on_the_chunked_path(monkeypatch):
    from vector_quantization import gumbel, search

    calls = []
    chunked = gumbel._chunked_backward

    def spy(*args, **kwargs):
        calls.append(1)
        return chunked(*args, **kwargs)

    monkeypatch.setattr(gumbel, "_chunked_backward", spy)
    # D = 400: outside the kernels' range
    shape = (1, 64, 40, 400)
    x, c, g, ind = _inputs(shape, "dot")
    assert search.get_backend().reinmax_backward(x.cuda(), c.cuda(), g.cuda(), ind.cuda(), metric=_metric("dot"), tau=2.0) is None
    got = _relaxed_grads(x, c, g, ind, _metric("dot"), 2.0)
    assert len(calls) == 1
    ref64, ref32 = _reference(x, c, g, ind, 2.0, True)
    _compare("D = 400", got, ref64, ref32, names=("gx", "gc"))
    # live codes (an EMA step between forward and backward): chunked, whatever the width
    x, c, g, ind = _inputs(DISPATCH, "dot")
    _relaxed_grads(x, c, g, ind, _metric("dot"), 2.0, live=c.cuda().clone())
    assert len(calls) == 2


# ------------------------------------------------------------------------------------------------ 10. module level
def test_vector_quantize_module_end_to_end(monkeypatch):
    """VectorQuantize (learnable codebook, no EMA, reinmax at temperature 0.5, dims 64) in train mode, the chunked path made to
    raise.  The module returns x + (picked - x).detach(), so what reaches the relaxed selection is the gradient of the
    commitment loss through ``picked``; it is recorded with a hook as g, and the closed form is fed with the module's own ind
    and that g.  Two backward passes over one forward each:
    * the loss alone: embeddings.grad = gc(g), and x.grad = gx(g) - g (the loss's direct term).  x.grad + g is compared with
      gx(g); the sum x.grad was rounded to fp32 at the size of g, so half an ulp of max|g| is added to the tolerance;
    * (q * r).sum() + loss: x.grad = r - g + gx(g), the straight-through term on top."""
    import vector_quantization as vq
    from vector_quantization import gumbel
    from vector_quantization.codebooks import CodebookParams, GumbelParams

    def boom(*args, **kwargs):
        raise AssertionError("the chunked path was taken")

    monkeypatch.setattr(gumbel, "_chunked_backward", boom)
    seen = []
    relaxed_gather = gumbel.relaxed_gather

    def recording(*args, **kwargs):
        out = relaxed_gather(*args, **kwargs)
        out.register_hook(lambda grad: seen.append(grad.detach().clone()))
        return out

    monkeypatch.setattr(gumbel, "relaxed_gather", recording)
    dim, k, m = 64, 256, 300
    params = CodebookParams(dim=dim, codebook_size=k, learnable_codebook=True, ema_update=False,
                            gumbel_params=GumbelParams(temperature=0.5, straight_through=True, reinmax=True))
    torch.manual_seed(11)
    mod = vq.VectorQuantize(dim=dim, codebook_params=params).cuda().train()
    x = make_x((1, m, dim), "S")
    r = torch.randn((1, m, dim), generator=torch.Generator().manual_seed(2024))
    c = mod._codebook.embeddings.detach().cpu().reshape(1, k, dim).clone()

    def run(with_output_term):
        seen.clear()
        mod.zero_grad(set_to_none=True)
        xr = x.cuda().requires_grad_(True)
        q, ind, loss = mod(xr)
        ((q * r.cuda()).sum() + loss.sum() if with_output_term else loss.sum()).backward()
        assert len(seen) == 1, "the relaxed selection was not part of the graph"
        return xr.grad.cpu(), mod._codebook.embeddings.grad.cpu().reshape(1, k, dim), ind.cpu().reshape(1, m), seen[0].cpu().reshape(1, m, dim)

    gx_got, gc_got, ind, g = run(False)
    assert float(g.abs().max()) > 0
    _, gx64, _, gc64 = closed_form64(x, c, g, ind, 2.0, False, reinmax=True)
    _, gx32, _, gc32 = closed_form64(x, c, g, ind, 2.0, False, reinmax=True, dtype=torch.float32)
    errs = {}
    for r32, want, what in ((gx32, gx64, "gx"), (gc32, gc64, "gc")):
        errs[what] = float((r32.double() - want).abs().max() / want.abs().max())
        print(f"module {what}: the reference's fp32 sequence is {errs[what]:.2e} of the largest entry off fp64")
    assert_grad_close(gc_got, gc64, "module embeddings.grad", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * errs["gc"]))
    half_ulp = float(g.abs().max()) * 2.0 ** -24 / float(gx64.abs().max())
    print(f"module gx: half an ulp of max|g| is {half_ulp:.2e} of the largest entry of gx")
    assert_grad_close(gx_got.double() + g.double(), gx64, "module x.grad + g", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * errs["gx"]) + half_ulp)

    gx_got2, gc_got2, ind2, g2 = run(True)
    assert torch.equal(ind, ind2) and torch.equal(g, g2)
    assert_grad_close(gc_got2, gc64, "module embeddings.grad, second pass", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * errs["gc"]))
    assert_grad_close(gx_got2, r.double() - g.double() + gx64, "module x.grad with the straight-through term")
