"""GPU edge suite of the straight-through Gumbel backward sweeps (vq_gumbel_stats_f32, vq_gumbel_backward_x_f32,
vq_gumbel_backward_codes_f32) against the fp64 closed form on the CPU:

1. the codes sweep with SEVERAL staged tiles per row split (the LDS ring, odd split starts, an uneven last split, the
   sub-tile break in a later tile) -- the plan each shape took is derived from the workspace size and asserted;
2. every padded width with D below, on and above it; scalar loads at D % 4 == 0; a destination view;
3. row and code counts on the 32 / 128 / 256 boundaries, M = 1;
4. the online softmax under saturated / flat temperatures, logits past fp32 exp's overflow, and codebooks ordered so that
   the running maximum moves at every sub-tile (or never).

Tolerance (the rule of test_reinmax_against_fp64): the reference's own fp32 op sequence is evaluated on the CPU first and
measured against fp64 as a fraction of the largest fp64 entry; the kernel may deviate by the larger of the project tolerance
(atol = 2e-5 * max|fp64|, rtol = 2e-4) and 4 x that error (native exp2 / log / rsq, another summation order).  lse2 / log2(e)
against the fp64 log-sum-exp: atol = the larger of 2e-5 (the project's for vq_softmax_stats_f32) and 4 x the fp32 reference's
absolute error, rtol = 2e-6.  Every measured reference error and kernel error is printed."""
from __future__ import annotations

import functools
import math

import pytest
import torch

from gen import make_codebook, make_x
from gumbel_run import GRAD_ATOL_OF_MAX, assert_grad_close, closed_form64, logsumexp64, similarities64

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
LSE_ATOL, LSE_RTOL = 2e-5, 2e-6
PACK_SLACK = 2048  # floats behind every packed image (vq_packed_floats)
NAMES = ("delta", "gx", "gc_sim", "gc")


# ------------------------------------------------------------------------------------------------ inputs and references
def _metric(metric):
    from vector_quantization import search

    return search.DOT if metric == "dot" else search.EUCLID


def _argmax64(x, c, dot):
    return similarities64(x.double(), c.double(), dot).argmax(-1)


@functools.lru_cache(maxsize=4)
def _inputs(shape, metric):
    """(x, c, g, ind) on the CPU: the suite's seeded rows (x 0.25 under dot, as elsewhere), codes and upstream gradient; the
    selection is the fp64 argmax."""
    h, m, k, d = shape
    x = make_x((h, m, d), "S") * (0.25 if metric == "dot" else 1.0)
    c = make_codebook(h, k, d, "S")
    g = torch.randn((h, m, d), generator=torch.Generator().manual_seed(2024))
    return x, c, g, _argmax64(x, c, metric == "dot")


def _reference(x, c, g, ind, tau, dot):
    """fp64 closed form and the reference's fp32 op sequence: two dicts of delta, gx, gc_sim, gc, lse (natural log)."""
    out = []
    for dtype in (torch.float64, torch.float32):
        ref = dict(zip(NAMES, closed_form64(x, c, g, ind, tau, dot, dtype=dtype)))
        ref["lse"] = logsumexp64(x, c, tau, dot, dtype=dtype)
        out.append(ref)
    return out


@functools.lru_cache(maxsize=4)
def _suite_reference(shape, metric, tau):
    return _reference(*_inputs(shape, metric), tau, metric == "dot")


def _native(x, c, g, ind, mt, tau, xd=None, gd=None, gx_out=None):
    """The three sweeps and the deterministic scatter -> dict of delta, gx, gc_sim, gc, lse (natural log) on the GPU."""
    from vector_quantization import native

    xd = x.cuda() if xd is None else xd
    gd = g.cuda() if gd is None else gd
    cd = c.cuda()
    m = x.shape[1]
    packed = native.pack_codebooks(cd, mt)
    lse2, delta = native.gumbel_stats(xd, cd, gd, metric=mt, tau=tau, packed=packed)
    gx = native.gumbel_backward_x(xd, cd, gd, lse2, delta, metric=mt, tau=tau, packed=packed, out=gx_out)
    gc_sim = native.gumbel_backward_codes(xd, cd, gd, lse2, delta, metric=mt, tau=tau)
    scatter = native.ema_accumulate(gd.contiguous(), ind.cuda(), c.shape[1], deterministic=True)[1]
    return dict(delta=delta[:, :m], gx=gx, gc_sim=gc_sim, gc=gc_sim + scatter, lse=lse2[:, :m].double() / LOG2E)


def _compare(case, got, ref64, ref32, names=NAMES + ("lse",), rows=None, codes=None):
    """``rows`` / ``codes``: index lists the comparison is restricted to (per-row and per-code outputs respectively)."""
    def cut(name, t):
        t = torch.as_tensor(t).detach().double().cpu()
        if rows is not None and name in ("delta", "gx", "lse"):
            t = t[:, rows]
        if codes is not None and name in ("gc_sim", "gc"):
            t = t[:, codes]
        return t

    for name in names:
        want, r32, have = cut(name, ref64[name]), cut(name, ref32[name]), cut(name, got[name])
        if name == "lse":
            ref_err = float((r32 - want).abs().max())
            atol = max(LSE_ATOL, 4 * ref_err)
            assert have.shape == want.shape and bool(torch.isfinite(have).all()), (case, name)
            err = (have - want).abs()
            print(f"{case} lse: the reference's fp32 sequence is {ref_err:.3e} off fp64 | kernel max err {float(err.max()):.3e} "
                  f"(atol {atol:.3e})")
            assert float((err - LSE_RTOL * want.abs()).max()) <= atol, (case, name, float(err.max()), atol)
        else:
            ref_err = float((r32 - want).abs().max() / want.abs().max())
            print(f"{case} {name}: the reference's fp32 sequence is {ref_err:.2e} of the largest entry off fp64")
            assert_grad_close(have, want, f"{case} {name}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * ref_err))


def _run_suite_case(shape, metric, tau, names=NAMES + ("lse",)):
    x, c, g, ind = _inputs(shape, metric)
    ref64, ref32 = _suite_reference(shape, metric, tau)
    got = _native(x, c, g, ind, _metric(metric), tau)
    _compare(f"{'x'.join(map(str, shape))} {metric} tau={tau:g}", got, ref64, ref32, names)


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ------------------------------------------------------------------------------------------------ 1. several tiles per split
MULTI_TILE = [(1, 2130, 130, 200), (1, 4150, 130, 256), (1, 8500, 130, 100), (1, 16600, 40, 64), (1, 8300, 40, 33),
              (1, 33200, 40, 32), (1, 16500, 40, 7), (4, 2565, 1030, 64)]
ODD_TILES_PER_SPLIT = {MULTI_TILE[i] for i in (1, 2, 3, 5, 7)}


def _padded_dim(d):
    return next(p for p in (32, 64, 128, 256) if d <= p)


def _codes_plan(shape):
    """(ntiles, tiles_per_split, splits) of vq_gumbel_backward_codes_f32, from the sizes the library reports: the packed row
    image fixes the staged tile, the workspace (two images + one [H, K, D] partial per split) the number of splits."""
    from vector_quantization import native

    h, m, k, d = shape
    dp = _padded_dim(d)
    tile = 32 * max(1, 256 // dp)
    ntiles = -(-m // tile)
    img_floats = native.packed_floats(m, d)
    assert img_floats == ntiles * tile * (dp + 4) + PACK_SLACK, (shape, img_floats)
    nbytes = int(native.load().vq_gumbel_workspace_bytes(h, m, k, d))
    assert nbytes > 0 and nbytes % 4 == 0
    part_floats = nbytes // 4 - 2 * h * img_floats
    assert part_floats >= 0 and part_floats % (h * k * d) == 0, (shape, nbytes)
    splits = max(1, part_floats // (h * k * d))  # (a single split writes the gradient directly: no partials)
    return ntiles, -(-ntiles // splits), splits


@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("shape", MULTI_TILE, ids=_ids(MULTI_TILE))
def test_codes_sweep_with_several_tiles_per_split(shape, metric):
    ntiles, tiles_per_split, splits = _codes_plan(shape)
    print(f"plan of {shape}: ntiles {ntiles}, tiles_per_split {tiles_per_split}, splits {splits}")
    assert tiles_per_split >= 2, "the shape no longer stages a second tile in any split: the LDS ring is not exercised"
    if shape in ODD_TILES_PER_SPLIT:
        assert tiles_per_split % 2 == 1, "the shape no longer starts a split on an odd tile"
    _run_suite_case(shape, metric, 1.0)


@pytest.mark.parametrize("shape", [MULTI_TILE[1], MULTI_TILE[7]], ids=_ids([MULTI_TILE[1], MULTI_TILE[7]]))
def test_multi_tile_reruns_are_bit_identical(shape):
    assert _codes_plan(shape)[1] >= 2
    x, c, g, ind = _inputs(shape, "euclid")
    one = _native(x, c, g, ind, _metric("euclid"), 1.0)
    two = _native(x, c, g, ind, _metric("euclid"), 1.0)
    for name in NAMES + ("lse",):
        assert torch.equal(one[name], two[name]), name


def test_row_equal_to_a_code_in_a_later_tile_of_a_later_split():
    """Euclid, s == 0 for (row 3050, code 77) of shape 2: tile 95, the third tile of split 31.  Everything must be finite; the
    row (delta, lse, gx) and the code (gc) of the pair are left out of the comparison, as in
    test_gpu_gumbel.py::test_row_equal_to_a_code_gives_finite_gradients -- the gradient is singular there."""
    shape, row, code = MULTI_TILE[1], 3050, 77
    ntiles, tiles_per_split, _ = _codes_plan(shape)
    assert tiles_per_split >= 2 and (row // 32) // tiles_per_split > 0 and (row // 32) % tiles_per_split > 0
    x, c, g, ind = (t.clone() for t in _inputs(shape, "euclid"))
    x[0, row] = c[0, code]
    ind[0, row] = code
    ref64, ref32 = _reference(x, c, g, ind, 1.0, False)
    got = _native(x, c, g, ind, _metric("euclid"), 1.0)
    for name in NAMES + ("lse",):
        assert bool(torch.isfinite(got[name]).all()), name
    _compare("coinciding pair", got, ref64, ref32, rows=[r for r in range(shape[1]) if r != row],
             codes=[k for k in range(shape[2]) if k != code])


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_relaxed_gather_over_the_multi_tile_path(metric):
    """The production dispatch (gumbel.relaxed_gather -> the backend's fused backward) at shape 1."""
    from vector_quantization import gumbel

    shape = MULTI_TILE[0]
    assert _codes_plan(shape)[1] >= 2
    x, c, g, ind = _inputs(shape, metric)
    ref64, ref32 = _suite_reference(shape, metric, 1.0)
    xr, cr = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    (gumbel.relaxed_gather(xr, cr, ind.cuda(), _metric(metric), 1.0) * g.cuda()).sum().backward()
    _compare(f"relaxed_gather {metric}", dict(gx=xr.grad, gc=cr.grad), ref64, ref32, names=("gx", "gc"))


# ------------------------------------------------------------------------------------------------ 2. dim edges
DIM_EDGES = [1, 3, 31, 32, 33, 63, 65, 127, 129, 200, 255]


@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("d", DIM_EDGES)
def test_dim_edges_of_every_padded_width(d, metric):
    """(D = 1 under Euclid is ill-conditioned for any fp32 evaluation: rows all but coincide with a code on the line and
    |x|^2 + |c|^2 - 2 x c loses the distance r = w / s divides by.  Measured on an MI355X: gx 1.4e-2 of the largest entry for
    the kernel and for the reference's fp32 sequence alike; every other width stays below 1.2e-5.)"""
    _run_suite_case((2, 133, 70, d), metric, 1 / 0.7)


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_rows_one_float_into_a_buffer_take_scalar_loads(metric):
    """D = 64 (D % 4 == 0) with x and g starting 4 bytes into their buffers: the 16-byte loads are off."""
    shape = (2, 133, 70, 64)
    x, c, g, ind = _inputs(shape, metric)
    ref64, ref32 = _suite_reference(shape, metric, 1 / 0.7)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return view

    got = _native(x, c, g, ind, _metric(metric), 1 / 0.7, xd=shifted(x), gd=shifted(g))
    _compare(f"shifted rows {metric}", got, ref64, ref32)


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_destination_view_at_a_padded_width(metric):
    """gx at D = 200 (Dp = 256) written into an unaligned view of a larger buffer; the bytes around it stay untouched."""
    shape = (2, 133, 70, 200)
    h, m, _, d = shape
    x, c, g, ind = _inputs(shape, metric)
    ref64, ref32 = _suite_reference(shape, metric, 1 / 0.7)
    big = torch.full((h, m + 2, d + 7), 777.0, device="cuda")
    out = big[:, 1:m + 1, 3:d + 3]
    got = _native(x, c, g, ind, _metric(metric), 1 / 0.7, gx_out=out)
    assert got["gx"].data_ptr() == out.data_ptr()
    _compare(f"destination view {metric}", got, ref64, ref32, names=("gx",))
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:, 1:m + 1, 3:d + 3] = False
    assert bool((big[keep] == 777.0).all()), "bytes around the destination view were written"


# ------------------------------------------------------------------------------------------------ 3. tiling boundaries
BOUNDARIES = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257]


@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("d", [48, 256])
@pytest.mark.parametrize("m", BOUNDARIES)
def test_row_counts_on_the_tiling_boundaries(m, d, metric):
    _run_suite_case((1, m, 70, d), metric, 1.0)


@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("d", [48, 256])
@pytest.mark.parametrize("k", [2] + BOUNDARIES[1:])
def test_code_counts_on_the_tiling_boundaries(k, d, metric):
    _run_suite_case((1, 133, k, d), metric, 1.0)


@pytest.mark.parametrize("entry", ["vq_gumbel_backward_codes_f32", "vq_gumbel_reinmax_backward_codes_f32"])
def test_an_empty_call_clears_grad_codes(entry):
    """M = 0 (H = 2, K = 7, D = 5) through the C ABI (the Python wrappers refuse M = 0): no sweep, grad_codes all zeros.  The
    statistics arrays and the workspace of an empty call are NULL."""
    import ctypes

    from vector_quantization import native

    h, k, d = 2, 7, 5
    a = native.VqArgs()
    a.H, a.Q, a.M, a.K, a.D, a.metric, a.flags = h, 1, 0, k, d, 0, 0
    cb = torch.randn((h, k, d), device="cuda")
    g = torch.empty((h, 0, d), device="cuda")
    a.cb, a.cb_hs = cb.data_ptr(), k * d
    gc = torch.full((h, k, d), float("nan"), device="cuda")
    stats = [None] * (2 if entry == "vq_gumbel_backward_codes_f32" else 5)
    with torch.cuda.device(gc.device):
        rc = getattr(native.load(), entry)(ctypes.byref(a), g.data_ptr() or 16, d, 0, 1.0, *stats, gc.data_ptr(), None, 0,
                                           native._stream_ptr(gc.device))
    assert rc == 0, native.load().vq_last_error()
    assert torch.equal(gc, torch.zeros_like(gc))


# ------------------------------------------------------------------------------------------------ 4. online softmax under stress
@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("shape,tau", [((2, 133, 70, 48), 20.0), ((2, 133, 70, 48), 1e-3), ((1, 300, 520, 64), 8.0)],
                         ids=["saturated", "flat", "saturated-17-subtiles"])
def test_saturated_and_flat_temperatures(shape, tau, metric):
    _run_suite_case(shape, metric, tau)


STRESS = (1, 300, 520, 64)


def test_logits_beyond_the_range_of_fp32_exp():
    """Dot metric, tau = 2, rows scaled until max |tau s| passes 88.7 (exp overflows in fp32 from there): a softmax that
    does not subtract the running maximum returns inf / nan here."""
    h, m, k, d = STRESS
    tau = 2.0
    x = make_x((h, m, d), "S") * 1.25
    c = make_codebook(h, k, d, "S")
    g = torch.randn((h, m, d), generator=torch.Generator().manual_seed(2024))
    logits = similarities64(x.double(), c.double(), True) * tau
    print(f"large logits: tau s in [{float(logits.min()):.1f}, {float(logits.max()):.1f}]")
    assert float(logits.max()) > 88.7 and float(logits.min()) < -88.7
    ind = logits.argmax(-1)
    ref64, ref32 = _reference(x, c, g, ind, tau, True)
    got = _native(x, c, g, ind, _metric("dot"), tau)
    _compare("large logits", got, ref64, ref32, names=("lse", "delta", "gx", "gc"))


def _ordered_codebook(metric):
    """(x, c) with every row's per-sub-tile (32 codes) maximum of the similarity rising strictly with the sub-tile index."""
    h, m, k, d = STRESS
    gen = torch.Generator().manual_seed(515)
    if metric == "euclid":  # -|x - c_k| ~ -|c_k|: the code norms fall linearly from 3 sqrt(D) to about 0, the rows are small
        dirs = torch.nn.functional.normalize(torch.randn((h, k, d), generator=gen), dim=-1)
        c = dirs * (3.0 * math.sqrt(d) * (1.0 - torch.arange(k) / k))[None, :, None]
        x = 0.05 * torch.randn((h, m, d), generator=gen)
    else:  # x . c_k ~ 32 k / K: the codes walk along u, the rows sit near 4 u
        u = torch.nn.functional.normalize(torch.randn((d,), generator=gen), dim=-1)
        c = (torch.arange(k) / k)[None, :, None] * u * 8.0 + 0.01 * torch.randn((h, k, d), generator=gen)
        x = 4.0 * u + 0.05 * torch.randn((h, m, d), generator=gen)
    return x, c


def _subtile_maxima(s):
    pad = -s.shape[-1] % 32
    s = torch.nn.functional.pad(s, (0, pad), value=-math.inf)
    return s.view(*s.shape[:-1], -1, 32).max(-1).values


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_running_maximum_that_moves_at_every_subtile_or_never(metric, order):
    dot = metric == "dot"
    x, c = _ordered_codebook(metric)
    if order == "descending":
        c = c.flip(1)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(2024))
    s = similarities64(x.double(), c.double(), dot)
    steps = _subtile_maxima(s).diff(dim=-1)
    assert steps.shape[-1] == 16
    assert bool((steps > 0).all() if order == "ascending" else (steps < 0).all()), "the codebook order is no longer adversarial"
    ind = s.argmax(-1)
    ref64, ref32 = _reference(x, c, g, ind, 1.0, dot)
    got = _native(x, c, g, ind, _metric(metric), 1.0)
    _compare(f"{order} codebook {metric}", got, ref64, ref32, names=("lse", "delta", "gx", "gc"))
