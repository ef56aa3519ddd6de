"""GPU suite of the Gumbel straight-through / reinmax relaxations: the fused sweeps (vq_gumbel_stats_f32,
vq_gumbel_backward_x_f32, vq_gumbel_backward_codes_f32) against the fp64 closed form on the CPU, their layout and edge cases,
and the modules against the fixtures captured from the reference.

Tolerance of the straight-through kernels: the project's own for vq_ce_backward_f32, atol = 2e-5 * max|fp64 gradient|,
rtol = 2e-4 (the reference's fp32 op sequence on the CPU stays within 7.3e-6 of the largest entry on these shapes)."""
from __future__ import annotations

import functools

import pytest
import torch

from gen import make_codebook, make_x
from gumbel_cases import GUMBEL_CASES
from gumbel_run import GRAD_ATOL_OF_MAX, assert_grad_close, check_fixture, closed_form64

pytestmark = pytest.mark.gpu

SHAPES = [(1, 300, 256, 64), (4, 130, 520, 64), (1, 111, 301, 100), (2, 33, 7, 5), (1, 40, 1, 16), (1, 70, 1000, 128),
          (1, 96, 512, 256), (1, 512, 1024, 256)]
TEMPERATURES = [0.5, 1.0, 2.0]


@functools.lru_cache(maxsize=4)
def _inputs(shape, metric):
    """(x, c, g) on the CPU and the native search's index (the selection the relaxation differentiates)."""
    from vector_quantization import search

    h, m, k, d = shape
    x = make_x((h, m, d), "S") * (0.25 if metric == "dot" else 1.0)
    c = make_codebook(h, k, d, "S")
    g = torch.randn((h, m, d), generator=torch.Generator().manual_seed(2024))
    mt = search.DOT if metric == "dot" else search.EUCLID
    ind, _, _ = search.nearest_with_distance(x.cuda(), c.cuda(), metric=mt)
    return x, c, g, ind.cpu(), mt


def _native_grads(x, c, g, ind, mt, tau):
    from vector_quantization import native

    xd, cd, gd = x.cuda(), c.cuda(), g.cuda()
    packed = native.pack_codebooks(cd, mt)
    lse2, delta = native.gumbel_stats(xd, cd, gd, metric=mt, tau=tau, packed=packed)
    gx = native.gumbel_backward_x(xd, cd, gd, lse2, delta, metric=mt, tau=tau, packed=packed)
    gc_sim = native.gumbel_backward_codes(xd, cd, gd, lse2, delta, metric=mt, tau=tau)
    scatter = native.ema_accumulate(gd, ind.cuda(), c.shape[1], deterministic=True)[1]  # (the atomics-free variant)
    return delta[:, :x.shape[1]], gx, gc_sim, gc_sim + scatter


@pytest.mark.parametrize("temperature", TEMPERATURES)
@pytest.mark.parametrize("metric", ["euclid", "dot"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernels_match_the_fp64_closed_form(shape, metric, temperature):
    x, c, g, ind, mt = _inputs(shape, metric)
    tau = 1.0 / temperature
    delta64, gx64, gcs64, gc64 = closed_form64(x, c, g, ind, tau, metric == "dot")
    delta, gx, gc_sim, gc = _native_grads(x, c, g, ind, mt, tau)
    assert_grad_close(delta, delta64, "delta")
    if shape[2] == 1:  # one code: p = 1, a - delta = 0 -- nothing flows through the similarities
        assert not bool(gx.any()), "gx must be exactly 0 with a single code"
        assert_grad_close(gc_sim, torch.zeros_like(gc_sim), "gc_sim (K = 1)", atol_of_max=0.0, rtol=0.0)
    else:
        assert_grad_close(gx, gx64, "gx")
    assert_grad_close(gc, gc64, "gc")


def test_strided_rows_and_a_destination_view():
    """Head-split views [h, rows, d] of [rows, 3, 32] buffers for x and g; gx written into a view of a larger buffer."""
    from vector_quantization import native, search

    rows, h, d, k = 150, 3, 32, 70
    gen = torch.Generator().manual_seed(11)
    xb = torch.randn((rows, h, d), generator=gen)
    gb = torch.randn((rows, h, d), generator=gen)
    c = torch.randn((h, k, d), generator=gen)
    x, g = xb.cuda().permute(1, 0, 2), gb.cuda().permute(1, 0, 2)
    assert not x.is_contiguous()
    cd = c.cuda()
    ind = torch.cdist(xb.permute(1, 0, 2).double(), c.double()).argmin(-1)
    for mt, dot in ((search.EUCLID, False), (search.DOT, True)):
        lse2, delta = native.gumbel_stats(x, cd, g, metric=mt, tau=1.25)
        big = torch.full((rows + 2, h, d + 8), 777.0, device="cuda")
        out = big[1:rows + 1, :, 4:d + 4].permute(1, 0, 2)
        native.gumbel_backward_x(x, cd, g, lse2, delta, metric=mt, tau=1.25, out=out)
        gc_sim = native.gumbel_backward_codes(x, cd, g, lse2, delta, metric=mt, tau=1.25)
        _, gx64, gcs64, _ = closed_form64(xb.permute(1, 0, 2), c, gb.permute(1, 0, 2), ind, 1.25, dot)
        assert_grad_close(out, gx64, "gx (strided)")
        assert_grad_close(gc_sim, gcs64, "gc_sim (strided)")
        keep = torch.ones_like(big, dtype=torch.bool)
        keep[1:rows + 1, :, 4:d + 4] = False
        assert bool((big[keep] == 777.0).all()), "bytes around the destination view were written"


def test_row_equal_to_a_code_gives_finite_gradients():
    """Euclid, s == 0 for one (row, code) pair: ATen masks the pair's contribution.  Everything must be finite; the row (gx)
    and the code (gc) of the pair are left out of the comparison -- the gradient is singular there, and fp32 cdist itself
    returns a tiny nonzero distance for such a pair."""
    from vector_quantization import search

    x, c, g, ind, mt = (t.clone() if torch.is_tensor(t) else t for t in _inputs((1, 300, 256, 64), "euclid"))
    x[0, 5] = c[0, 7]
    ind[0, 5] = 7
    _, gx64, _, gc64 = closed_form64(x, c, g, ind, 1.0, False)
    _, gx, gc_sim, gc = _native_grads(x, c, g, ind, mt, 1.0)
    for t in (gx, gc_sim, gc):
        assert bool(torch.isfinite(t).all())
    rows = [r for r in range(300) if r != 5]
    codes = [k for k in range(256) if k != 7]
    assert_grad_close(gx[:, rows], gx64[:, rows], "gx without the coinciding row")
    assert_grad_close(gc[:, codes], gc64[:, codes], "gc without the coinciding code")


@pytest.mark.parametrize("shape", [(4, 130, 520, 64), (1, 512, 1024, 256)], ids=["4x130x520x64", "1x512x1024x256"])
def test_two_runs_are_bit_identical(shape):
    x, c, g, ind, mt = _inputs(shape, "euclid")
    one = _native_grads(x, c, g, ind, mt, 2.0)
    two = _native_grads(x, c, g, ind, mt, 2.0)
    for a, b, what in zip(one, two, ("delta", "gx", "gc_sim", "gc")):
        assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------ module level
@pytest.mark.parametrize("name", list(GUMBEL_CASES))
def test_fixture_on_the_gpu(name):
    check_fixture(name, "cuda")


def _module_grads(x, c, g, ind, mt, temperature, reinmax=False):
    from vector_quantization import gumbel

    xr, cr = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    (gumbel.relaxed_gather(xr, cr, ind.cuda(), mt, temperature, reinmax) * g.cuda()).sum().backward()
    return xr.grad, cr.grad


@pytest.mark.parametrize("shape", [(2, 150, 300, 400), (1, 64, 2048, 512)], ids=["2x150x300x400", "1x64x2048x512"])
@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_wide_rows_take_the_chunked_path(shape, metric):
    from vector_quantization import native, search

    x, c, g, ind, mt = _inputs(shape, metric)
    assert search.get_backend().gumbel_backward(x.cuda(), c.cuda(), g.cuda(), metric=mt, tau=1.0) is None
    assert shape[3] > native.GUMBEL_MAX_DIM
    gx, gc = _module_grads(x, c, g, ind, mt, 0.7)
    _, gx64, _, gc64 = closed_form64(x, c, g, ind, 1 / 0.7, metric == "dot")
    assert_grad_close(gx, gx64, "gx (chunked)")
    assert_grad_close(gc, gc64, "gc (chunked)")


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_fused_and_chunked_agree(metric):
    from vector_quantization import gumbel, search

    x, c, g, ind, mt = _inputs((1, 300, 256, 64), metric)
    xd, cd, gd = x.cuda(), c.cuda(), g.cuda()
    fused = search.get_backend().gumbel_backward(xd, cd, gd, metric=mt, tau=1 / 0.7)
    assert fused is not None
    chunked = gumbel._chunked_backward(xd, cd, None, ind.cuda(), gd, mt, 1 / 0.7, False, True, True)
    _, gx64, gcs64, _ = closed_form64(x, c, g, ind, 1 / 0.7, metric == "dot")
    for got, other, want, what in ((fused[0], chunked[0], gx64, "gx"), (fused[1], chunked[1], gcs64, "gc_sim")):
        assert_grad_close(got, want, f"{what}: fused vs fp64")
        assert_grad_close(other, want, f"{what}: chunked vs fp64")
        assert_grad_close(got, other, f"{what}: fused vs chunked")


def test_reinmax_against_fp64():
    """(1, 512, 1024, 256), dot metric, T = 0.5: the reference's own fp32 op sequence (CPU) is measured against fp64 first;
    the chunked path may deviate by the larger of the project tolerance and 4 x that error (native exp / log and another
    summation order)."""
    x, c, g, ind, mt = _inputs((1, 512, 1024, 256), "dot")
    tau = 2.0
    _, gx64, _, gc64 = closed_form64(x, c, g, ind, tau, True, reinmax=True)
    _, gx32, _, gc32 = closed_form64(x, c, g, ind, tau, True, reinmax=True, dtype=torch.float32)
    gx, gc = _module_grads(x, c, g, ind, mt, 0.5, reinmax=True)
    for got, ref32, want, what in ((gx, gx32, gx64, "gx"), (gc, gc32, gc64, "gc")):
        ref_err = float((ref32.double() - want).abs().max() / want.abs().max())
        print(f"reinmax {what}: the reference's fp32 sequence is {ref_err:.2e} of the largest entry off fp64")
        assert_grad_close(got, want, f"reinmax {what}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * ref_err))
