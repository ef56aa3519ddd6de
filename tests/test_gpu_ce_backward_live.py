"""vq_ce_backward_live_f32: the fused cross-entropy backward when the codebook was rewritten between forward and backward
(EMA training).  The weights come from the codes the forward searched (c), what they are multiplied with from the live
codes (l):

    gs_mk = coef [t_m >= 0] (softmax_k(s_m)_k - [k == t_m]),   s = similarities(x, c)
    dot     gx_m = sum_k gs_mk l_k
    Euclid  r_mk = gs_mk / s_mk (0 where s_mk == 0);   gx_m = x_m sum_k r_mk - sum_k r_mk l_k

Reference: that closed form in float64 on the CPU, the distances written out as sqrt(sum (x - c)^2) (torch.cdist's expanded
form turns an exact zero into 1e-7 and the ratio into 1e6).  Tolerance: the project's own for vq_ce_backward_f32,
atol = 2e-5 * max|fp64 gradient|, rtol = 2e-4; where the fp64 gradient is identically zero (K == 1) the scale is coef, as in
test_fused_cross_entropy_backward (fp32 leaves 1e-7 of noise there).  Every test prints its figure before it asserts.
"""
from __future__ import annotations

import contextlib
import copy
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gen import make_codebook, make_x  # noqa: E402

DEV = "cuda:0"
COEF = 0.37
ATOL, RTOL = 2e-5, 2e-4


def _native():
    from vector_quantization import native

    native.load()
    return native


@contextlib.contextmanager
def _env(name):
    os.environ[name] = "1"
    try:
        yield
    finally:
        os.environ.pop(name, None)


def _inputs(H, M, K, D, metric):
    x, c = make_x((H, M, D), "S"), make_codebook(H, K, D, "S")
    if metric == 1:
        x = x * 0.25  # keep the dot-product softmax away from one-hot saturation
    target = torch.randint(0, K, (H, M), generator=torch.Generator().manual_seed(11))
    target[:, 4::5] = -1  # rows m % 5 == 4 are ignored (M == 1 keeps a valid row)
    return x, c, target


def _live_codebooks(c):
    g = torch.Generator().manual_seed(23)
    return {"independent": torch.randn(c.shape, generator=g),
            "near": 0.8 * c + 0.2 * torch.randn(c.shape, generator=g),
            "zeros": torch.zeros_like(c)}


def _closed_form(x, c, lives, target, metric, coef):
    """float64 closed form of the module docstring -> one gradient [H, M, D] per live codebook in `lives`."""
    x, c = x.double(), c.double()
    lives = [l.double() for l in lives]
    outs = [torch.zeros_like(x) for _ in lives]
    for h in range(x.shape[0]):
        if metric == 0:
            s = -((x[h][:, None, :] - c[h][None, :, :]) ** 2).sum(-1).sqrt()
        else:
            s = x[h] @ c[h].T
        t = target[h]
        valid = t >= 0
        onehot = torch.zeros_like(s)
        onehot[valid, t[valid]] = 1.0
        gs = coef * valid[:, None].double() * (torch.softmax(s, -1) - onehot)
        if metric == 0:
            assert bool((s[valid] != 0).all()), "the closed-form cases hold no coinciding (row, code) pair"
            r = torch.where(s == 0, torch.zeros_like(gs), gs / s)
        for out, l in zip(outs, lives):
            out[h] = gs @ l[h] if metric == 1 else x[h] * r.sum(-1, keepdim=True) - r @ l[h]
    return outs


@functools.lru_cache(maxsize=None)
def _case(H, M, K, D, metric):
    """Inputs, live codebooks and their float64 gradients of one (shape, metric): computed once, shared, never modified."""
    x, c, target = _inputs(H, M, K, D, metric)
    lives = _live_codebooks(c)
    wants = dict(zip(lives, _closed_form(x, c, list(lives.values()), target, metric, COEF)))
    return x, c, target, lives, wants


def _assert_close(got, want, what, floor=COEF):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    scale = float(want.abs().max())
    if scale == 0.0:
        scale = floor
    err = (got - want).abs()
    bound = ATOL * scale + RTOL * want.abs()
    print(f"{what}: max error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}, scale {scale:.3e}")
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=ATOL * scale, rtol=RTOL)


def _fused(native, xs, cs, ts, metric, live, coef=COEF, **kw):
    lse, tl = native.softmax_stats(xs, cs, metric=metric, target=ts)
    return native.ce_backward(xs, cs, lse, tl, ts, torch.tensor([coef], device=DEV), metric=metric, live=live, **kw)


CLOSED_FORM_SHAPES = [
    (2, 133, 130, 256),   # 5 staged tiles of 32 codes, K tail, heads
    (1, 161, 97, 256),    # 4 tiles, a one-code tail
    (1, 129, 200, 128),   # 4 tiles of 64
    (1, 300, 300, 64),    # 3 tiles of 128, two 8-wave workgroups
    (1, 70, 520, 32),     # 3 tiles of 256, the sub-tile break
    (3, 129, 257, 200),   # padded dims, head strides of both images
    (1, 130, 70, 250),    # scalar row loads
    (2, 33, 7, 5),
    (1, 1, 33, 48),
    (1, 40, 1, 16),       # the gradient is exactly 0
]


@pytest.mark.parametrize("H,M,K,D", CLOSED_FORM_SHAPES)
@pytest.mark.parametrize("metric", [0, 1])
def test_closed_form(H, M, K, D, metric):
    """Three live codebooks per shape: an independent one (any mix-up of the two images is an O(1) error), 0.8 c + 0.2 noise,
    and all zeros -- under dot nothing of c may reach the contraction or the finalize, so the gradient is exactly 0."""
    native = _native()
    x, c, target, lives, wants = _case(H, M, K, D, metric)
    xs, cs, ts = x.to(DEV), c.to(DEV), target.to(DEV)
    for kind, live in lives.items():
        got = _fused(native, xs, cs, ts, metric, live.to(DEV))
        torch.cuda.synchronize()
        _assert_close(got, wants[kind], f"closed form {(H, M, K, D)} metric {metric} live {kind}")
        assert bool((got[:, 4::5] == 0).all()), "ignored rows must get exactly zero gradient"
        if kind == "zeros" and metric == 1:
            assert int(torch.count_nonzero(got)) == 0, "dot, live codes all zero: something of the searched codes reached gx"


@pytest.mark.parametrize("H,M,K,D", [(1, 128, 32, 256), (2, 333, 1030, 200), (1, 4097, 64, 132), (3, 129, 7, 256), (1, 300, 300, 64),
                                     (1, 70, 520, 32)])
@pytest.mark.parametrize("metric", [0, 1])
def test_live_equal_to_searched_codes_is_the_non_live_kernel_bit_for_bit(H, M, K, D, metric):
    """live = c.clone(): the same MFMA chains in the same order as the one-wave vq_ce_backward (VQ_CE_NO_ROLES=1), a zero
    distance included under Euclid."""
    native = _native()
    x, c, target = _inputs(H, M, K, D, metric)
    if metric == 0:
        x[0, 3] = c[0, K // 2]  # a coinciding (row, code) pair: ATen's subgradient 0
    xs, cs, ts = x.to(DEV), c.to(DEV), target.to(DEV)
    lse, tl = native.softmax_stats(xs, cs, metric=metric, target=ts)
    coef = torch.tensor([0.5], device=DEV)
    got = native.ce_backward(xs, cs, lse, tl, ts, coef, metric=metric, live=cs.clone())
    with _env("VQ_CE_NO_ROLES"):
        ref = native.ce_backward(xs, cs, lse, tl, ts, coef, metric=metric)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    # the same pointers for both images are legal too
    pk = native.pack_codebooks(cs, metric)
    same = native.ce_backward(xs, cs, lse, tl, ts, coef, metric=metric, packed=pk, live=cs, live_packed=pk)
    torch.cuda.synchronize()
    assert torch.equal(same.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("D", [30, 250])
@pytest.mark.parametrize("metric", [0, 1])
def test_rows_one_float_into_a_wider_buffer(D, metric):
    native = _native()
    H, M, K = 1, 130, 70
    x, c, target, lives, wants = _case(H, M, K, D, metric)
    wide = torch.full((H, M, D + 1), 9.0, device=DEV)
    wide[:, :, 1:] = x.to(DEV)
    xs = wide[:, :, 1:]  # row stride D + 1, base 4 bytes past a 16-byte boundary
    assert xs.data_ptr() % 16 == 4 and not xs.is_contiguous()
    got = _fused(native, xs, c.to(DEV), target.to(DEV), metric, lives["independent"].to(DEV))
    torch.cuda.synchronize()
    _assert_close(got, wants["independent"], f"offset view D {D} metric {metric}")


def test_strided_heads_and_a_strided_live_codebook():
    """[h, rows]-strided x / target (as test_fused_cross_entropy_backward_strided_heads), and a live codebook that is a strided
    slice of a larger tensor: the wrapper makes it contiguous."""
    native = _native()
    rows, heads, d, K = 200, 3, 32, 96
    x4 = make_x((rows, heads, d), "S")
    c = make_codebook(heads, K, d, "S")
    target = torch.randint(0, K, (rows, heads), generator=torch.Generator().manual_seed(2))
    target[4::5] = -1
    big = torch.randn((heads, 2 * K, d), generator=torch.Generator().manual_seed(3))
    live = big[:, ::2]
    flat, ts = x4.to(DEV).permute(1, 0, 2), target.to(DEV).permute(1, 0)
    live_dev = big.to(DEV)[:, ::2]
    assert not flat.is_contiguous() and not ts.is_contiguous() and not live_dev.is_contiguous()
    (want,) = _closed_form(x4.permute(1, 0, 2), c, [live], target.permute(1, 0), 0, COEF)
    got = _fused(native, flat, c.to(DEV), ts, 0, live_dev)
    torch.cuda.synchronize()
    _assert_close(got, want, "strided heads, strided live codebook")


def _autograd_gradient(x, c, target, metric, live, live_packed=None):
    from vector_quantization import losses

    xs = x.clone().requires_grad_(True)
    loss = losses.cross_entropy_to_codes(xs, c, target, metric, live_codes=live, live_packed=live_packed)
    loss.backward()
    torch.cuda.synchronize()
    return xs.grad


@pytest.mark.parametrize("metric", [0, 1])
def test_rows_wider_than_256_keep_the_chunked_path(metric):
    from vector_quantization import search

    native = _native()
    H, M, K, D = 1, 70, 50, 400
    x, c, target = _inputs(H, M, K, D, metric)
    live = _live_codebooks(c)["independent"]
    xs, cs, ts, ls = x.to(DEV), c.to(DEV), target.to(DEV), live.to(DEV)
    lse, tl = native.softmax_stats(xs, cs, metric=metric, target=ts)
    coef = torch.tensor([COEF], device=DEV)
    assert search.get_backend().cross_entropy_backward(xs, cs, lse, tl, ts, coef, metric=metric, live=ls) is None
    count = int((target >= 0).sum())
    (want,) = _closed_form(x, c, [live], target, metric, 1.0 / count)
    _assert_close(_autograd_gradient(xs, cs, ts, metric, ls), want, f"D = 400 metric {metric}, autograd function", floor=1.0 / count)


@pytest.mark.parametrize("metric", [0, 1])
def test_switch_takes_the_chunked_path(monkeypatch, metric):
    """VQ_CE_NO_LIVE=1: backend.similarities runs during backward; without it not once.  Both against each other."""
    from vector_quantization import search

    _native()
    H, M, K, D = 2, 133, 130, 64
    x, c, target = _inputs(H, M, K, D, metric)
    live = _live_codebooks(c)["near"]
    xs, cs, ts, ls = x.to(DEV), c.to(DEV), target.to(DEV), live.to(DEV)
    backend = search.get_backend()
    real, calls = backend.similarities, []

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(backend, "similarities", counting)
    fused = _autograd_gradient(xs, cs, ts, metric, ls)
    assert len(calls) == 0
    with _env("VQ_CE_NO_LIVE"):
        chunked = _autograd_gradient(xs, cs, ts, metric, ls)
    assert len(calls) > 0
    _assert_close(fused, chunked, f"fused against chunked, metric {metric}")


# ------------------------------------------------------------------------------------------------ the module, end to end
def _module(heads):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    K = 256
    if heads == 1:
        mod = vq.VectorQuantize(dim=64, codebook_params=CodebookParams(dim=64, codebook_size=K, threshold_ema_dead_code=0),
                                commitment_use_cross_entropy_loss=True)
    else:
        mod = vq.VectorQuantize(dim=64, heads=heads, codebook_dim=64 // heads, separate_codebook_per_head=True,
                                codebook_params=CodebookParams(dim=64 // heads, codebook_size=K, threshold_ema_dead_code=0),
                                commitment_use_cross_entropy_loss=True)
    with torch.no_grad():
        e = mod._codebook.embeddings
        e.copy_(torch.randn(e.shape, generator=torch.Generator().manual_seed(5)))
        mod._codebook.embed_avg.copy_(e)
    return mod.to(DEV).train()


def _forward(mod, x, given):
    """One training forward, reproducible: the atomics-free EMA accumulation (and no dead-code replacement in _module, as in
    test_modules_train_reproducibly_under_torch_deterministic_mode), so that two copies of a module leave bit-equal buffers.  -> (loss, indices | None, x leaf)"""
    xs = x.clone().requires_grad_(True)
    torch.manual_seed(1234)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        if given is None:
            _, idx, loss = mod(xs)
        else:
            (_, loss), idx = mod(xs, indices=given), None
    finally:
        torch.use_deterministic_algorithms(was)
    return loss.sum(), idx, xs


def _buffers(mod):
    book = mod._codebook
    return [book.embeddings.detach().clone(), book.cluster_size.detach().clone(), book.embed_avg.detach().clone()]


@pytest.mark.parametrize("heads,shape", [(1, (4, 64, 64)), (2, (2, 50, 64))])
@pytest.mark.parametrize("teacher_forcing", [False, True])
def test_module_end_to_end(heads, shape, teacher_forcing):
    """EMA codebook, cross-entropy commitment (or `indices=`: the return_loss branch), train mode: two deep copies, one under
    VQ_CE_NO_LIVE=1.  The forward is untouched (loss, indices and EMA buffers bit-equal); x.grad agrees within the tolerance."""
    _native()
    base = _module(heads)
    x = make_x(shape, "S").to(DEV)
    given = None
    if teacher_forcing:
        ishape = shape[:2] if heads == 1 else shape[:2] + (heads,)
        given = torch.randint(0, 256, ishape, generator=torch.Generator().manual_seed(9)).to(DEV)
    results = []
    for switch in (False, True):
        mod = copy.deepcopy(base)
        loss, idx, xs = _forward(mod, x, given)
        with _env("VQ_CE_NO_LIVE") if switch else contextlib.nullcontext():
            loss.backward()
        torch.cuda.synchronize()
        results.append((loss.detach(), idx, _buffers(mod), xs.grad))
    (loss_f, idx_f, buf_f, g_f), (loss_c, idx_c, buf_c, g_c) = results
    assert torch.equal(loss_f, loss_c)
    assert teacher_forcing or torch.equal(idx_f, idx_c)
    for a, b in zip(buf_f, buf_c):
        assert torch.equal(a, b)
    assert not torch.equal(buf_f[0], base._codebook.embeddings), "the EMA step did not run"
    assert float(g_c.abs().max()) > 0
    _assert_close(g_f, g_c, f"module heads {heads} teacher forcing {teacher_forcing}: fused against chunked")


def test_live_means_backward_time():
    """The codes are overwritten between forward and backward: the fused path reads them (and their image) when backward runs."""
    _native()
    base = _module(1)
    x = make_x((4, 64, 64), "S").to(DEV)
    other = torch.randn((1, 256, 64), generator=torch.Generator().manual_seed(77)).to(DEV)
    grads = {}
    for name, overwrite, switch in (("fused", True, False), ("chunked", True, True), ("untouched", False, False)):
        mod = copy.deepcopy(base)
        loss, _, xs = _forward(mod, x, None)
        if overwrite:
            mod._codebook.embeddings.data.copy_(other)
            mod._codebook.invalidate_packed()
        with _env("VQ_CE_NO_LIVE") if switch else contextlib.nullcontext():
            loss.backward()
        torch.cuda.synchronize()
        grads[name] = xs.grad
    _assert_close(grads["fused"], grads["chunked"], "overwritten codes: fused against chunked")
    moved = float((grads["fused"] - grads["untouched"]).abs().max())
    bound = ATOL * float(grads["untouched"].abs().max())
    print(f"overwrite moved the gradient by {moved:.3e} = {moved / bound:.1f} x the tolerance")
    assert moved > 100 * bound


def test_nothing_of_m_by_k():
    """M = 65536, K = 1024, D = 64, EMA codebook, cross-entropy commitment: forward + backward stay under 128 MiB above the
    baseline -- one [M, K] chunk of the chunked path alone is 256 MiB."""
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    _native()
    torch.manual_seed(0)
    mod = vq.VectorQuantize(dim=64, codebook_params=CodebookParams(dim=64, codebook_size=1024),
                            commitment_use_cross_entropy_loss=True).to(DEV).train()
    x = torch.randn(64, 1024, 64, device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _, _, loss = mod(x)
    loss.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the baseline: {peak / 2**20:.1f} MiB")
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    assert peak < 128 * 2**20, peak / 2**20


@pytest.mark.parametrize("H,M,K,D", [(2, 133, 130, 256), (1, 300, 300, 64)])
@pytest.mark.parametrize("metric", [0, 1])
def test_two_runs_are_equal(H, M, K, D, metric):
    native = _native()
    x, c, target, lives, _ = _case(H, M, K, D, metric)
    xs, cs, ts, ls = x.to(DEV), c.to(DEV), target.to(DEV), lives["near"].to(DEV)
    a = _fused(native, xs, cs, ts, metric, ls)
    b = _fused(native, xs, cs, ts, metric, ls)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
