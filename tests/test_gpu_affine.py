"""use_affine codebooks on the native path (vq_affine_stats_f32 / vq_affine_apply_f32 around the search): the reference's
fixtures, the tensor-op path as a second opinion, dense recomputation from the buffers, strided inputs, wide rows and
hipGraph replay of an eval-mode module."""
from __future__ import annotations

import copy
import os

import numpy as np
import pytest
import torch

from affine_cases import AFFINE_CASES
from affine_run import build_module, check_fixture, dense_effective_codes, run_step

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STATS = ("batch_mean", "batch_variance", "codebook_mean", "codebook_variance")


@pytest.fixture(autouse=True)
def _native_path():
    os.environ.pop("VQ_NO_FUSED_AFFINE", None)
    yield
    os.environ.pop("VQ_NO_FUSED_AFFINE", None)


def _params(dim, k, **kw):
    from vector_quantization.codebooks import AffineParameters, CodebookParams

    return CodebookParams(dim=dim, codebook_size=k, use_affine=True, threshold_ema_dead_code=0,
                          affine_params=AffineParameters(sync=False, batch_decay=0.9, codebook_decay=0.8), **kw)


@pytest.mark.parametrize("name", list(AFFINE_CASES))
def test_fixture_on_the_native_path(name):
    check_fixture(name, DEV)


@pytest.mark.parametrize("name", list(AFFINE_CASES))
def test_native_and_tensor_op_paths_agree(name):
    outs = []
    for switch in (False, True):
        if switch:
            os.environ["VQ_NO_FUSED_AFFINE"] = "1"
        mod, book, arrays, c = build_module(name, DEV)
        res = [run_step(mod, book, arrays, c, s, DEV) for s in range(len(c["steps"]))]
        outs.append((res, book))
    (a, book_a), (b, book_b) = outs
    for ra, rb in zip(a, b):
        assert torch.equal(ra["embed_ind"], rb["embed_ind"])
        np.testing.assert_allclose(ra["quantize"].detach().cpu().numpy(), rb["quantize"].detach().cpu().numpy(), atol=1e-5, rtol=0)
    for n in STATS:
        np.testing.assert_allclose(getattr(book_a, n).cpu().numpy(), getattr(book_b, n).cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(book_a.cluster_size.cpu().numpy(), book_b.cluster_size.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(book_a.embed_avg.cpu().numpy(), book_b.embed_avg.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(book_a.embeddings.detach().cpu().numpy(), book_b.embeddings.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)


def test_a_training_forward_runs_the_native_kernels(monkeypatch):
    """One training forward with EMA reaches vq_affine_stats_f32 twice (the codes, the batch) and vq_affine_apply_f32 twice
    (mode 0 for the searched codes, mode 1 for the accumulated sums); with VQ_NO_FUSED_AFFINE=1 neither is reached."""
    import vector_quantization as vq
    from vector_quantization import search

    backend = search.get_backend()
    calls = []
    real_stats, real_apply = backend.column_stats, backend.affine_apply

    def spy_stats(x, mask=None):
        calls.append(("stats", tuple(x.shape)))
        return real_stats(x, mask)

    def spy_apply(src, *stats, mode, **kw):
        calls.append(("apply", mode))
        return real_apply(src, *stats, mode=mode, **kw)

    monkeypatch.setattr(backend, "column_stats", staticmethod(spy_stats))
    monkeypatch.setattr(backend, "affine_apply", staticmethod(spy_apply))
    torch.manual_seed(1)
    mod = vq.VectorQuantize(dim=32, codebook_params=_params(32, 64)).to(DEV).train()
    x = torch.randn((2, 50, 32), device=DEV)
    with torch.no_grad():
        mod(x)
    assert calls == [("stats", (1, 64, 32)), ("stats", (1, 100, 32)), ("apply", 0), ("apply", 1)], calls
    del calls[:]
    mod.eval()
    with torch.no_grad():
        mod(x)
    assert calls == [("stats", (1, 100, 32)), ("apply", 0)], calls  # eval: the batch statistics move, the codebook's do not
    del calls[:]
    os.environ["VQ_NO_FUSED_AFFINE"] = "1"
    with torch.no_grad():
        mod.train()(x)
    assert calls == []


def _assert_dense(book, x_rows, q_rows, idx_rows, what):
    """Every row's chosen code is the nearest of the codes recomputed in fp64 from the buffers as they stand (ties within
    1e-5 of the scale), and the returned row is that code."""
    codes = dense_effective_codes(book)[0]
    dist = torch.cdist(x_rows.double(), codes)
    chosen = dist.gather(1, idx_rows[:, None])[:, 0]
    assert bool((chosen <= dist.min(dim=1).values + 1e-5 * float(dist.max())).all()), f"{what}: a row missed its nearest code"
    np.testing.assert_allclose(q_rows.cpu().numpy(), codes[idx_rows].float().cpu().numpy(), atol=1e-5, rtol=0, err_msg=what)


def test_no_stale_packed_image_between_forwards():
    """Two forwards on different batches with the codes frozen: the statistics move, so the searched codes move, and each
    forward matches a dense recomputation from the buffers it left."""
    import vector_quantization as vq

    torch.manual_seed(3)
    mod = vq.VectorQuantize(dim=64, codebook_params=_params(64, 256)).to(DEV).train()
    book = mod._codebook
    gen = torch.Generator(device=DEV).manual_seed(11)
    seen = []
    for step, (scale, shift) in enumerate([(1.0, 0.0), (2.5, 1.5)]):
        x = torch.randn((4, 300, 64), generator=gen, device=DEV) * scale + shift
        with torch.no_grad():
            q, idx, _ = mod(x, freeze_codebook=True)
        _assert_dense(book, x.reshape(-1, 64), q.reshape(-1, 64), idx.reshape(-1), f"forward {step}")
        seen.append(dense_effective_codes(book).clone())
    assert float((seen[0] - seen[1]).abs().max()) > 0.1
    mod.eval()
    x = torch.randn((4, 300, 64), generator=gen, device=DEV) * 0.5 - 1.0
    with torch.no_grad():
        q, idx, _ = mod(x)
    _assert_dense(book, x.reshape(-1, 64), q.reshape(-1, 64), idx.reshape(-1), "eval forward")


def _both_paths(make, x, steps=2, **fwd):
    """Run `steps` training forwards natively and with VQ_NO_FUSED_AFFINE=1 on twins of one module -> [(outputs, module)]"""
    torch.manual_seed(9)
    first = make().train()
    book = first._codebook
    with torch.no_grad():  # codes and warm EMA statistics on the scale of the rows, as in the fixtures: the tolerances of the
        # buffers are absolute (1e-6 / 1e-5), i.e. meant for values of order one -- a cold codebook (cluster_size 0) sends
        # every code without a hit to ~1e3 through the Laplace smoothing
        book.embeddings.copy_(torch.randn(book.embeddings.shape))
        book.embed_avg.copy_(book.embeddings * 10.0)
        book.cluster_size.fill_(10.0)
    first = first.to(DEV)
    runs = []
    for switch in (False, True):
        mod = copy.deepcopy(first)
        if switch:
            os.environ["VQ_NO_FUSED_AFFINE"] = "1"
        with torch.no_grad():
            outs = [mod(x * (1.0 + 0.5 * s) + 0.25 * s, **fwd) for s in range(steps)]
        os.environ.pop("VQ_NO_FUSED_AFFINE", None)
        runs.append((outs, mod))
    return runs


def _assert_paths_agree(runs):
    (a, mod_a), (b, mod_b) = runs
    for oa, ob in zip(a, b):
        assert torch.equal(oa[1], ob[1])
        np.testing.assert_allclose(oa[0].cpu().numpy(), ob[0].cpu().numpy(), atol=1e-5, rtol=0)
        np.testing.assert_allclose(oa[2].cpu().numpy(), ob[2].cpu().numpy(), atol=1e-5, rtol=1e-5)
    sa, sb = mod_a.state_dict(), mod_b.state_dict()
    assert list(sa) == list(sb)
    for key in sa:
        tight = any(n in key for n in STATS) or "cluster_size" in key
        np.testing.assert_allclose(sa[key].cpu().numpy(), sb[key].cpu().numpy(), rtol=1e-6 if tight else 1e-4,
                                   atol=1e-6 if tight else 1e-5, err_msg=key)


def test_head_strided_and_channel_first_inputs():
    """Per-head codebooks search the permuted [heads, rows, d] view of the (row, head) buffer -- the statistics kernel reads
    it in place -- and a channel-first input arrives as a permuted view as well."""
    import vector_quantization as vq

    gen = torch.Generator(device=DEV).manual_seed(21)
    x = torch.randn((3, 48, 10, 7), generator=gen, device=DEV)  # b, d, h, w

    def make():
        return vq.VectorQuantize(dim=48, heads=3, codebook_dim=16, separate_codebook_per_head=True, channel_last=False,
                                 codebook_params=_params(16, 40))

    runs = _both_paths(make, x)
    _assert_paths_agree(runs)
    book = runs[0][1]._codebook
    assert tuple(book.batch_mean.shape) == (3, 1, 16) and tuple(runs[0][0][0][0].shape) == (3, 48, 10, 7)
    assert not torch.equal(book.batch_mean[0], book.batch_mean[1])


def test_wide_rows():
    """D = 640 takes the sliced wide-row search; the statistics kernel covers it with three column groups."""
    import vector_quantization as vq

    gen = torch.Generator(device=DEV).manual_seed(22)
    x = torch.randn((2, 150, 640), generator=gen, device=DEV)
    runs = _both_paths(lambda: vq.VectorQuantize(dim=640, codebook_params=_params(640, 96)), x)
    _assert_paths_agree(runs)
    mod = runs[0][1].eval()
    with torch.no_grad():
        q, idx, _ = mod(x)
    _assert_dense(mod._codebook, x.reshape(-1, 640), q.reshape(-1, 640), idx.reshape(-1), "wide rows")


def test_graphed_eval_forward_equals_eager():
    """In-place statistics and no host synchronisation: an eval-mode affine module replays as a hipGraph; every replay moves
    the batch statistics exactly as an eager forward does."""
    import vector_quantization as vq
    from vector_quantization.graphs import GraphedForward

    torch.manual_seed(4)
    mod = vq.VectorQuantize(dim=64, codebook_params=_params(64, 128)).to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(31)
    with torch.no_grad():
        mod(torch.randn((4, 200, 64), generator=gen, device=DEV))
    mod.eval()
    twin = copy.deepcopy(mod)
    example = torch.randn((4, 200, 64), generator=gen, device=DEV)
    warmup = 2
    fast = GraphedForward(mod, example, warmup=warmup)
    with torch.no_grad():
        for _ in range(warmup):  # the warm-up forwards of the capture moved the batch statistics
            twin(example)
        for step in range(3):
            x = torch.randn((4, 200, 64), generator=gen, device=DEV) * (1.0 + step) - 0.5 * step
            q, idx, loss = fast(x)
            wq, widx, wloss = twin(x)
            assert torch.equal(idx, widx), f"replay {step}"
            assert torch.equal(q, wq) and torch.equal(loss, wloss)
            for n in STATS:
                assert torch.equal(getattr(mod._codebook, n), getattr(twin._codebook, n)), (step, n)
