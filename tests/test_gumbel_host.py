"""CPU suite: the Gumbel straight-through / reinmax relaxations through the chunked path (the CPU oracle stands in for the
native similarities), against fixtures captured from the imported reference (tests/golden/make_golden_gumbel.py)."""
from __future__ import annotations

import pytest
import torch

from gumbel_cases import GUMBEL_CASES
from gumbel_run import assert_grad_close, check_fixture, closed_form64, run_fixture
from helpers import OracleBackend


@pytest.fixture(autouse=True)
def _oracle_backend(oracle):
    from vector_quantization import search

    search.set_backend(OracleBackend)
    yield
    search.set_backend(None)


@pytest.mark.parametrize("name", list(GUMBEL_CASES))
def test_fixture_through_the_chunked_path(name):
    check_fixture(name)


def test_inactive_relaxations_equal_the_plain_path():
    """temperature = 0 and GumbelParams(training=False): the reference returns before the softmax."""
    a0, _ = run_fixture("t0")
    a1, _ = run_fixture("not_training")
    for key in ("gx", "gcb", "quantize"):
        assert (a0[key] == a1[key]).all()
    assert not (a0["gcb"] == run_fixture("st_euclid")[0]["gcb"]).all()


def test_reinmax_without_straight_through_asserts_at_construction():
    from vector_quantization.codebook import Codebook
    from vector_quantization.codebooks import GumbelParams

    with pytest.raises(AssertionError, match="reinmax can only be turned on if using straight through gumbel softmax"):
        Codebook(dim=8, codebook_size=16, gumbel_params=GumbelParams(reinmax=True))


def test_stochastic_with_straight_through_still_raises():
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams, GumbelParams

    for extra in (dict(straight_through=True), dict(straight_through=True, reinmax=True)):
        mod = vq.VectorQuantize(dim=8, codebook_params=CodebookParams(
            dim=8, codebook_size=32, gumbel_params=GumbelParams(stochastic=True, **extra)))
        with pytest.raises(NotImplementedError):
            mod(torch.randn(2, 10, 8))


def test_eval_mode_gathers_by_index():
    """codebooks.py:393-397: no relaxation outside train mode -- x receives no gradient from an eval-mode gather."""
    from vector_quantization.codebook import Codebook
    from vector_quantization.codebooks import GumbelParams

    mod = Codebook(dim=8, codebook_size=16, ema_update=False, learnable_codebook=True,
                   gumbel_params=GumbelParams(straight_through=True)).eval()
    x = torch.randn(1, 20, 8, requires_grad=True)
    q, ind, _ = mod(x, return_similarities=False)
    q.sum().backward()
    assert x.grad is None or not bool(x.grad.any())
    want = torch.zeros(16, 8).index_add_(0, ind[0], torch.ones(20, 8))
    assert torch.equal(mod.embeddings.grad[0], want)


@pytest.mark.parametrize("reinmax", [False, True], ids=["straight_through", "reinmax"])
@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_chunking_does_not_change_the_result(monkeypatch, metric, reinmax):
    from vector_quantization import gumbel, losses, search

    h, m, k, d = 2, 420, 24, 12
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(h, m, d, generator=gen) * (0.25 if metric == "dot" else 1.0)
    c = torch.randn(h, k, d, generator=gen)
    g = torch.randn(h, m, d, generator=gen)
    mt = search.DOT if metric == "dot" else search.EUCLID
    ind = OracleBackend.similarities(x, c, metric=mt).argmax(-1)

    def grads():
        xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
        (gumbel.relaxed_gather(xr, cr, ind, mt, 0.7, reinmax) * g).sum().backward()
        return xr.grad, cr.grad

    whole = grads()
    monkeypatch.setattr(losses, "CHUNK_BYTES", 4 * h * k * 128)  # 128 rows a chunk
    assert len(losses._row_slices(m, losses._rows_per_chunk(h, k))) >= 3
    parts = grads()
    _, gx64, _, gc64 = closed_form64(x, c, g, ind, 1 / 0.7, metric == "dot", reinmax)
    for got, one, want, what in ((parts[0], whole[0], gx64, "gx"), (parts[1], whole[1], gc64, "gc")):
        assert_grad_close(got, one, f"{what}: chunks vs one chunk", atol_of_max=2e-6, rtol=2e-5)
        assert_grad_close(got, want, f"{what}: chunks vs fp64")
