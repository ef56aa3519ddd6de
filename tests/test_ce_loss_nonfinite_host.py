"""CPU suite: losses.cross_entropy_to_codes with non-finite rows (the CPU oracle stands in for the native sweep).

ATen's F.cross_entropy(..., ignore_index=-1) never looks at an ignored row: NaN or inf in it leaves the loss alone.  The
host side must select the rows it sums, not multiply them by 0 (NaN * 0 is NaN)."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from helpers import OracleBackend

NAN, INF = float("nan"), float("inf")
H, M, K = 2, 70, 50


@pytest.fixture(autouse=True)
def _oracle_backend(oracle):
    from vector_quantization import search

    search.set_backend(OracleBackend)
    yield
    search.set_backend(None)


def _inputs(D, metric):
    g = torch.Generator().manual_seed(40 + D + metric)
    x = torch.randn((H, M, D), generator=g)
    c = torch.randn((H, K, D), generator=g)
    target = torch.randint(0, K, (H, M), generator=g)
    target[:, ::5] = -1
    return x, c, target


def _poison_ignored_rows(x, D):
    """NaN, +inf, -inf, a whole row of inf, +inf and -inf together: all on rows m % 5 == 0.  Returns (head, row) of each."""
    x[0, 0, 3] = NAN
    x[0, 5, :] = INF
    x[1, 10, 0] = -INF
    x[1, 15, D - 1] = NAN
    x[0, 20, 0], x[0, 20, 1] = INF, -INF
    x[1, 65, D // 2] = INF
    return [(0, 0), (0, 5), (1, 10), (1, 15), (0, 20), (1, 65)]


@pytest.mark.parametrize("D", [64, 600])
@pytest.mark.parametrize("metric", [0, 1])
def test_poisoned_ignored_rows_leave_the_loss_alone(D, metric):
    from vector_quantization import losses

    x, c, target = _inputs(D, metric)
    rows = _poison_ignored_rows(x, D)
    assert all(int(target[h, m]) == -1 for h, m in rows)
    loss = losses.cross_entropy_to_codes(x, c, target, metric)
    assert bool(torch.isfinite(loss)), float(loss)
    sims = OracleBackend.similarities(x, c, metric=metric).double()
    want = F.cross_entropy(sims.reshape(-1, K), target.reshape(-1), ignore_index=-1)
    assert bool(torch.isfinite(want))
    rel = abs(float(loss) - float(want)) / abs(float(want))
    print(f"D {D} metric {metric}: loss {float(loss):.8f}, ATen on the oracle's similarities {float(want):.8f}, relative {rel:.2e}")
    assert rel <= 1e-6
    zeroed = x.clone()
    for h, m in rows:
        zeroed[h, m] = 0.0
    assert torch.equal(loss, losses.cross_entropy_to_codes(zeroed, c, target, metric)), "the ignored rows' values reached the loss"


@pytest.mark.parametrize("D", [64, 600])
@pytest.mark.parametrize("metric", [0, 1])
def test_a_poisoned_valid_row_makes_the_loss_nan(D, metric):
    """As ATen: a NaN in a row that counts."""
    from vector_quantization import losses

    x, c, target = _inputs(D, metric)
    _poison_ignored_rows(x, D)
    assert int(target[0, 1]) >= 0
    x[0, 1, 2] = NAN
    sims = OracleBackend.similarities(x, c, metric=metric).double()
    want = F.cross_entropy(sims.reshape(-1, K), target.reshape(-1), ignore_index=-1)
    loss = losses.cross_entropy_to_codes(x, c, target, metric)
    print(f"D {D} metric {metric}: loss {float(loss)}, ATen {float(want)}")
    assert bool(torch.isnan(want)) and bool(torch.isnan(loss))
