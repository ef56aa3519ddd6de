"""GPU: the dead-code expiry kernels (vq_expire_codes_f32) through native.expire_codes -- the exact state they leave, the rows
they pick against the host statement of the rule (tests/expire_rule.py), every edge of the scan and of the copy, the
normalisation against fp64, the residual chain bit for bit, poisoned buffers, and the registered custom op.

The entry point's case stands in the table of native calls (tests/native_cases.py), so that the poison suites run it like
every other one and find its kernels launched."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import alloc_poison as ap
import expire_rule as er
from native_cases import DEV, EXPIRE_SEED

pytestmark = pytest.mark.gpu

SEED = EXPIRE_SEED


def _native():
    from vector_quantization import native

    native.load()
    return native


def _seed(words=SEED):
    return torch.tensor(list(words), dtype=torch.int64, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu()


def _random_bits(shape, seed):
    """fp32 tensors of random bit patterns (NaNs, infinities and denormals among them): 'not written' is visible bit for bit."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2 ** 31), 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)


def _state(H, K, D, sizes, seed):
    """(cluster_size, embed_avg, embeddings) on the device, the two code buffers filled with random bits."""
    return sizes.to(DEV).contiguous(), _random_bits((H, K, D), seed).to(DEV), _random_bits((H, K, D), seed + 1).to(DEV)


def _run(sizes, pool, *, D=None, threshold=2.0, reset=2.0, l2norm=False, seed=SEED, chain=None, stage=0, state_seed=11):
    native = _native()
    H, K = sizes.shape
    D = D if D is not None else (pool.shape[-1] if pool is not None else chain[0].shape[-1])
    cs, avg, emb = _state(H, K, D, sizes, state_seed)
    before = tuple(t.clone() for t in (cs, avg, emb))
    n, picked = native.expire_codes(cs, avg, emb, pool, chain=chain, stage=stage, threshold=threshold, reset_cluster_size=reset,
                                    l2norm=l2norm, seed=_seed(seed), want_picked=True)
    torch.cuda.synchronize()
    return dict(cs=cs, avg=avg, emb=emb, before=before, n=n.cpu(), picked=picked.cpu())


def _check_exact(r, sizes, rows, threshold, reset, N, seed=SEED):
    """The whole contract for l2norm == 0: ``rows`` [H | 1, N, D] is the pool (CPU)."""
    H, K = sizes.shape
    dead = sizes < threshold  # torch's fp32 comparison
    assert torch.equal(r["n"].long(), dead.sum(dim=1))
    assert torch.equal(r["picked"] >= 0, dead), "the dead set is not torch's cluster_size < threshold"
    cs0, avg0, emb0 = r["before"]
    live = ~dead
    assert torch.equal(_bits(r["cs"])[live], _bits(cs0)[live])
    assert torch.equal(_bits(r["avg"])[live], _bits(avg0)[live]) and torch.equal(_bits(r["emb"])[live], _bits(emb0)[live])
    for h in range(H):
        ks = torch.nonzero(dead[h])[:, 0]
        n_dead = len(ks)
        sel = r["picked"][h, ks]
        assert bool(((sel >= 0) & (sel < N)).all())
        if n_dead <= N:
            assert len(set(sel.tolist())) == n_dead, "rows picked twice although there are enough of them"
        want = er.select(np.array(seed, dtype=np.int64), h, np.arange(n_dead), n_dead, N)
        assert np.array_equal(sel.numpy(), want), f"head {h}: the kernel does not pick the rows the header's rule picks"
        row = rows[h if rows.shape[0] > 1 else 0][sel]
        assert torch.equal(_bits(r["emb"][h, ks]), _bits(row))
        assert torch.equal(_bits(r["avg"][h, ks]), _bits(row * torch.tensor(reset, dtype=torch.float32)))
        assert torch.equal(r["cs"][h, ks].cpu(), torch.full((n_dead,), reset))


def _sizes_from_set(H, K, seed):
    values = torch.tensor([0.0, 1.0, float(np.nextafter(np.float32(2), np.float32(0))), 2.0, 2.5, float("nan"), float("inf"),
                           float("-inf")])
    g = torch.Generator().manual_seed(seed)
    return values[torch.randint(0, len(values), (H, K), generator=g)]


def _pool(H, N, D, seed):
    return torch.randn((H, N, D), generator=torch.Generator().manual_seed(seed))


def test_exact_state():
    H, K, D, N = 3, 37, 5, 50
    sizes, rows = _sizes_from_set(H, K, 1), _pool(H, N, D, 2)
    assert {0.0, 2.0}.issubset(set(sizes.flatten().tolist())) and bool(torch.isnan(sizes).any())
    r = _run(sizes, rows.to(DEV))
    _check_exact(r, sizes, rows, 2.0, 2.0, N)
    again = _run(sizes, rows.to(DEV))
    for name in ("cs", "avg", "emb", "picked"):
        assert torch.equal(_bits(again[name]), _bits(r[name])), "the same seed gives another result"
    other = _run(sizes, rows.to(DEV), seed=(5, 6))
    _check_exact(other, sizes, rows, 2.0, 2.0, N, seed=(5, 6))
    assert not torch.equal(other["picked"], r["picked"])


def test_reset_and_threshold_are_fp32_values():
    sizes = torch.tensor([[0.05, 0.1, float(np.float32(0.1)) * 2, 3.0]])
    rows = _pool(1, 9, 4, 3)
    r = _run(sizes, rows.to(DEV), threshold=0.1, reset=0.3)
    assert r["n"].tolist() == [int((sizes < 0.1).sum())]
    _check_exact(r, sizes, rows, 0.1, float(np.float32(0.3)), 9)


def test_nothing_dead():
    sizes, rows = torch.full((2, 70), 2.0), _pool(2, 5, 8, 4)
    r = _run(sizes, rows.to(DEV))
    assert r["n"].tolist() == [0, 0] and bool((r["picked"] == -1).all())
    for got, was in zip((r["cs"], r["avg"], r["emb"]), r["before"]):
        assert torch.equal(_bits(got), _bits(was))


def test_everything_dead_is_a_permutation():
    sizes, rows = torch.zeros((2, 64)), _pool(2, 64, 8, 5)
    r = _run(sizes, rows.to(DEV))
    _check_exact(r, sizes, rows, 2.0, 2.0, 64)
    for h in range(2):
        assert sorted(r["picked"][h].tolist()) == list(range(64))
    assert r["picked"][0].tolist() != r["picked"][1].tolist()


def test_more_dead_codes_than_rows_draws_with_replacement():
    sizes, rows = torch.zeros((2, 40)), _pool(2, 7, 6, 6)
    r = _run(sizes, rows.to(DEV))
    _check_exact(r, sizes, rows, 2.0, 2.0, 7)


@pytest.mark.parametrize("K,N,D", [(5, 1, 4), (1, 6, 4), (9, 12, 1), (9, 12, 3), (9, 12, 260), (3, 4, 2048)],
                         ids=lambda v: str(v))
def test_small_and_odd_shapes(K, N, D):
    sizes = torch.zeros((2, K))
    if K > 1:
        sizes[:, 1::2] = 5.0
    rows = _pool(2, N, D, 7 + D)
    _check_exact(_run(sizes, rows.to(DEV)), sizes, rows, 2.0, 2.0, N)


def test_ranks_cross_every_edge_of_the_scan():
    K, N, D = 4099, 16, 4
    sizes = torch.full((2, K), 3.0)
    sizes[0, [0, 255, 256, 1023, 1024, 4098]] = 0.0
    sizes[1, 1020:1030] = 1.0
    sizes[1, 2047:2050] = 1.0
    rows = _pool(2, N, D, 8)
    r = _run(sizes, rows.to(DEV))
    assert r["n"].tolist() == [6, 13]
    _check_exact(r, sizes, rows, 2.0, 2.0, N)
    # a long codebook with every third code dead: 22 passes of the scan, ranks beyond one pass
    K = 65536 // 3
    sizes = torch.full((1, K), 3.0)
    sizes[0, ::3] = 0.0
    rows = _pool(1, K, 3, 9)
    _check_exact(_run(sizes, rows.to(DEV)), sizes, rows, 2.0, 2.0, K)


def test_strided_shared_and_misaligned_pools():
    H, K, D, N = 2, 21, 8, 30
    sizes = torch.zeros((H, K))
    sizes[:, ::4] = 9.0
    wide = torch.randn((H, N, D + 5), generator=torch.Generator().manual_seed(10)).to(DEV)
    pool = wide[:, :, :D]  # pool_rs > D
    assert pool.stride(1) == D + 5
    _check_exact(_run(sizes, pool), sizes, pool.cpu(), 2.0, 2.0, N)
    shared = torch.randn((1, N, D), generator=torch.Generator().manual_seed(11)).to(DEV)
    _check_exact(_run(sizes, shared), sizes, shared.cpu(), 2.0, 2.0, N)  # one pool for both heads
    _check_exact(_run(sizes, shared.expand(H, N, D)), sizes, shared.cpu(), 2.0, 2.0, N)  # pool_hs == 0
    flat = torch.randn((H * N * D + 1,), generator=torch.Generator().manual_seed(12)).to(DEV)
    off = flat[1:].view(H, N, D)  # starts 4 bytes off the 16-byte grid
    assert off.data_ptr() % 16 == 4
    _check_exact(_run(sizes, off), sizes, off.cpu(), 2.0, 2.0, N)


@pytest.mark.parametrize("D", [1, 3, 64, 260, 2048])
def test_l2norm_against_fp64(D):
    H, K, N = 2, 12, 11  # eleven dead codes, eleven rows: every row is picked once
    sizes = torch.zeros((H, K))
    sizes[:, 5] = 4.0
    rows = _pool(H, N, D, 20 + D) * 3.0
    rows[:, 2] = 0.0          # an all-zero row stays zero
    rows[:, 3] *= 1e-18       # squares that underflow: the 1e-12 clamp takes over
    r = _run(sizes, rows.to(DEV), l2norm=True, reset=1.5)
    dead = sizes < 2.0
    assert set(r["picked"][dead].tolist()) >= {2, 3}, "the case does not pick the rows it is about"
    tol = (D + 4) * 2.0 ** -24
    worst = 0.0
    for h in range(H):
        for k in torch.nonzero(dead[h])[:, 0].tolist():
            row = rows[h, r["picked"][h, k]].double()
            want = row / row.norm().clamp_min(1e-12)
            got = r["emb"][h, k].cpu().double()
            if not bool(row.any()):
                assert not bool(got.any())
            err = ((got - want).abs() / want.abs().clamp_min(1e-300))[want != 0]
            worst = max(worst, float(err.max()) if err.numel() else 0.0)
            assert torch.equal(_bits(r["avg"][h, k]), _bits(r["emb"][h, k].cpu() * torch.tensor(1.5)))
    print(f"D = {D}: largest relative error {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol
    live = ~dead
    assert torch.equal(_bits(r["emb"])[live], _bits(r["before"][2])[live])


@pytest.mark.parametrize("share", [False, True], ids=["per-stage", "shared"])
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_residual_chain_rows_bit_for_bit(share, stage):
    from vector_quantization.residual import _residual_chain

    Q, K, D, M = 3, 8, 6, 20
    g = torch.Generator().manual_seed(30 + stage)
    x = torch.randn((M, D), generator=g).to(DEV)
    codes = (torch.randn((1 if share else Q, K, D), generator=g) * 0.5).to(DEV)
    idx = torch.randint(0, K, (M, Q), generator=g).to(DEV)
    chain = _residual_chain(x, codes.expand(Q, K, D), idx, ste=True)[stage]
    sizes = torch.zeros((1, K))
    sizes[0, 3] = 7.0
    r = _run(sizes, None, chain=(x, codes, idx), stage=stage)
    _check_exact(r, sizes, chain[None].cpu(), 2.0, 2.0, M)
    # the rows of a strided input (one group of a grouped stack) and normalised rows go through the same chain
    wide = torch.randn((M, 2 * D), generator=g).to(DEV)
    r = _run(sizes, None, chain=(wide[:, D:], codes, idx), stage=stage)
    _check_exact(r, sizes, _residual_chain(wide[:, D:], codes.expand(Q, K, D), idx, ste=True)[stage][None].cpu(), 2.0, 2.0, M)


def test_poisoned_workspace_and_picked(monkeypatch):
    """Every allocation of the binding (workspace, picked, n_expired's zeros aside) filled with each poison in turn: the
    results are the same bit for bit, every picked entry is defined, the guard bands stay as they were."""
    native = _native()
    H, K, D, N = 2, 1500, 12, 400
    sizes, rows = _sizes_from_set(H, K, 40), _pool(H, N, D, 41).to(DEV)
    runs = []
    for pattern in ap.PATTERNS:
        proxy = ap.TorchProxy(pattern)
        with monkeypatch.context() as m:
            m.setattr(native, "torch", proxy)
            cs, avg, emb = _state(H, K, D, sizes, 42)
            n, picked = native.expire_codes(cs, avg, emb, rows, threshold=2.0, reset_cluster_size=2.0, l2norm=False, seed=_seed(),
                                            want_picked=True)
            torch.cuda.synchronize()
        proxy.check_guards()
        assert any("expire_codes" in s for s in proxy.sites()) and any("_alloc_workspace" in s for s in proxy.sites())
        dead = sizes < 2.0
        assert torch.equal(picked.cpu() >= 0, dead) and bool((picked.cpu()[~dead] == -1).all()) and bool((picked.cpu() < N).all())
        runs.append((cs, avg, emb, n, picked))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))


def test_custom_op_gives_the_wrappers_result():
    native = _native()
    import vector_quantization  # noqa: F401  (registers the ops)

    H, K, D, N = 2, 33, 16, 40
    sizes, rows = _sizes_from_set(H, K, 50), _pool(H, N, D, 51).to(DEV)
    a, b = _state(H, K, D, sizes, 52), _state(H, K, D, sizes, 52)
    _, picked = native.expire_codes(*a, rows, threshold=2.0, reset_cluster_size=2.0, l2norm=True, seed=_seed(), want_picked=True)
    got = torch.ops.vq_mi355x.expire_codes(*b, rows, None, None, None, 0, 2.0, 2.0, True, _seed())
    assert torch.equal(got, picked)
    for s, t in zip(a, b):
        assert torch.equal(_bits(s), _bits(t))
    torch.library.opcheck(torch.ops.vq_mi355x.expire_codes.default,
                          (*_state(H, K, D, sizes, 52), rows, None, None, None, 0, 2.0, 2.0, True, _seed()),
                          test_utils=("test_schema", "test_faketensor"))


def test_degenerate_calls_and_bad_arguments():
    native = _native()
    lib = native.load()
    sizes = torch.zeros((1, 4))
    cs, avg, emb = _state(1, 4, 3, sizes, 60)
    n, picked = native.expire_codes(cs, avg, emb, torch.empty((1, 0, 3), device=DEV), threshold=2.0, reset_cluster_size=2.0,
                                    l2norm=False, seed=_seed(), want_picked=True)
    assert n.tolist() == [0] and bool((picked == -1).all()) and torch.equal(cs.cpu(), sizes)
    ws = torch.empty(64, device=DEV)
    args = lambda D, seed, pool: (cs.data_ptr(), avg.data_ptr(), emb.data_ptr(), pool, 3, 0, 5, None, 0, 1, 4, D, 2.0, 2.0, 0, seed, None,
                                  None, ws.data_ptr(), None)
    pool = torch.zeros((1, 5, 3), device=DEV)
    assert lib.vq_expire_codes_f32(*args(0, _seed().data_ptr(), pool.data_ptr())) == -1
    assert lib.vq_expire_codes_f32(*args(3, None, pool.data_ptr())) == -1
    assert lib.vq_expire_codes_f32(*args(3, _seed().data_ptr(), None)) == -1 and b"pool" in lib.vq_last_error()
    assert lib.vq_expire_workspace_bytes(3, 100) >= 3 * 4 + 3 * 100 * 4
    torch.cuda.synchronize()
