"""vq_ema_sizes_kernel / vq_ema_codes_kernel through direct native.ema_update calls, and vq_ema_accumulate_residual_kernel
(plus the atomics-free variant) through native.ema_accumulate_residual.

ema_update is compared with tests/train_dense.py's fp64 model under the derived bounds (that module's docstring has the
derivation; tests/test_train_dense_host.py shows that the reference's own fp32 ops stay within them and that a dropped
K * eps, head 0's total for every head and a missing 1e-12 clamp fall outside them on these very inputs), and bit for bit
where the result is exactly determined.  The residual statistics are compared with residual_stats_model: counts exactly,
sums within the order-free fp32 summation bound n_k 2^-23 sum |terms|."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import train_dense as td
from helpers import OracleBackend

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {"cs": 0.0, "avg": 0.0, "emb": 0.0, "res": 0.0}


def _native():
    from vector_quantization import native

    return native


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _update(inputs, decay, eps, l2norm):
    """-> (cluster_size', embed_avg', embeddings) on the GPU; checks that counts and sums are not written."""
    old, avg, counts, sums = (t.to(DEV).clone() for t in inputs)
    emb = torch.full_like(avg, -77.25)
    _native().ema_update(old, avg, emb, counts, sums, decay, eps, l2norm)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(counts), _bits(inputs[2])) and np.array_equal(_bits(sums), _bits(inputs[3]))
    return old, avg, emb


def _check_bounds(inputs, decay, l2norm, label):
    H, K, D = inputs[1].shape
    cs, avg, emb = (t.cpu().numpy() for t in _update(inputs, decay, td.EMA_EPS, l2norm))
    m = td.ema_update_model(*inputs, decay, td.EMA_EPS, l2norm)
    tol_cs, tol_avg, tol_e = td.ema_update_bounds(m, K, D, l2norm)
    assert np.isfinite(m["emb"]).all() and np.isfinite(tol_e).all()
    ratios = dict(cs=td.error_ratio(cs, m["cs"], tol_cs), avg=td.error_ratio(avg, m["avg"], tol_avg),
                  emb=td.error_ratio(emb, m["emb"], tol_e))
    for k, v in ratios.items():
        WORST[k] = max(WORST[k], v)
    print(f"ema_update {label} decay={decay} l2norm={l2norm}: error / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + " (worst so far " + " ".join(f"{k} {WORST[k]:.3f}" for k in ratios) + ")")
    assert max(ratios.values()) <= 1.0
    return m, emb


# ------------------------------------------------------------------------------------------------
# the fp64 model and the derived bounds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2norm", [False, True])
@pytest.mark.parametrize("decay", td.EMA_DECAYS)
@pytest.mark.parametrize("shape", td.EMA_SHAPES, ids=lambda s: "H%d-K%d-D%d" % s)
def test_ema_update_within_derived_bounds_of_fp64_model(shape, decay, l2norm):
    H, K, D = shape
    inputs = td.ema_case_inputs(H, K, D)
    m, emb = _check_bounds(inputs, decay, l2norm, str(shape))
    if K == 5000:  # the Laplace case: K eps stands three orders of magnitude above the tolerance
        assert K * m["eps"] / float(m["tot"].min()) >= 1e-3
    if K > 1:  # dead codes (no hits, no old size, zero rows): exactly zero, never NaN
        dead = ((inputs[0] == 0) & (inputs[2] == 0)).numpy()
        assert dead[:, 0].all() and not emb[dead].any()
    if l2norm:  # rows of live codes have norm 1
        live = (m["cs"] > 0) & (np.abs(m["avg"]).sum(-1) > 0)
        assert live.sum() >= max(1, (H * K) // 2)
        norms = np.sqrt((emb.astype(np.float64) ** 2).sum(-1))
        assert np.abs(norms[live] - 1.0).max() <= (D / 64 + 16) * td.U


@pytest.mark.parametrize("l2norm", [False, True])
@pytest.mark.parametrize("decay", td.EMA_DECAYS)
def test_heads_with_different_laplace_terms(decay, l2norm):
    """K eps / total is 1e-3 in head 0 and 3e-4 in head 1: a row that read the other head's total would miss the bound by
    two orders of magnitude (shown on the CPU in test_train_dense_host.py)."""
    _check_bounds(td.ema_laplace_heads_inputs(), decay, l2norm, "laplace-heads")


# ------------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 7, 64), (2, 1030, 8)], ids=str)
def test_decay_one_leaves_the_running_statistics_bit_identical(shape):
    inputs = td.ema_case_inputs(*shape)
    cs, avg, _emb = _update(inputs, 1.0, td.EMA_EPS, False)
    assert np.array_equal(_bits(cs), _bits(inputs[0])) and np.array_equal(_bits(avg), _bits(inputs[1]))


@pytest.mark.parametrize("D", [5, 64, 100])
def test_zero_rows_stay_zero_under_l2norm(D):
    """An all-zero embed_avg' row of a LIVE code (and of a dead one) has norm 0: the 1e-12 clamp makes it 0, not 0 / 0."""
    old, avg, counts, sums = td.ema_inputs(2, 33, D, 7300 + D)
    assert old[0, 3] > 0 and counts[0, 3] > 0
    avg[0, 3] = 0
    sums[0, 3] = 0
    _cs, avg2, emb = _update((old, avg, counts, sums), 0.8, td.EMA_EPS, True)
    emb = emb.cpu().numpy()
    assert np.isfinite(emb).all()
    assert not avg2[0, 3].any() and not emb[0, 3].any() and not emb[:, 0].any()
    assert np.abs(emb[0, 4]).max() > 0


# ------------------------------------------------------------------------------------------------
# head isolation
# ------------------------------------------------------------------------------------------------
def _klass(a):
    return np.where(np.isnan(a), 2, np.where(np.isinf(a), 1, 0))


@pytest.mark.parametrize("l2norm", [False, True])
@pytest.mark.parametrize("empty_head", [0, 1])
def test_a_head_with_total_zero_does_not_disturb_its_neighbour(empty_head, l2norm):
    inputs = td.ema_isolation_inputs(empty_head)
    other = 1 - empty_head
    cs, avg, emb = _update(inputs, 0.8, td.EMA_EPS, l2norm)
    alone = _update(tuple(t[other:other + 1] for t in inputs), 0.8, td.EMA_EPS, l2norm)
    for got, want in zip((cs, avg, emb), alone):
        assert np.array_equal(_bits(got[other:other + 1]), _bits(want))
    assert np.isfinite(emb[other].cpu().numpy()).all()
    ref = [t.clone() for t in inputs]
    ref_emb = torch.empty_like(ref[1])
    OracleBackend.ema_update(ref[0], ref[1], ref_emb, ref[2], ref[3], decay=0.8, eps=td.EMA_EPS, l2norm=l2norm)
    got_k, want_k = _klass(emb[empty_head].cpu().numpy()), _klass(ref_emb[empty_head].numpy())
    assert np.array_equal(got_k, want_k)
    assert (want_k == 2).any() and (l2norm or (want_k == 1).any())
    assert not cs[empty_head].any()


# ------------------------------------------------------------------------------------------------
# residual statistics
# ------------------------------------------------------------------------------------------------
RES_M, RES_K, RES_Q = 3000, 40, 4


def _residual_check(x, cb, idx, ste, share, deterministic, label):
    counts, sums = _native().ema_accumulate_residual(x.to(DEV), cb.to(DEV), idx.to(DEV), ste=ste, stages_share_codebook=share,
                                                     deterministic=deterministic)
    torch.cuda.synchronize()
    want_c, want_s, abs_s = td.residual_stats_model(x, cb, idx, ste=ste, share=share)
    assert np.array_equal(counts.cpu().numpy(), want_c.astype(np.float32))
    ratio = td.error_ratio(sums.cpu().numpy(), want_s, td.residual_sums_bound(want_c, abs_s))
    WORST["res"] = max(WORST["res"], ratio)
    print(f"ema_accumulate_residual {label} ste={ste} share={share} deterministic={deterministic}: error / bound = {ratio:.3f} "
          f"(worst so far {WORST['res']:.3f})")
    assert ratio <= 1.0
    return counts, sums, want_c


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("D", [5, 64, 300])
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("ste", [True, False])
def test_residual_statistics_with_dropped_stages(ste, share, H, D, deterministic):
    x, cb, idx = td.residual_inputs(H, RES_M, D, RES_Q, RES_K, 8000 + 10 * D + H, share=share)
    gone = idx < 0
    assert 0.25 < float(gone[..., -1].float().mean()) < 0.42 and bool(gone[..., 0].any())
    assert bool((gone[..., 1:] >= gone[..., :-1]).all())  # dropped from a stage onward
    counts, sums, want_c = _residual_check(x, cb, idx, ste, share, deterministic, f"H={H} D={D}")
    assert np.array_equal(want_c.sum(-1), (~gone).sum(1).numpy())
    if deterministic:
        for _ in range(2):  # bit for bit over 3 runs
            c2, s2 = _native().ema_accumulate_residual(x.to(DEV), cb.to(DEV), idx.to(DEV), ste=ste, stages_share_codebook=share,
                                                       deterministic=True)
            assert np.array_equal(_bits(c2), _bits(counts)) and np.array_equal(_bits(s2), _bits(sums))


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("D", [5, 300])
def test_rows_dropped_at_stage_zero_contribute_nothing(D, deterministic):
    x, cb, idx = td.residual_inputs(2, RES_M, D, RES_Q, RES_K, 8100 + D, share=False)
    never = idx[..., 0] < 0
    assert 100 < int(never.sum()) < RES_M
    nat = _native()
    a = nat.ema_accumulate_residual(x.to(DEV), cb.to(DEV), idx.to(DEV), ste=True, deterministic=True)
    poisoned = torch.where(never[..., None], torch.full_like(x, 1e30), x)
    b = nat.ema_accumulate_residual(poisoned.to(DEV), cb.to(DEV), idx.to(DEV), ste=True, deterministic=True)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    c, s = nat.ema_accumulate_residual(poisoned.to(DEV), cb.to(DEV), idx.to(DEV), ste=True, deterministic=deterministic)
    assert float(s.abs().max()) < 1e6 and torch.equal(c, a[0])


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("ste", [True, False])
def test_a_chain_ends_at_its_first_dropped_stage(ste, deterministic):
    """Live indices AFTER a dropped stage are not reached (the kernel leaves the stage loop; the atomics-free variant must
    agree with it).  Quantize dropout never produces such rows, a caller's own index tensor may."""
    x, cb, idx = td.residual_inputs(2, RES_M, 64, RES_Q, RES_K, 8200, share=False)
    g = torch.Generator().manual_seed(8201)
    revive = (idx[..., -1] < 0) & (torch.rand(idx.shape[:2], generator=g) < 0.5)
    idx[..., -1] = torch.where(revive, torch.randint(0, RES_K, idx.shape[:2], generator=g), idx[..., -1])
    assert int(revive.sum()) > 100
    _, _, want_c = _residual_check(x, cb, idx, ste, False, deterministic, "revived last stage")
    assert int(want_c[:, -1].sum()) == int((idx >= 0).all(-1).sum()) < int((idx[..., -1] >= 0).sum())
