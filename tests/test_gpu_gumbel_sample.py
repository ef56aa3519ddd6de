"""GPU suite for the fused Gumbel-max sampling sweep (vq_gumbel_sample_f32) and its noise hook (vq_gumbel_noise_f32).

The kernel is random but exactly checkable: the noise is a documented function of (seed, head, row, code), the hook writes
it out, and the sampled code must be the first index of the maximum of  similarities * tau + noise  computed with separate
torch ops from the library's own similarity output -- every row, no tolerance.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from test_gumbel_sample_host import gumbel64, noise_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EUCLID, DOT = 0, 1
SHAPES = [(1, 40, 1, 16), (2, 33, 7, 5), (1, 300, 256, 64), (4, 130, 520, 64), (1, 111, 301, 100), (1, 70, 1000, 128),
          (1, 96, 512, 256), (1, 65, 100, 400), (1, 40, 70, 512)]
TEMPERATURES = (0.5, 1.0, 2.0)


def _seed(a, b):
    return torch.tensor([a, b], dtype=torch.int64, device=DEV)


def _data(H, M, K, D, salt=0):
    gen = torch.Generator().manual_seed(1000 * H + 100 * K + D + salt)
    return torch.randn(H, M, D, generator=gen).to(DEV), torch.randn(H, K, D, generator=gen).to(DEV)


def _first_argmax(key: torch.Tensor) -> np.ndarray:
    """ATen's argmax rule, spelled out on the CPU: a NaN is the maximum, the first of the maxima wins."""
    k = key.cpu().numpy()
    nan = np.isnan(k)
    top = np.where(nan, -np.inf, k).max(axis=-1, keepdims=True)
    is_max = np.where(nan.any(axis=-1, keepdims=True), nan, k == top)
    return is_max.argmax(axis=-1)  # first True


def _expected(x, cb, metric, temperature, seed):
    """First index of the maximum of sims * tau32 + noise: similarities and noise from the library, the key from two
    separate torch kernels (one rounding each), the reduction on the CPU."""
    from vector_quantization import native

    H, M, _ = x.shape
    K = cb.shape[1]
    sims = native.similarities(x, cb, metric=metric)
    noise = native.gumbel_noise(seed, H, M, K)
    tau32 = float(np.float32(1.0 / temperature))
    key = torch.add(torch.mul(sims, tau32), noise)
    return _first_argmax(key)


def _sample(x, cb, metric, temperature, seed):
    from vector_quantization import native

    idx = native.sample_codes(x, cb, metric=metric, tau=1.0 / temperature, seed=seed)
    assert idx is not None and idx.dtype == torch.int64 and tuple(idx.shape) == tuple(x.shape[:2])
    return idx


# ------------------------------------------------------------------------------------------------ the noise
@pytest.mark.parametrize("H,M,K", [(2, 33, 7), (1, 130, 301)])
def test_noise_bits_equal_numpy_philox(H, M, K):
    from vector_quantization import native

    words = (0x0123456789ABCDEF, -0x0FEDCBA987654321)  # (seed[1] negative: the 64-bit sum of the upper counter half wraps)
    noise, bits = native.gumbel_noise(_seed(*words), H, M, K, want_bits=True)
    got = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, noise_bits(words, H, M, K))
    assert noise.shape == (H, M, K) and bool(torch.isfinite(noise).all())


@pytest.mark.parametrize("H,M,K", [(2, 33, 7), (1, 130, 301), (1, 2000, 1000)])
def test_noise_values_against_fp64(H, M, K):
    """|noise - g64| <= 1e-4 absolute, g64 the fp64 double-clamped transform of the same bits.  The last shape has 2e6
    entries: about 20 of them sit on the inner clamp (1 - u < 1e-5) and thousands in the region where -log(u) is tiny."""
    from vector_quantization import native

    noise, bits = native.gumbel_noise(_seed(77, 99), H, M, K, want_bits=True)
    words = bits.cpu().numpy().view(np.uint32)
    want = gumbel64(words)
    err = np.abs(noise.cpu().numpy().astype(np.float64) - want)
    u = (words >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    near_one = u > 1 - 2.0 ** -6
    print(f"noise ({H},{M},{K}): worst |err| {err.max():.3e}, worst for 1-u < 2^-6 "
          f"{(err[near_one].max() if near_one.any() else 0.0):.3e}, entries on the inner clamp {int((u > 1 - 1e-5).sum())}")
    assert err.max() <= 1e-4
    assert want.min() >= -np.log(-np.log(1e-5)) - 1e-12 and want.max() <= -np.log(1e-5) + 1e-12


# ------------------------------------------------------------------------------------------------ exact selection
@pytest.mark.parametrize("metric", [EUCLID, DOT], ids=["euclid", "dot"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_is_first_argmax_of_the_key(shape, metric):
    H, M, K, D = shape
    x, cb = _data(H, M, K, D)
    seed = _seed(20260101 + K, -D)
    for temperature in TEMPERATURES:
        got = _sample(x, cb, metric, temperature, seed).cpu().numpy()
        want = _expected(x, cb, metric, temperature, seed)
        assert np.array_equal(got, want), (shape, metric, temperature, int((got != want).sum()))
    assert got.min() >= 0 and got.max() < K


@pytest.mark.parametrize("pad", [8, 3], ids=["stride_D+8", "stride_D+3"])
def test_selection_with_strided_rows(pad):
    H, M, K, D = 2, 130, 301, 64
    wide, cb = _data(H, M, K, D + pad)
    cb = cb[..., :D].contiguous()
    x = wide[..., :D]
    assert x.stride(1) == D + pad
    seed = _seed(5, 6)
    for metric in (EUCLID, DOT):
        got = _sample(x, cb, metric, 0.8, seed).cpu().numpy()
        assert np.array_equal(got, _expected(x, cb, metric, 0.8, seed))
        assert np.array_equal(got, _sample(x.contiguous(), cb, metric, 0.8, seed).cpu().numpy())


@pytest.mark.parametrize("metric", [EUCLID, DOT], ids=["euclid", "dot"])
def test_selection_at_a_tiny_temperature_resolves_ties_to_the_first_index(metric):
    """temperature 1e-6: keys of ~1e6 .. 1e7 with a spacing of 1/16 .. 1, so the O(1) noise survives only in its leading
    bits and equal keys are common -- more so with every code present twice."""
    H, M, K, D = 1, 300, 256, 64
    x, cb = _data(H, M, K, D)
    cb[0, 128:] = cb[0, :128]
    seed = _seed(31, 41)
    got = _sample(x, cb, metric, 1e-6, seed).cpu().numpy()
    want = _expected(x, cb, metric, 1e-6, seed)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("metric", [EUCLID, DOT], ids=["euclid", "dot"])
def test_non_finite_inputs_follow_atens_argmax(metric):
    H, M, K, D = 1, 40, 33, 16
    x, cb = _data(H, M, K, D)
    seed = _seed(3, 4)
    xr = x.clone()
    xr[0, 5, 3] = float("nan")
    got = _sample(xr, cb, metric, 1.0, seed)
    assert int(got[0, 5]) == 0  # every key of the row is NaN: the first code
    assert np.array_equal(got.cpu().numpy(), _expected(xr, cb, metric, 1.0, seed))
    for poisoned, winner in (((17,), 17), ((6, 17), 6), ((17, 22), 17), ((32, 6), 6)):
        c = cb.clone()
        for k in poisoned:
            c[0, k, 2] = float("nan")
        got = _sample(x, c, metric, 1.0, seed)
        assert bool((got == winner).all()), (poisoned, got)
        assert np.array_equal(got.cpu().numpy(), _expected(x, c, metric, 1.0, seed))


# ------------------------------------------------------------------------------------------------ the draws
def test_draws_do_not_depend_on_the_launch_geometry():
    H, M, K, D = 2, 333, 301, 64
    x, cb = _data(H, M, K, D)
    x[1], cb[1] = x[0], cb[0]
    seed = _seed(123456789, 987654321)
    whole = _sample(x, cb, EUCLID, 1.0, seed)
    part = _sample(x[:, :100].contiguous(), cb, EUCLID, 1.0, seed)
    assert torch.equal(whole[:, :100], part)  # the first rows of a longer call
    assert not torch.equal(whole[0], whole[1])  # the head enters the counter
    from vector_quantization import native

    assert torch.equal(native.gumbel_noise(seed, H, 100, K), native.gumbel_noise(seed, H, M, K)[:, :100])


def test_equal_seeds_equal_draws():
    x, cb = _data(1, 500, 64, 16)
    a = _sample(x, cb, EUCLID, 1.0, _seed(7, 7))
    b = _sample(x, cb, EUCLID, 1.0, _seed(7, 7))
    c = _sample(x, cb, EUCLID, 1.0, _seed(7, 8))
    d = _sample(x, cb, EUCLID, 1.0, _seed(8, 7))
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)


DIST_SEED = (20261018, 42)
DIST_ROWS = 20000


def distribution_inputs(K, D):
    """One row and a codebook, on the CPU (the host-side check of DIST_SEED uses the same inputs)."""
    gen = torch.Generator().manual_seed(4321 + K)
    codes = torch.randn(1, K, D, generator=gen)
    row = torch.randn(1, 1, D, generator=gen) * 0.5
    return row, codes


@pytest.mark.parametrize("K,D", [(8, 4), (70, 16)])
def test_frequencies_follow_the_softmax(K, D):
    """20000 copies of one row at temperature 0.7: |freq - softmax(s / T)| <= 5 sigma + 1e-4 per code (binomial sigma).
    The seed is fixed, so the outcome is deterministic; the numpy Philox + fp64 transform on these inputs passes the same
    bound on the CPU (checked before the seed was committed)."""
    from vector_quantization import native

    temp = 0.7
    row, codes = distribution_inputs(K, D)
    x = row.expand(1, DIST_ROWS, D).contiguous().to(DEV)
    codes = codes.to(DEV)
    ind = _sample(x, codes, EUCLID, temp, _seed(*DIST_SEED))
    sims = native.similarities(x[:, :1].contiguous(), codes, metric=EUCLID)
    prob = (sims[0, 0].double() / temp).softmax(-1).cpu()
    freq = torch.bincount(ind.reshape(-1).cpu(), minlength=K).double() / DIST_ROWS
    sigma = (prob * (1 - prob) / DIST_ROWS).sqrt()
    assert bool(((freq - prob).abs() <= 5 * sigma + 1e-4).all()), (freq, prob)


# ------------------------------------------------------------------------------------------------ the modules
def _stochastic_codebook(K, D, temperature):
    from vector_quantization.codebook import Codebook
    from vector_quantization.codebooks import GumbelParams

    torch.manual_seed(1)
    return Codebook(dim=D, codebook_size=K, gumbel_params=GumbelParams(stochastic=True, temperature=temperature)).to(DEV).eval()


def test_codebook_forward_is_the_sweep_on_a_drawn_seed(monkeypatch):
    from vector_quantization import gumbel, native

    K, D = 100, 24
    mod = _stochastic_codebook(K, D, 0.9)
    x = torch.randn(3, 50, D, device=DEV)
    monkeypatch.delenv("VQ_NO_FUSED_SAMPLE", raising=False)
    torch.manual_seed(17)
    q, ind, _ = mod(x, return_similarities=False)
    torch.manual_seed(17)
    seed = gumbel.draw_seed(DEV)
    want = native.sample_codes(x.reshape(1, -1, D), mod.embeddings.detach(), metric=EUCLID, tau=1.0 / 0.9, seed=seed)
    assert torch.equal(ind.reshape(1, -1), want)
    assert torch.equal(q, mod.embeddings[0][ind])
    # the A/B switch: the chunked loop, other draws, still valid samples
    monkeypatch.setenv("VQ_NO_FUSED_SAMPLE", "1")
    torch.manual_seed(17)
    q2, ind2, _ = mod(x, return_similarities=False)
    assert ind2.shape == ind.shape and int(ind2.min()) >= 0 and int(ind2.max()) < K and not torch.equal(ind2, ind)
    assert torch.equal(q2, mod.embeddings[0][ind2])


def test_registered_op_equals_the_direct_call():
    """torch.ops.vq_mi355x.gumbel_sample: schema and fake-tensor agreement on a real launch, same indices as native.sample_codes."""
    from vector_quantization import native

    x, cb = _data(2, 130, 301, 64)
    seed = _seed(9, 10)
    packed = native.pack_codebooks(cb, DOT)
    for pk in (None, packed):
        torch.library.opcheck(torch.ops.vq_mi355x.gumbel_sample.default, (x, cb, pk, seed, DOT, 1.25),
                              test_utils=("test_schema", "test_faketensor"))
        got = torch.ops.vq_mi355x.gumbel_sample(x, cb, pk, seed, DOT, 1.25)
        assert torch.equal(got, native.sample_codes(x, cb, metric=DOT, tau=1.25, seed=seed))


def test_vector_quantize_and_residual_train_through_sampled_codes():
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams, GumbelParams

    params = CodebookParams(dim=8, codebook_size=32, gumbel_params=GumbelParams(stochastic=True))
    torch.manual_seed(0)
    mod = vq.VectorQuantize(dim=8, codebook_params=params).to(DEV).train()
    x = torch.randn(2, 50, 8, device=DEV, requires_grad=True)
    q, ind, loss = mod(x, freeze_codebook=True)
    codes = mod._codebook.embeddings[0][ind]
    torch.testing.assert_close(q, codes)  # straight-through value == the sampled code
    (q.sum() + loss.sum()).backward()
    torch.testing.assert_close(x.grad, 1.0 + 2.0 * (x.detach() - codes) / x.numel(), rtol=1e-5, atol=1e-6)
    assert len(torch.unique(ind)) > 8  # sampled, not one code

    rvq = vq.ResidualVQ(dim=8, num_quantizers=3, shared_codebook=True, codebook_params=params).to(DEV).train()
    x2 = torch.randn(2, 50, 8, device=DEV, requires_grad=True)
    out, idx, losses = rvq(x2, freeze_codebook=True)
    assert idx.shape == (2, 50, 3) and losses.shape == (1, 3)
    book = rvq.layers[0]._codebook.embeddings[0]
    picked = [book[idx[..., s]] for s in range(3)]
    torch.testing.assert_close(out, picked[0] + picked[1] + picked[2])
    (out.sum() + losses.sum()).backward()
    # every stage: straight-through (identity) + commitment 2 (r_s - c_s) / numel, r_s = x - the earlier stages' codes
    want = torch.full_like(x2, 3.0)
    r = x2.detach().clone()
    for s in range(3):
        want += 2.0 * (r - picked[s]) / x2.numel()
        r = r - picked[s]
    torch.testing.assert_close(x2.grad, want, rtol=1e-5, atol=1e-6)


def test_forward_allocates_nothing_of_m_by_k(monkeypatch):
    """One stochastic forward at M = 65536, K = 1024, D = 64: the peak allocation grows by less than one [M, K] fp32 matrix
    (256 MiB); the chunked loop behind VQ_NO_FUSED_SAMPLE=1 -- the path this replaces -- grows by more."""
    M, K, D = 65536, 1024, 64
    mod = _stochastic_codebook(K, D, 1.0)
    x = torch.randn(1, M, D, device=DEV)
    matrix = M * K * 4

    def growth():
        torch.manual_seed(0)
        mod(x[:, :256], return_similarities=False)  # (packs the codebook, warms the allocator's small pools)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ind = mod(x, return_similarities=False)[1]
        torch.cuda.synchronize()
        assert int(ind.min()) >= 0 and int(ind.max()) < K
        return torch.cuda.max_memory_allocated() - base

    monkeypatch.delenv("VQ_NO_FUSED_SAMPLE", raising=False)
    fused = growth()
    monkeypatch.setenv("VQ_NO_FUSED_SAMPLE", "1")
    chunked = growth()
    print(f"peak allocation growth: fused {fused / 2**20:.1f} MiB, chunked {chunked / 2**20:.1f} MiB, [M, K] fp32 {matrix / 2**20:.0f} MiB")
    assert fused < matrix < chunked
