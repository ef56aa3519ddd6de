"""GPU: the screened Dp = 256 sweep (vq_search_persist<256, 8, EUCLID, false, true>): a bf16x3 screen with a proven error
bound decides the rows whose winner it certifies, the exact fp32 rule decides the rest.  Every row of every call must equal
the fp32 sweep (VQ_NO_SCREEN, read per call) bit for bit -- indices and quantized rows -- and a row sample the CPU oracle.
Data classes: separated, exact grid, duplicated grid (forced ties: every row uncertain), small-scale uniform (near-tie heavy),
rows equal to a code (distance clamps to 0), codes one ulp apart, magnitudes near the eligibility limits, NaN / inf rows and
codes, ragged row counts, strided multi-head views."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 1024
D = 256


def _native():
    from vector_quantization import native

    native.load()
    return native


def _both(x, cb):
    """(screened call, fp32-sweep call) of the same plain eval search; no distances requested (the screen's calls)."""
    native = _native()
    a = native.quantize(x, cb, metric=0, want_best=False)
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        b = native.quantize(x, cb, metric=0, want_best=False)
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    torch.cuda.synchronize()
    return a, b


def _check(x, cb, oracle, n_sample=200):
    a, b = _both(x, cb)
    assert torch.equal(a["idx"], b["idx"])
    assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32))
    H, M = x.shape[0], x.shape[1]
    rows = torch.cat([torch.randperm(M, generator=torch.Generator().manual_seed(3))[:n_sample], torch.arange(max(0, M - 20), M)])
    for h in range(H):
        ri, _ = oracle.nearest(x[h, rows].cpu().numpy(), cb[h, 0].cpu().numpy(), 0)
        np.testing.assert_array_equal(a["idx"][h, rows, 0].cpu().numpy(), ri)
    return a


def _data(kind, M, seed, H=1, k=K, d=D):
    g = torch.Generator().manual_seed(seed)
    if kind == "S":      # separated
        cb = torch.randn((H, 1, k, d), generator=g)
        x = torch.randn((H, M, d), generator=g)
    elif kind == "G":    # exact grid: small integers, many exact ties between distances
        cb = torch.randint(-3, 4, (H, 1, k, d), generator=g).float()
        x = torch.randint(-3, 4, (H, M, d), generator=g).float()
    elif kind == "Gdup":  # duplicated grid: every code twice -> every row has an exact tie (the lower index must win)
        half = torch.randint(-2, 3, (H, 1, k // 2, d), generator=g).float()
        cb = torch.cat([half, half], dim=2)[:, :, torch.randperm(k, generator=g)]
        x = torch.randint(-2, 3, (H, M, d), generator=g).float()
    elif kind == "R":    # kaiming-uniform-like codes, rows of the same scale: near ties everywhere
        bound = (6.0 / d) ** 0.5
        cb = (torch.rand((H, 1, k, d), generator=g) * 2 - 1) * bound
        x = (torch.rand((H, M, d), generator=g) * 2 - 1) * bound
    else:
        raise ValueError(kind)
    return x.to(DEV), cb.to(DEV)


@pytest.mark.parametrize("kind", ["S", "G", "Gdup", "R"])
def test_screened_equals_fp32_sweep(oracle, kind):
    x, cb = _data(kind, 140001, 7)
    _check(x, cb, oracle)


@pytest.mark.parametrize("M,k,d", [(131072 + 77, 1000, 256), (200003, 2048, 252), (150000, 3000, 256)])
def test_screened_ragged_shapes(oracle, M, k, d):
    x, cb = _data("S", M, M, k=k, d=d)
    _check(x, cb, oracle)


def test_rows_equal_to_a_code_and_codes_one_ulp_apart(oracle):
    x, cb = _data("S", 140000, 11)
    c = cb[0, 0]
    # code 5 and code 700 differ in one ulp of one element; code 9 == code 600 exactly
    c[700] = c[5]
    c[700, 17] = torch.nextafter(c[5, 17], torch.tensor(float("inf"), device=DEV))
    c[600] = c[9]
    x[0, ::3] = c[torch.arange(0, x.shape[1], 3, device=DEV) % K]      # rows equal to a code: distance 0 (clamped)
    x[0, 1::7] = c[5]
    x[0, 2::11] = c[700]
    x[0, 4::13] = c[9]
    _check(x, cb, oracle, n_sample=400)


@pytest.mark.parametrize("scale", [2.0 ** 45, 2.0 ** 49, 2.0 ** -40, 2.0 ** -60])
def test_magnitudes_near_the_eligibility_limits(oracle, scale):
    x, cb = _data("S", 131072 + 5, 13)
    _check(x * scale, cb * scale, oracle)
    _check(x * scale, cb, oracle)


def test_non_finite_rows_and_codes(oracle):
    x, cb = _data("S", 140000, 17)
    x[0, 3, 7] = float("nan")
    x[0, 1000, 0] = float("inf")
    x[0, 2000, 255] = -float("inf")
    _check(x, cb, oracle)
    cb2 = cb.clone()
    cb2[0, 0, 321, 5] = float("inf")
    _check(x[:, :131073], cb2, oracle, n_sample=60)
    cb2[0, 0, 100, 9] = float("nan")
    _check(x[:, :131073], cb2, oracle, n_sample=60)


def test_screened_strided_head_views():
    """The module's layout: x [rows, heads * d] searched as [heads, rows, d] views, out / idx strided; both sweeps agree."""
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    torch.manual_seed(0)
    mod = vq.VectorQuantize(dim=512, codebook_params=CodebookParams(dim=256, codebook_size=1024), heads=2, codebook_dim=256,
                            separate_codebook_per_head=True).to(DEV).eval()
    x = torch.randn((140, 1024, 512), generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        q, idx, _ = mod(x)
        os.environ["VQ_NO_SCREEN"] = "1"
        try:
            q2, idx2, _ = mod(x)
        finally:
            os.environ.pop("VQ_NO_SCREEN", None)
    assert torch.equal(idx, idx2)
    assert torch.equal(q, q2)


def test_the_screened_kernel_is_the_one_that_runs():
    """cfg2's call (plain eval search, no distances) must run the screened sweep; VQ_NO_SCREEN the fp32 one."""
    from torch.profiler import ProfilerActivity, profile

    native = _native()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, 262144, 256), generator=g).to(DEV)
    cb = torch.randn((1, 1, 1024, 256), generator=g).to(DEV)
    packed = native.pack_codebooks(cb, 0)

    def names():
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            native.quantize(x, cb, packed=packed, want_best=False)
            torch.cuda.synchronize()
        return [ev.name for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and "vq_" in ev.name]

    plain = names()
    if not plain:
        pytest.skip("torch.profiler reported no device activity on this build")
    assert any("vq_search_persist" in n and "true>" in n for n in plain), plain
    assert any("vq_pack_scr_kernel" in n for n in plain), plain
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        off = names()
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    assert any("vq_search_persist" in n for n in off) and not any("true>" in n for n in off), off
