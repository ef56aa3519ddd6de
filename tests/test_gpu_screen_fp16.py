"""GPU: the fp16 screened Dp = 256 sweep (vq_search_persist<256, 8, EUCLID, false, true>) over the data classes of its error
bound (tests/test_screen_fp16_bound_host.py has the bound itself), and the image its pack kernels write.

Every case compares idx and the quantized rows bit for bit, viewed as int32, among the default call, the call with a cached
image and the fp32 sweep (VQ_NO_SCREEN, read per call), and a sample of 200 rows, every constructed row included, with the
CPU oracle.  Classes with ineligible rows (beyond the limit xn s_x^2 = 2^30, NaN, inf) hold 64 of them, so the second pass
stays short; one case has every row ineligible.  The control block's words 4 and 5 (the list lengths of the last call) show
that those rows took the full search.

M = 131 072 is the smallest row count at which this kernel runs at K = 1024 on 256 CUs."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M0 = 131072
CTRL_BYTES = 16384      # kScrCtrlBytes
ROW_BYTES = 528         # kScrRowBytes
TILE_BYTES = 32 * ROW_BYTES + 128  # kScrTileBytes
N_BAD = 64


def _native():
    from vector_quantization import native

    native.load()
    return native


def _exponents(cb):
    hmax = float(cb.abs().max()) * 2.0
    lg = int(np.floor(np.log2(hmax)))
    return 13 - lg, 8 - lg


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


@functools.lru_cache(maxsize=None)
def _case(name, K, D):
    """-> x [1, M0, D], cb4 [1, 1, K, D], the constructed rows (indices), the number of rows that cannot be eligible."""
    cb = _randn((K, D), 100 + K + D)
    x = _randn((M0, D), 200 + K + D)
    special = torch.arange(0)
    n_bad = 0
    if name == "randn":
        pass
    elif name == "all_2^-20":
        cb, x = cb * 2.0 ** -20, x * 2.0 ** -20
    elif name == "codes_2^12":
        cb, x = cb * 2.0 ** 12, x * 2.0 ** 12
    elif name == "rows_30x":  # at the limit: 16 * 30 * s_x ~ 2^15, a good part of the rows is beyond it
        x = x * 30.0
    elif name == "rows_1/1000x":
        x = x * 1e-3
    elif name == "code_range_1e5":
        ramp = torch.logspace(0, -5, D, device=DEV)
        cb[3] *= ramp
        cb[K - 2] *= ramp.flip(0)
    elif name == "rows_straddle_2^-14":
        e_x = _exponents(cb)[1]
        x = x * (2.0 ** -14 / 2.0 ** e_x) * torch.exp2(4.0 * torch.rand((M0, D), generator=torch.Generator(device=DEV).manual_seed(5),
                                                                          device=DEV) - 2.0)
    elif name in ("limit", "nonfinite", "all_ineligible"):
        e_x = _exponents(cb)[1]
        xn = (x.double() ** 2).sum(1)
        to_limit = torch.sqrt(2.0 ** 30 / (xn * 4.0 ** e_x)).float()
        if name == "all_ineligible":
            x = x * (to_limit * 1.01)[:, None]
            n_bad = M0
            special = torch.randperm(M0, generator=torch.Generator().manual_seed(4))[:N_BAD]
        else:
            special = torch.randperm(M0, generator=torch.Generator().manual_seed(4))[:2 * N_BAD]
            above, below = special[:N_BAD].to(DEV), special[N_BAD:].to(DEV)
            x[below] *= (to_limit[below] * (1 - 1e-3))[:, None]
            if name == "limit":
                x[above] *= (to_limit[above] * (1 + 1e-3))[:, None]
            else:
                x[above[0::4], 3] = float("nan")
                x[above[1::4], D - 1] = float("inf")
                x[above[2::4], 0] = -float("inf")
                x[above[3::4]] *= 1e30
            n_bad = N_BAD
    else:
        raise KeyError(name)
    return x[None].contiguous(), cb[None, None].contiguous(), special, n_bad


def _three_ways(x, cb4):
    native = _native()
    H, _, K, D = cb4.shape
    packed = native.pack_codebooks(cb4, native.EUCLID)
    screen = native.pack_screen(packed, H, K, D, native.EUCLID)
    assert screen is not None
    a = native.quantize(x, cb4, packed=packed, want_best=False)
    b = native.quantize(x, cb4, packed=packed, screen=screen, want_best=False)
    torch.cuda.synchronize()
    counts = screen[-CTRL_BYTES:].view(torch.int32)[4:6].cpu().numpy().view(np.uint32)
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        c = native.quantize(x, cb4, packed=packed, want_best=False)
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    for r in (a, b):
        assert torch.equal(r["idx"], c["idx"])
        assert torch.equal(r["out"].view(torch.int32), c["out"].view(torch.int32))
    return a, (int(counts[0]), int(counts[1]))


CASES = [("randn", 1024, 256), ("randn", 3072, 132), ("all_2^-20", 1030, 132), ("codes_2^12", 3072, 200), ("rows_30x", 1024, 200),
         ("rows_1/1000x", 1030, 256), ("code_range_1e5", 1024, 132), ("rows_straddle_2^-14", 1030, 200), ("limit", 3072, 256),
         ("nonfinite", 1024, 256), ("all_ineligible", 1024, 256)]


@pytest.mark.parametrize("name,K,D", CASES, ids=[f"{n}-K{k}-D{d}" for n, k, d in CASES])
def test_classes_default_cached_fp32_oracle(oracle, name, K, D):
    x, cb4, special, n_bad = _case(name, K, D)
    res, (n_full, n_rescore) = _three_ways(x, cb4)
    print(f"{name} K={K} D={D}: {n_full} rows searched in full, {n_rescore} rescored, of {M0}")
    assert n_full + n_rescore <= M0
    if name == "all_ineligible":
        assert (n_full, n_rescore) == (M0, 0)
    elif name == "rows_30x":
        assert n_full > 0
    else:
        assert n_bad <= n_full <= n_bad + M0 // 4  # the rows that cannot be eligible, and few others
    rows = torch.cat([special, torch.randperm(M0, generator=torch.Generator().manual_seed(3))[:200 - special.numel()]])
    ri, _ = oracle.nearest(x[0, rows].cpu().numpy(), cb4[0, 0].cpu().numpy(), 0)
    np.testing.assert_array_equal(res["idx"][0, rows, 0].cpu().numpy(), ri)


@pytest.mark.parametrize("name,K,D", [("randn", 1030, 132), ("all_2^-20", 1024, 256), ("code_range_1e5", 3072, 200)])
def test_image_tail_and_code_halves(name, K, D):
    native = _native()
    _, cb4, _, _ = _case(name, K, D)
    packed = native.pack_codebooks(cb4, native.EUCLID)
    screen = native.pack_screen(packed, 1, K, D, native.EUCLID)
    torch.cuda.synchronize()
    img = screen[:-CTRL_BYTES].cpu().numpy()
    nt = (K + 31) // 32
    tail = img[nt * TILE_BYTES:nt * TILE_BYTES + 4 * (5 * nt + 2)]
    tf, ti = tail.view(np.float32), tail.view(np.int32)
    mcn, ec, l1, flag, absmax = (tf[i * nt:(i + 1) * nt] for i in range(5))
    e_c, e_x = int(ti[5 * nt]), int(ti[5 * nt + 1])
    cb = cb4[0, 0].cpu().numpy()
    c64 = cb.astype(np.float64)
    assert 2.0 ** 13 <= np.abs(2.0 * c64).max() * 2.0 ** e_c < 2.0 ** 14
    assert 2.0 ** 7 <= np.abs(c64).max() * 2.0 ** e_x < 2.0 ** 8
    assert (tail.view(np.uint32)[3 * nt:4 * nt] == 0).all()
    # the model of the pack kernel: plain float16 cast of s_c * (-2c), values below 2^-14 stored as 0
    v = np.zeros((nt * 32, 256), np.float32)
    v[:K, :D] = (np.float32(-2.0) * cb) * np.float32(2.0 ** e_c)
    ct = v.astype(np.float16)
    ct[np.abs(ct.astype(np.float64)) < 2.0 ** -14] = 0
    diff = v.astype(np.float64) - ct.astype(np.float64)
    want_ec = np.sqrt((diff * diff).sum(1)).reshape(nt, 32).max(1)
    want_l1 = np.abs(ct.astype(np.float64)).sum(1).reshape(nt, 32).max(1)
    want_abs = np.abs(v.astype(np.float64) / 2.0 ** e_c).reshape(nt, -1).max(1)
    assert (ec >= want_ec).all() and (ec <= 1.002 * want_ec).all(), (ec / want_ec).min()
    assert (l1 >= want_l1).all() and (l1 <= 1.002 * want_l1).all(), (l1 / want_l1).min()
    np.testing.assert_array_equal(absmax.astype(np.float64), want_abs)
    cn = np.zeros(nt * 32)
    cn[:K] = (c64 * c64).sum(1)
    np.testing.assert_allclose(mcn, cn.reshape(nt, 32).max(1), rtol=1e-5)
    # the code halves of the first, a middle and the last tile (with its padding rows), and the tiles' scaled |c|^2
    for t in (0, nt // 2, nt - 1):
        tile = img[t * TILE_BYTES:(t + 1) * TILE_BYTES]
        rows = tile[:32 * ROW_BYTES].reshape(32, ROW_BYTES)
        got = rows[:, :512].copy().view(np.float16)
        np.testing.assert_array_equal(got.view(np.uint16), ct[32 * t:32 * t + 32].view(np.uint16))
        assert (rows[:, 512:] == 0).all()
        cs = tile[32 * ROW_BYTES:].view(np.float32)
        real = np.arange(32 * t, 32 * t + 32) < K
        np.testing.assert_allclose(cs[real], cn[32 * t:32 * t + 32][real] * 2.0 ** (e_c + e_x), rtol=1e-5)
        assert np.isinf(cs[~real]).all()
