"""Host only: the error bound of the fp16 screened Dp = 256 sweep (csrc/vq_search_persist.inc, "The bound"), checked on a
numpy model of the screen against the exact value in fp64.

The model is the kernel's arithmetic: c' = -2c, ct = fp16(s_c c') with values below 2^-14 stored as 0, X = s_x x, xh = fp16(X),
xl = fp16(X - xh) (numpy's float16 casts round to nearest), products exact (float64 holds 22-bit products exactly), 513 terms
-- |c|^2 s_c s_x and the 512 products -- added in float32 in natural, reversed and one random order, with fp16 operands below
2^-14 both kept and flushed to 0; S = the sum / (s_c s_x).  E = |c|^2 - 2 x.c in fp64.

delta_0 is written once, in `delta0`, and quotes the kernel's comment:

    |S - E| <= 1.0001 (E_c / s_c) nx + 4.63e-5 L + 3.07e-5 nc^2 + 1.21e-7 xn + (2^-13 l1 + 2^-116) / sg + 2^-140 =: delta_0

with L = 2 nx nc, nx = sqrt(xn), nc = sqrt(max cn), E_c = max_k |s_c c'_k - ct_k|_2, l1 = max_k sum_i |ct_ki|, sg = s_c s_x.
A row is eligible when xn s_x^2 <= 2^30 (and finite)."""
from __future__ import annotations

import numpy as np
import pytest

D, K, M = 256, 40, 24
F16_MIN_NORMAL = 2.0 ** -14


def chain32(v):
    """d-ordered float32 sum of squares along the last axis (the packed image's |c|^2 and the prologue's |x|^2)."""
    acc = np.zeros(v.shape[:-1], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(v.shape[-1]):
            acc = (v[..., d] * v[..., d] + acc).astype(np.float32)
    return acc


def exponents(cb):
    """(e_c, e_x): max |2c| 2^e_c in [2^13, 2^14), max |c_i| 2^e_x in [2^7, 2^8)."""
    hmax = float(np.abs(2.0 * cb.astype(np.float64)).max())
    if hmax == 0.0:
        return 0, 0
    lg = int(np.floor(np.log2(hmax)))
    return 13 - lg, 8 - lg


def pack(cb):
    """The image of a codebook [K, D] float32: ct (float16, flushed), cn (float32 chain), e_c, e_x, E_c, l1 (exact, float64)."""
    e_c, e_x = exponents(cb)
    v = (np.float32(-2.0) * cb).astype(np.float32) * np.float32(2.0 ** e_c)
    ct = v.astype(np.float16)
    ct[np.abs(ct.astype(np.float64)) < F16_MIN_NORMAL] = 0
    diff = v.astype(np.float64) - ct.astype(np.float64)
    return dict(ct=ct, cn=chain32(cb), e_c=e_c, e_x=e_x, E_c=float(np.sqrt((diff * diff).sum(1)).max()),
                l1=float(np.abs(ct.astype(np.float64)).sum(1).max()))


def split_rows(x, e_x):
    with np.errstate(over="ignore", invalid="ignore"):
        X = (x * np.float32(2.0 ** e_x)).astype(np.float32)
        xh = X.astype(np.float16)
        xl = (X - xh.astype(np.float32)).astype(np.float16)
    return xh, xl


def eligible(x, img):
    xn = chain32(x).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return xn * 4.0 ** img["e_x"] <= 2.0 ** 30  # (False for NaN and inf)


def delta0(x, img):
    """The proven bound for every row of x, in fp64 (the formula of the kernel's comment)."""
    xn = chain32(x).astype(np.float64)
    mcn = float(img["cn"].max())
    nx, nc = np.sqrt(xn), np.sqrt(mcn)
    s_c, sg = 2.0 ** img["e_c"], 2.0 ** (img["e_c"] + img["e_x"])
    return (1.0001 * (img["E_c"] / s_c) * nx + 4.63e-5 * (2.0 * nx * nc) + 3.07e-5 * mcn + 1.21e-7 * xn
            + (2.0 ** -13 * img["l1"] + 2.0 ** -116) / sg + 2.0 ** -140)


def screen(x, img, flush, order):
    """S [M, K]: the screened values of rows x against the image, 513 float32 additions in `order`."""
    xh, xl = split_rows(x, img["e_x"])
    xh, xl = xh.astype(np.float64), xl.astype(np.float64)
    if flush:
        xh = np.where(np.abs(xh) < F16_MIN_NORMAL, 0.0, xh)
        xl = np.where(np.abs(xl) < F16_MIN_NORMAL, 0.0, xl)
    ct = img["ct"].astype(np.float64)
    sg = 2.0 ** (img["e_c"] + img["e_x"])
    terms = np.empty((x.shape[0], ct.shape[0], 2 * D + 1), np.float32)
    terms[:, :, 0] = (img["cn"].astype(np.float64) * sg)[None, :]
    terms[:, :, 1:D + 1] = xh[:, None, :] * ct[None, :, :]   # exact: 22 significant bits
    terms[:, :, D + 1:] = xl[:, None, :] * ct[None, :, :]
    acc = np.zeros(terms.shape[:2], np.float32)
    for j in order:
        acc = (acc + terms[:, :, j]).astype(np.float32)
    return acc.astype(np.float64) / sg


def exact(x, cb):
    c = cb.astype(np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * x.astype(np.float64) @ c.T


ORDERS = {"natural": np.arange(2 * D + 1), "reversed": np.arange(2 * D + 1)[::-1],
          "random": np.random.default_rng(5).permutation(2 * D + 1)}


def _classes():
    r = np.random.default_rng(20)
    randn = lambda *s: r.standard_normal(s).astype(np.float32)
    out = {}
    cb = randn(K, D)
    out["randn"] = (cb, randn(M, D))
    out["near_codes_scale8"] = (cb * 8, cb[r.integers(0, K, M)] * 8 + np.float32(0.5) * randn(M, D))
    out["all_2^-20"] = (cb * np.float32(2.0 ** -20), randn(M, D) * np.float32(2.0 ** -20))
    out["codes_2^12"] = (cb * np.float32(2.0 ** 12), randn(M, D) * np.float32(2.0 ** 12))
    out["rows_30x"] = (cb, randn(M, D) * 30)
    out["rows_1/1000x"] = (cb, randn(M, D) * np.float32(1e-3))
    wide = cb.copy()
    wide[3] *= np.logspace(0, -5, D).astype(np.float32)   # 10^5 of dynamic range across the dims of one code
    wide[4] *= np.logspace(-5, 0, D).astype(np.float32)
    out["code_range_1e5"] = (wide, randn(M, D))
    e_x = exponents(cb)[1]
    # rows whose scaled elements lie within a factor 4 of fp16's smallest normal value, on both sides
    tiny = randn(M, D) * np.float32(2.0 ** -14 / 2.0 ** e_x) * (2.0 ** r.uniform(-2, 2, (M, D))).astype(np.float32)
    out["rows_straddle_2^-14"] = (cb, tiny)
    uni = (r.uniform(-1, 1, (K, D)) * 0.01).astype(np.float32)
    out["small_uniform"] = (uni, uni[r.integers(0, K, M)] + np.float32(0.002) * randn(M, D))
    return out


@pytest.mark.parametrize("name", list(_classes()))
def test_screen_within_delta0(name):
    cb, x = _classes()[name]
    img = pack(cb)
    assert 2.0 ** 13 <= np.abs(2.0 * cb.astype(np.float64)).max() * 2.0 ** img["e_c"] < 2.0 ** 14
    assert 2.0 ** 7 <= np.abs(cb.astype(np.float64)).max() * 2.0 ** img["e_x"] < 2.0 ** 8
    ok = eligible(x, img)
    # (rows 30 x the codes' scale sit at the limit: |X|_2 = 16 * 30 * s_x ~ 2^15; the bound is claimed for eligible rows only)
    assert ok.all() if name != "rows_30x" else ok.sum() >= M // 2, ok
    x = x[ok]
    d0 = delta0(x, img)
    E = exact(x, cb)
    worst = 0.0
    for flush in (False, True):
        for oname, order in ORDERS.items():
            err = np.abs(screen(x, img, flush, order) - E)
            ratio = float((err / d0[:, None]).max())
            worst = max(worst, ratio)
            assert (err <= d0[:, None]).all(), (name, flush, oname, ratio)
    print(f"{name}: largest |S - E| / delta_0 = {worst:.3f}")


def test_rows_around_the_eligibility_limit():
    """A row just below the limit xn s_x^2 = 2^30 is eligible, finite in fp16 and inside the bound; a row just above it, and
    every NaN / inf row, is ineligible."""
    cb, x = _classes()["randn"]
    img = pack(cb)
    x = x[:8].copy()
    xn = chain32(x).astype(np.float64)
    limit = np.sqrt(2.0 ** 30 / (xn * 4.0 ** img["e_x"]))
    below = (x * (limit * (1 - 1e-3))[:, None]).astype(np.float32)
    above = (x * (limit * (1 + 1e-3))[:, None]).astype(np.float32)
    # one element carrying almost the whole norm: the largest scaled element an eligible row can hold
    spike = np.zeros((1, D), np.float32)
    spike[0, 7] = np.float32(2.0 ** 15 / 2.0 ** img["e_x"] * (1 - 1e-3))
    below = np.concatenate([below, spike])
    assert eligible(below, img).all() and not eligible(above, img).any()
    bad = x.copy()
    bad[0, 3], bad[1, 0], bad[2, D - 1] = np.nan, np.inf, -np.inf
    bad[3] *= np.float32(1e30)
    assert not eligible(bad[:4], img).any()
    xh, _ = split_rows(below, img["e_x"])
    assert np.isfinite(xh.astype(np.float64)).all()
    d0 = delta0(below, img)
    E = exact(below, cb)
    for flush in (False, True):
        for oname, order in ORDERS.items():
            err = np.abs(screen(below, img, flush, order) - E)
            assert (err <= d0[:, None]).all(), (flush, oname, float((err / d0[:, None]).max()))


def test_new_delta_against_the_bf16_pair_formula_on_the_list_tests_data():
    """tests/test_gpu_screened_rescore.py, test_gpu_screened_resolve.py and test_gpu_screen_cache.py steer rows onto the two
    lists by margins of 0.1, 3 and 4 delta of the EARLIER formula (2.5e-4 L + 1e-4 nc^2 + 3e-7 xn) on codes randn * 8 and rows
    a code + 0.5 randn.  The kernel's delta = 1.1 delta_0 must stay within 1.25 x of that (and above 0.55 x: a pair 0.1 old
    delta apart is then uncertain whatever the screen's error, 0.1 old + 2 delta_0 <= 2 delta)."""
    r = np.random.default_rng(21)
    cb = (r.standard_normal((1024, D)) * 8).astype(np.float32)
    x = cb[r.integers(0, 1024, 512)] + (0.5 * r.standard_normal((512, D))).astype(np.float32)
    img = pack(cb)
    new = 1.1 * delta0(x, img)
    xn, mcn = chain32(x).astype(np.float64), float(img["cn"].max())
    old = 2.5e-4 * 2.0 * np.sqrt(xn) * np.sqrt(mcn) + 1e-4 * mcn + 3e-7 * xn
    ratio = new / old
    print(f"delta / old delta: min {ratio.min():.4f} median {np.median(ratio):.4f} max {ratio.max():.4f}")
    assert ratio.max() <= 1.25 and ratio.min() >= 0.55
