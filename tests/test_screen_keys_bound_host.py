"""Host only: the error bound of the screened Dp = 256 sweep with TAGGED KEYS (csrc/vq_search_persist.inc, "The bound", item
(6); csrc/vq_scr_keys.h), on the numpy model of tests/test_screen_fp16_bound_host.py extended by the tag.

The model is that file's (copied here: c' = -2c, ct = fp16(s_c c') with values below 2^-14 stored as 0, X = s_x x, xh = fp16(X),
xl = fp16(X - xh), exact products, 513 float32 additions in natural, reversed and one random order, fp16 operands below
2^-14 kept and flushed), followed by what the kernel does to the accumulator: the 4 low bits of the float32 pattern are
replaced by the accumulator register's number r of the code (code k sits at offset o = k % 32 of its sub-tile, lane half
(o >> 2) & 1, register r = (o & 3) + 4 (o >> 3)), and, as the worst cases whatever the layout, by 0 and by 15.
S = key / (s_c s_x), E = |c|^2 - 2 x.c in fp64, and

    |S - E| <= 1.0001 (E_c / s_c) nx + 4.81e-5 L + 3.25e-5 nc^2 + 1.21e-7 xn + (2^-13 l1 + 2^-116) / sg + 2^-140 =: delta_0

with L = 2 nx nc, nx = sqrt(xn), nc = sqrt(max cn), E_c = max_k |s_c c'_k - ct_k|_2, l1 = max_k sum_i |ct_ki|, sg = s_c s_x."""
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


def delta0(x, img, tagged=True):
    """The proven bound for every row of x, in fp64 (the formula of the kernel's comment; tagged=False: before the keys)."""
    xn = chain32(x).astype(np.float64)
    mcn = float(img["cn"].max())
    nx, nc = np.sqrt(xn), np.sqrt(mcn)
    s_c, sg = 2.0 ** img["e_c"], 2.0 ** (img["e_c"] + img["e_x"])
    cl, cc = (4.81e-5, 3.25e-5) if tagged else (4.63e-5, 3.07e-5)
    return (1.0001 * (img["E_c"] / s_c) * nx + cl * (2.0 * nx * nc) + cc * mcn + 1.21e-7 * xn
            + (2.0 ** -13 * img["l1"] + 2.0 ** -116) / sg + 2.0 ** -140)


def accumulators(x, img, flush, order):
    """[M, K] float32: the accumulators of rows x against the image, 513 float32 additions in `order` (units of s_c s_x)."""
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
    return acc


def register_of(k):
    o = np.asarray(k) % 32
    return (o & 3) + 4 * (o >> 3)


def keys(acc, tag):
    """The accumulators with their 4 low bits replaced: tag = "r" (the code's register), or a number for every code."""
    r = register_of(np.arange(acc.shape[1])) if tag == "r" else np.full(acc.shape[1], tag)
    bits = (np.ascontiguousarray(acc).view(np.uint32) & np.uint32(0xFFFFFFF0)) | r.astype(np.uint32)[None, :]
    return bits.view(np.float32)


def exact(x, cb):
    c = cb.astype(np.float64)
    return (c * c).sum(1)[None, :] - 2.0 * x.astype(np.float64) @ c.T


ORDERS = {"natural": np.arange(2 * D + 1), "reversed": np.arange(2 * D + 1)[::-1],
          "random": np.random.default_rng(5).permutation(2 * D + 1)}
TAGS = ("r", 0, 15)


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
def test_keys_within_delta0(name):
    cb, x = _classes()[name]
    img = pack(cb)
    ok = eligible(x, img)
    assert ok.all() if name != "rows_30x" else ok.sum() >= M // 2, ok
    x = x[ok]
    d0 = delta0(x, img)
    E = exact(x, cb)
    sg = 2.0 ** (img["e_c"] + img["e_x"])
    worst = 0.0
    for flush in (False, True):
        for oname, order in ORDERS.items():
            acc = accumulators(x, img, flush, order)
            for tag in TAGS:
                key = keys(acc, tag)
                assert (np.abs(key.view(np.int32).astype(np.int64) - acc.view(np.int32).astype(np.int64)) <= 15).all()
                err = np.abs(key.astype(np.float64) / sg - E)
                ratio = float((err / d0[:, None]).max())
                worst = max(worst, ratio)
                assert (err <= d0[:, None]).all(), (name, flush, oname, tag, ratio)
    print(f"{name}: largest |key / sg - E| / delta_0 = {worst:.3f}")


def test_zero_accumulator_gives_a_subnormal_key_inside_the_absolute_term():
    """A zero code against any row: the accumulator is +0 exactly, the key r * 2^-149, and key / sg stays inside the
    bound's absolute term whatever the scales (sg >= 2^-124)."""
    acc = np.zeros((1, 32), np.float32)
    key = keys(acc, "r")
    assert (key.view(np.uint32)[0] == register_of(np.arange(32))).all()
    for e in (-124, -20, 0, 40, 124):
        assert (key.astype(np.float64) / 2.0 ** e <= 2.0 ** -116 / 2.0 ** e + 2.0 ** -140).all()


def test_tagged_delta_against_the_bf16_pair_formula_on_the_list_tests_data():
    """tests/test_gpu_screened_rescore.py, test_gpu_screened_resolve.py and test_gpu_screen_cache.py steer rows onto the two
    lists by margins of 0.1, 3 and 4 delta of the EARLIER formula (2.5e-4 L + 1e-4 nc^2 + 3e-7 xn) on codes randn * 8 and rows
    a code + 0.5 randn.  The kernel's delta = 1.1 delta_0 must stay within 1.25 x of that, the margin those tests were built
    for (and above 0.55 x), with the keys' share in delta_0; and the keys add at most 6 % to delta."""
    r = np.random.default_rng(21)
    cb = (r.standard_normal((1024, D)) * 8).astype(np.float32)
    x = cb[r.integers(0, 1024, 512)] + (0.5 * r.standard_normal((512, D))).astype(np.float32)
    img = pack(cb)
    new = 1.1 * delta0(x, img)
    before = 1.1 * delta0(x, img, tagged=False)
    xn, mcn = chain32(x).astype(np.float64), float(img["cn"].max())
    old = 2.5e-4 * 2.0 * np.sqrt(xn) * np.sqrt(mcn) + 1e-4 * mcn + 3e-7 * xn
    ratio = new / old
    print(f"delta / bf16-form delta: min {ratio.min():.4f} median {np.median(ratio):.4f} max {ratio.max():.4f}; "
          f"delta / delta before the keys: max {(new / before).max():.4f}")
    assert ratio.max() <= 1.25 and ratio.min() >= 0.55
    assert (new / before).max() <= 3.25 / 3.07  # the largest ratio of two coefficients
