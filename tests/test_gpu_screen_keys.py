"""GPU: the tagged keys of the screened Dp = 256 sweep (vq_search_persist<256, 8, EUCLID, false, true>; csrc/vq_scr_keys.h has
the tracker, tests/test_scr_keys_host.py checks it on the host).  The sweep writes the accumulator register's number into
the 4 low mantissa bits of every screened value and decodes the codes of a lane's two lowest keys once, after the sweep.
What that could break, one group of cases each:

  * padding codes (K not a multiple of 32): their +inf would become a NaN key, and v_med3_f32 answers min3 for a NaN, which
    would send every row to the full-search list -- right results, slowly.  The list lengths must stay at those of the
    build before the keys (profiles/cfg2_tagged_keys.md, "Padding codes");
  * a zero code that wins: its accumulator is +0 exactly, the key the subnormal r * 2^-149, and the row is CERTAIN, so its
    index comes from the decoded key and from nothing else (both lists must be empty);
  * equal keys: identical code rows at the same register in two sub-tiles (equal keys), at two registers of one sub-tile
    (keys that differ by the tag only), and three of them in one lane half (more candidates than a lane tracks: full search).

Every case compares idx and the quantized rows bit for bit, viewed as int32, among the default call, the call with a cached
image, the call with all epilogues at one place (VQ_NO_STAGGER) and the fp32 sweep (VQ_NO_SCREEN; both read per call), and a
sample of 200 rows with the CPU oracle.  The control block's words 4 and 5 hold the list lengths of the last call.

M = 131 072 is the smallest row count at which this kernel runs on 256 CUs."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M0 = 131072
CTRL_BYTES = 16384  # kScrCtrlBytes

# (rows searched in full, rows rescored) of the build before the keys on _padding_case's data, measured once on an MI355X
# (profiles/cfg2_tagged_keys.md, "Padding codes")
PARENT_COUNTS = {(1030, 132): (22, 3845), (3067, 200): (46, 5016)}


def _native():
    from vector_quantization import native

    native.load()
    return native


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _four_ways(x, cb4):
    """x [1, M, D], cb4 [1, 1, K, D] on the GPU -> the default call's result and the (full-search, rescore) list lengths."""
    native = _native()
    H, _, K, D = cb4.shape
    packed = native.pack_codebooks(cb4, native.EUCLID)
    screen = native.pack_screen(packed, H, K, D, native.EUCLID)
    assert screen is not None
    a = native.quantize(x, cb4, packed=packed, want_best=False)
    b = native.quantize(x, cb4, packed=packed, screen=screen, want_best=False)
    torch.cuda.synchronize()
    counts = screen[-CTRL_BYTES:].view(torch.int32)[4:6].cpu().numpy().view(np.uint32)
    others = []
    for var in ("VQ_NO_STAGGER", "VQ_NO_SCREEN"):
        os.environ[var] = "1"
        try:
            others.append(native.quantize(x, cb4, packed=packed, want_best=False))
        finally:
            os.environ.pop(var, None)
    fp32 = others[1]
    for r in (a, b, others[0]):
        assert torch.equal(r["idx"], fp32["idx"])
        assert torch.equal(r["out"].view(torch.int32), fp32["out"].view(torch.int32))
    assert int(a["idx"].min()) >= 0 and int(a["idx"].max()) < K  # every element a code: no candidate word survives
    return a, (int(counts[0]), int(counts[1]))


def _oracle_sample(oracle, res, x, cb4):
    rows = torch.cat([torch.randperm(M0, generator=torch.Generator().manual_seed(3))[:180], torch.arange(M0 - 20, M0)])
    ri, _ = oracle.nearest(x[0, rows].cpu().numpy(), cb4[0, 0].cpu().numpy(), 0)
    np.testing.assert_array_equal(res["idx"][0, rows, 0].cpu().numpy(), ri)


def _padding_case(K, D):
    return _randn((M0, D), 300 + K + D)[None].to(DEV), _randn((K, D), 400 + K + D)[None, None].to(DEV)


@pytest.mark.parametrize("K,D", [(1030, 132), (3072 - 5, 200)])
def test_padding_codes_keep_the_lists_short(oracle, K, D):
    x, cb4 = _padding_case(K, D)
    res, (n_full, n_rescore) = _four_ways(x, cb4)
    p_full, p_rescore = PARENT_COUNTS[(K, D)]
    print(f"padding K={K} D={D}: {n_full} rows searched in full (before the keys {p_full}), {n_rescore} rescored ({p_rescore}), of {M0}")
    # delta grows by <= 2 %: the rescore count is linear in delta, the full-search count quadratic (and a small count with
    # Poisson scatter).  A NaN key would put all M0 rows on the full-search list.
    assert n_rescore <= 1.10 * p_rescore
    assert n_full <= 1.5 * p_full
    _oracle_sample(oracle, res, x, cb4)


ZERO_AT = [(5, 1, 1), (32 * 11 + 18, 0, 10), (1023, 1, 15)]  # (code, its lane half h, its accumulator register r)


def _zero_case(pos):
    """Codes randn * 8 with an all-zero code at `pos`, rows 0.3 randn: |x|^2 ~ 23 > 2 delta ~ 1.5 and every other code is
    thousands further than the zero code (checked in fp64 on the host for this recipe, every row of all three cases:
    profiles/cfg2_tagged_keys.md, "Zero code")."""
    cb = _randn((1024, 256), 500) * 8.0
    cb[pos] = 0.0
    x = _randn((M0, 256), 501) * 0.3
    return x[None].to(DEV), cb[None, None].to(DEV)


@pytest.mark.parametrize("pos,h,r", ZERO_AT)
def test_zero_code_wins_by_its_decoded_key(oracle, pos, h, r):
    assert pos % 32 == 4 * h + (r & 3) + 8 * (r >> 2)  # the accumulator layout of run_sub_scr
    x, cb4 = _zero_case(pos)
    res, (n_full, n_rescore) = _four_ways(x, cb4)
    print(f"zero code at {pos}: {n_full} rows searched in full, {n_rescore} rescored, of {M0}")
    assert bool((res["idx"] == pos).all())
    assert n_full + n_rescore <= M0 // 1000  # the decode produced the indices, not the second pass
    _oracle_sample(oracle, res, x, cb4)


def _equal_case(kind):
    """Codes randn * 8 (unrelated codes are thousands of delta apart), some of them exact copies of others; rows are a code
    + 0.5 randn, so the copies of the nearest code tie exactly -- 0 is within 0.1 delta -- and the lowest index must win.
    -> x, cb, the expected index of every row, the rows whose nearest code has copies."""
    K, D = 1024, 256
    cb = _randn((K, D), 600) * 8.0
    pick = torch.randint(0, K, (M0,), generator=torch.Generator().manual_seed(601))
    copied = torch.ones(M0, dtype=torch.bool)
    if kind == "same_r_two_subtiles":      # code i and i + 512: the same lane half and register, sub-tiles u and u + 16
        cb[512:] = cb[:512]
        want = pick % 512
    elif kind == "two_r_one_subtile":      # code i and i ^ 1: one lane half, registers r and r ^ 1 of one sub-tile
        cb[1::2] = cb[0::2]
        want = pick & ~1
    elif kind == "three_same_r":           # code i, i + 320, i + 640: one register in three sub-tiles; the last 64 codes unrelated
        cb[320:640] = cb[:320]
        cb[640:960] = cb[:320]
        copied = pick < 960
        want = torch.where(copied, pick % 320, pick)
    elif kind == "three_one_half":         # codes 8 g, 8 g + 1, 8 g + 2: three registers of one lane half; the other five unrelated
        cb[1::8] = cb[0::8]
        cb[2::8] = cb[0::8]
        copied = pick % 8 < 3
        want = torch.where(copied, pick - pick % 8, pick)
    else:
        raise KeyError(kind)
    x = cb[pick] + 0.5 * _randn((M0, D), 602)
    return x[None].to(DEV), cb[None, None].to(DEV), want, int(copied.sum())


@pytest.mark.parametrize("kind", ["same_r_two_subtiles", "two_r_one_subtile", "three_same_r", "three_one_half"])
def test_equal_keys_lowest_index_wins(oracle, kind):
    x, cb4, want, n_copied = _equal_case(kind)
    res, (n_full, n_rescore) = _four_ways(x, cb4)
    print(f"{kind}: {n_full} rows searched in full, {n_rescore} rescored, of {M0} ({n_copied} next to a copied code)")
    assert torch.equal(res["idx"][0, :, 0].cpu(), want)
    # The copies' keys are equal or differ by the tag only (<= 15 ulp, far below 2 delta): such a row is never certain.  Every
    # other code is thousands of delta further, so two copies are the lane's only candidates (both handed to the second
    # pass: rescored) and three make b3 <= thr (searched in full); rows next to an unrelated code are certain.
    if kind.startswith("three"):
        assert (n_full, n_rescore) == (n_copied, 0) and 0 < n_copied < M0
    else:
        assert (n_full, n_rescore) == (0, M0)
    _oracle_sample(oracle, res, x, cb4)
