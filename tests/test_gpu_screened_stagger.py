"""GPU: the staggered epilogue of the screened Dp = 256 sweep (vq_search_persist<256, 8, EUCLID, false, true>).  Waves 4..7
of a workgroup fold the previous sub-tile's values into their three lowest half a sub-tile later than their SIMD partners
0..3; VQ_NO_STAGGER in the environment (read per call) keeps all eight waves at the early place.  The three lowest values
of a lane are order statistics over distinct codes, so the place changes no output bit.

Each case runs one plain eval search three times in one process -- the default, VQ_NO_STAGGER, and VQ_NO_SCREEN (the fp32
sweep) -- and the three must agree bit for bit: indices, and quantized rows viewed as int32.  A sample of at most 200 rows
is checked against the CPU oracle (indices, and the quantized row = that code's bits).

The adversarial rows sit where waves 4..7 read them, rows 128..255 of a 256-row block, and the oracle sample is drawn from
them only:
  * rows equal to a code;
  * rows equal to / next to a code that is present twice, in two different 32-code tiles (the lowest index must win);
  * rows next to two codes that differ by one ulp in one dim (in two tiles, and in one tile);
  * one row holding a NaN and one holding an inf.

M = 131 073 is the smallest row count at which the persistent kernel is selected on 256 CUs (two row blocks per CU); the
sweep has K / 32 sub-tiles and the kernel takes 32..96 of them."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ADV = 198  # adversarial rows besides the NaN and the inf row: 200 sampled rows in all

#        M            K     D    what it covers
CASES = [
    (131072 + 77, 1024, 256),   # waves 4..7 of the last block own no row
    (131072 + 130, 1024, 256),  # wave 4 of the last block owns 2 rows
    (131072 + 5, 1056, 256),    # 33 sub-tiles: the odd tail, the last epilogue runs after the loop
    (131072 + 5, 1000, 252),    # ragged last tile and ragged D
    (131072 + 5, 3072, 256),    # 96 sub-tiles, the upper end
]


def _native():
    from vector_quantization import native

    native.load()
    return native


def _codebook(k, d, g):
    """randn codes; DUP pairs (a, b): cb[b] = cb[a], a and b in different tiles; ULP pairs: cb[b] = cb[a] one ulp up in one dim."""
    cb = torch.randn((k, d), generator=g)
    dup = [(5, k - 20), (33, 500), (70, 71 + 32 * 5), (k - 40, k - 1)]
    ulp = [(200, 650), (300, 301), (k - 70, k - 3)]
    for a, b in dup:
        assert a // 32 != b // 32 and a < b
        cb[b] = cb[a]
    for a, b in ulp:
        cb[b] = cb[a]
        cb[b, 3] = torch.nextafter(cb[a, 3], torch.tensor(float("inf")))
    return cb, dup, ulp


def _make(m, k, d, seed):
    """x [m, d], cb [k, d] on the host and the adversarial rows (all with row % 256 >= 128: waves 4..7)."""
    g = torch.Generator().manual_seed(seed)
    cb, dup, ulp = _codebook(k, d, g)
    x = torch.randn((m, d), generator=g)
    late = torch.nonzero(torch.arange(m) % 256 >= 128).flatten()
    rows = late[torch.randperm(late.numel(), generator=g)[:N_ADV + 2]]
    tail = late[late >= (m // 256) * 256]  # rows of waves 4..7 in the last, partial block (case 2: two rows)
    if tail.numel():
        rows[:tail.numel()] = tail
        rows = torch.unique(rows)
    code = torch.randint(0, k, (rows.numel(),), generator=g)
    noise = torch.randn((rows.numel(), d), generator=g)
    for n, r in enumerate(rows.tolist()):
        kind = n % 6
        if kind == 0:    # a code itself
            x[r] = cb[code[n]]
        elif kind == 1:  # a duplicated code itself: both copies at distance 0
            x[r] = cb[dup[(n // 6) % len(dup)][0]]
        elif kind == 2:  # next to a duplicated code: both copies at one distance > 0
            x[r] = cb[dup[(n // 6) % len(dup)][1]] + 0.05 * noise[n]
        elif kind == 3:  # one of two codes an ulp apart
            x[r] = cb[ulp[(n // 6) % len(ulp)][(n // 18) % 2]]
        elif kind == 4:  # next to two codes an ulp apart
            x[r] = cb[ulp[(n // 6) % len(ulp)][0]] + 0.05 * noise[n]
        else:            # next to an unrelated code, very close: the screen alone is sure
            x[r] = cb[code[n]] + 1e-3 * noise[n]
    x[rows[-1], 7] = float("nan")
    x[rows[-2], 2] = float("inf")
    return x, cb, rows


def _three(x, cb):
    native = _native()
    runs = {}
    for name, var in (("default", None), ("no_stagger", "VQ_NO_STAGGER"), ("fp32", "VQ_NO_SCREEN")):
        if var:
            os.environ[var] = "1"
        try:
            runs[name] = native.quantize(x, cb, metric=0, want_best=False)
        finally:
            if var:
                os.environ.pop(var, None)
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("m,k,d", CASES, ids=[f"M{m}-K{k}-D{d}" for m, k, d in CASES])
def test_stagger_changes_no_bit(oracle, m, k, d):
    x, cb, rows = _make(m, k, d, seed=1000 + k + d + m % 256)
    assert rows.numel() <= 200 and bool((rows % 256 >= 128).all())
    runs = _three(x[None].to(DEV), cb[None, None].to(DEV))
    a = runs["default"]
    assert a["idx"].shape == (1, m, 1) and a["out"].shape == (1, m, d)
    for other in ("no_stagger", "fp32"):
        b = runs[other]
        assert torch.equal(a["idx"], b["idx"]), other
        assert torch.equal(a["out"].contiguous().view(torch.int32), b["out"].contiguous().view(torch.int32)), other
    assert int(a["idx"].min()) >= 0 and int(a["idx"].max()) < k
    ri, _ = oracle.nearest(x[rows].numpy(), cb.numpy(), 0)
    np.testing.assert_array_equal(a["idx"][0, rows.to(DEV), 0].cpu().numpy(), ri)
    got = a["out"][0, rows.to(DEV)].cpu().numpy().view(np.int32)
    np.testing.assert_array_equal(got, cb.numpy()[ri].view(np.int32))
