"""The row-selection rule of vq_expire_codes_f32, written in numpy from the text of include/vq_mi355x.h alone (a plain module:
it holds no test).  tests/test_expire_rule_host.py checks the rule itself, tests/test_gpu_expire_codes.py the kernel against it."""
from __future__ import annotations

import numpy as np

ROUNDS = 6
WALK_BOUND = 64
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64 -> the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _seed_words(seed):
    """seed [..., 2] int64 -> the two words as uint64 arrays [...]."""
    seed = np.asarray(seed, dtype=np.int64).astype(np.uint64)
    return seed[..., 0], seed[..., 1]


def _key_and_counter(s0, s1, h):
    """The seed's words and the head(s), arrays that broadcast -> (k0, k1, c2, c3)."""
    with np.errstate(over="ignore"):
        c = (np.asarray(h, dtype=np.uint64) << np.uint64(32)) + s1  # mod 2^64
    return s0 & _M32, s0 >> np.uint64(32), c & _M32, c >> np.uint64(32)


def bijection(y, b, s0, s1, h):
    """One application of F on [0, 2^b): six Feistel rounds on uneven halves.  y, s0, s1 (the seed's words), h: arrays (broadcast)."""
    k0, k1, c2, c3 = _key_and_counter(s0, s1, h)
    y = np.asarray(y, dtype=np.uint64)
    wl, wr = b // 2, b - b // 2
    for i in range(ROUNDS):
        hi, lo = y >> np.uint64(wr), y & np.uint64((1 << wr) - 1)
        w0 = philox4x32_10(lo, i, c2, c3, k0, k1)[0]
        y = (lo << np.uint64(wl)) | ((hi ^ w0) & np.uint64((1 << wl) - 1))
        wl, wr = wr, wl
    return y


def select(seed, h, r, n_dead, N, return_steps=False):
    """sel(h, r) for a seed [..., 2] and arrays h, r (all broadcast) -> int64 rows in [0, N); with ``return_steps`` also the
    number of applications of F every walk took (WALK_BOUND + 1 where the bound was reached; 0 for draws with replacement)."""
    s0, s1 = _seed_words(seed)
    s0, s1, h, r = np.broadcast_arrays(s0, s1, np.asarray(h, dtype=np.uint64), np.asarray(r, dtype=np.uint64))
    if n_dead > N:
        k0, k1, c2, c3 = _key_and_counter(s0, s1, h)
        w = philox4x32_10(r, 0xFFFFFFFF, c2, c3, k0, k1)
        sel = ((w[1] << np.uint64(32)) | w[0]) % np.uint64(N)
        return (sel.astype(np.int64), np.zeros(sel.shape, dtype=np.int64)) if return_steps else sel.astype(np.int64)
    b = int(N - 1).bit_length()
    y = r.copy()
    steps = np.zeros(y.shape, dtype=np.int64)
    walking = np.ones(y.shape, dtype=bool)
    for t in range(WALK_BOUND):
        if not walking.any():
            break
        y[walking] = bijection(y[walking], b, s0[walking], s1[walking], h[walking])
        steps[walking] = t + 1
        walking &= y >= np.uint64(N)
    steps[walking] = WALK_BOUND + 1
    y[walking] -= np.uint64(N)
    return (y.astype(np.int64), steps) if return_steps else y.astype(np.int64)
