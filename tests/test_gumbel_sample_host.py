"""CPU suite for the fused Gumbel-max sampling: the C ABI's symbols and argument checks, a numpy restatement of
Philox4x32-10 and of the documented counter packing (include/vq_mi355x.h; the GPU suite imports it from here), and the
chunked path that backends without ``sample_codes`` keep running."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from helpers import OracleBackend

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) c0..c3, key: (k0, k1) -> four uint32 arrays (Salmon et al., SC'11)."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    k0, k1 = int(key[0]) & _MASK, int(key[1]) & _MASK
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_MASK)]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return [v.astype(np.uint32) for v in c]


def noise_bits(seed, H, M, K, row_offset=0):
    """The 32-bit word of every entry (h, m, k) under the documented packing: key = seed[0], counter = (row lo, row hi,
    ((h << 32) | (k >> 2)) + seed[1] lo, hi), word k & 3.  seed: two Python ints (int64 values).  -> uint32 [H, M, K]."""
    s0, s1 = int(seed[0]) & (2 ** 64 - 1), int(seed[1]) & (2 ** 64 - 1)
    groups = (K + 3) // 4
    h, m, g = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(M, dtype=np.uint64) + np.uint64(row_offset),
                          np.arange(groups, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        hi = ((h << np.uint64(32)) | g) + np.uint64(s1)  # mod 2^64
    words = philox4x32_10([m & np.uint64(_MASK), m >> np.uint64(32), hi & np.uint64(_MASK), hi >> np.uint64(32)],
                          (s0 & _MASK, s0 >> 32))
    return np.stack(words, axis=-1).reshape(H, M, groups * 4)[:, :, :K]


def gumbel64(bits):
    """fp64 double-clamped transform of the words: u = (w >> 8) * 2^-24, g = -log(max(-log(max(u, 1e-5)), 1e-5))."""
    u = (bits >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return -np.log(np.maximum(-np.log(np.maximum(u, 1e-5)), 1e-5))


def test_philox_known_answers():
    """The published known-answer vectors of Philox4x32-10 (Random123 kat_vectors)."""
    cases = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((_MASK,) * 4, (_MASK, _MASK), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for counter, key, want in cases:
        got = tuple(int(v) for v in philox4x32_10(counter, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])


def test_packing_keeps_rows_heads_and_codes_apart():
    """Rows keep 64 bits, heads and code groups never alias, seed word 1 offsets the upper counter half."""
    seed = (0x0123456789ABCDEF, -5)
    base = noise_bits(seed, 2, 3, 9)
    assert base.shape == (2, 3, 9) and len(np.unique(base)) == base.size
    far = noise_bits(seed, 1, 1, 8, row_offset=2 ** 32)  # row 2^32 differs from row 0 through c1 alone
    assert not np.array_equal(far[0, 0], base[0, 0, :8])
    # seed[1] = -5 wraps the 64-bit sum: group 5 of head 0 is counter half 0
    want = philox4x32_10([0, 0, 0, 0], (seed[0] & _MASK, (seed[0] >> 32) & _MASK))
    assert [int(v) for v in want] == [int(v) for v in noise_bits(seed, 1, 1, 24)[0, 0, 20:24]]
    g = gumbel64(np.array([0, 0xFFFFFFFF, 0x80000000], dtype=np.uint32))
    assert abs(g[0] + math.log(-math.log(1e-5))) < 1e-12 and abs(g[1] + math.log(1e-5)) < 1e-12
    assert abs(g[2] + math.log(math.log(2.0))) < 1e-12


def test_symbols_exported_and_arguments_checked():
    from vector_quantization import native

    lib = native.load()
    for name in ("vq_gumbel_sample_f32", "vq_gumbel_noise_f32"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.vq_gumbel_sample_f32(None, 1.0, None, None) == -1
    assert b"null" in lib.vq_last_error()
    a = native.VqArgs()
    a.H, a.Q, a.M, a.K, a.D = 1, 1, 0, 4, 4
    for tau in (float("inf"), float("-inf"), float("nan")):
        assert lib.vq_gumbel_sample_f32(ctypes.byref(a), tau, None, None) == -1
        assert b"tau" in lib.vq_last_error()
    assert lib.vq_gumbel_sample_f32(ctypes.byref(a), 1.0, None, None) == -1 and b"seed" in lib.vq_last_error()
    a.K = 0
    assert lib.vq_gumbel_sample_f32(ctypes.byref(a), 1.0, None, None) == -1 and b"non-positive" in lib.vq_last_error()
    assert lib.vq_gumbel_noise_f32(None, 1, 1, 1, None, None, None) == -1 and b"null" in lib.vq_last_error()


def test_draw_seed_follows_the_generator():
    from vector_quantization import gumbel

    torch.manual_seed(11)
    a = gumbel.draw_seed("cpu")
    torch.manual_seed(11)
    b = gumbel.draw_seed("cpu")
    c = gumbel.draw_seed("cpu")
    assert a.dtype == torch.int64 and tuple(a.shape) == (2,) and torch.equal(a, b) and not torch.equal(a, c)


def test_op_is_registered_with_a_fake_implementation():
    import vector_quantization  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x, cb = torch.empty((2, 77, 48)), torch.empty((2, 100, 48))
        idx = torch.ops.vq_mi355x.gumbel_sample(x, cb, None, torch.empty((2,), dtype=torch.int64), 0, 1.25)
        assert idx.shape == (2, 77) and idx.dtype == torch.int64


def test_backend_without_the_sweep_runs_the_chunked_loop(oracle):
    """The CPU checker backend has no ``sample_codes``: a stochastic Codebook forward still samples through the chunked
    loop -- valid indices, the gathered rows, equal seeds equal draws."""
    from vector_quantization import search
    from vector_quantization.codebook import Codebook
    from vector_quantization.codebooks import GumbelParams

    assert not hasattr(OracleBackend, "sample_codes")
    search.set_backend(OracleBackend)
    try:
        torch.manual_seed(2)
        cb = Codebook(dim=8, codebook_size=20, gumbel_params=GumbelParams(stochastic=True, temperature=0.8)).eval()
        x = torch.randn(1, 300, 8)
        torch.manual_seed(5)
        q, ind, _ = cb(x, return_similarities=False)
        torch.manual_seed(5)
        ind2 = cb(x, return_similarities=False)[1]
    finally:
        search.set_backend(None)
    assert ind.dtype == torch.int64 and tuple(ind.shape) == (1, 300)
    assert int(ind.min()) >= 0 and int(ind.max()) < 20 and len(torch.unique(ind)) > 3
    assert torch.equal(q, cb.embeddings[0][ind]) and torch.equal(ind, ind2)
