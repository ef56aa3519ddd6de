"""CPU: the row-selection rule of vq_expire_codes_f32 as include/vq_mi355x.h states it (tests/expire_rule.py is that text in
numpy): a bijection of [0, N) whose cycle walk stays far from its bound, and picks as uniform as torch.randperm's."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import expire_rule as er

SIZES = [1, 2, 3, 5, 64, 1000, 4097]


def _seeds(n, start):
    g = np.random.default_rng(start)
    return g.integers(-(2 ** 63), 2 ** 63 - 1, size=(n, 2), dtype=np.int64)


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32_10 (counter, key -> output)."""
    assert [int(w) for w in er.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(w) for w in er.philox4x32_10(f, f, f, f, f, f)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    got = er.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(w) for w in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


@pytest.mark.parametrize("N", SIZES)
def test_selection_is_a_bijection_of_the_rows(N):
    for seed in _seeds(8, 100 + N):
        for h in (0, 1, 77):
            sel = er.select(seed, h, np.arange(N), N, N)
            assert sel.min() >= 0 and sel.max() < N
            assert len(np.unique(sel)) == N, (N, seed, h)
    # a shorter list of dead codes takes the first ranks of the same permutation: sel does not depend on n_dead <= N
    seed = _seeds(1, 5)[0]
    assert np.array_equal(er.select(seed, 2, np.arange(N // 2 + 1), N // 2 + 1, N), er.select(seed, 2, np.arange(N), N, N)[:N // 2 + 1])


@pytest.mark.parametrize("N", SIZES)
def test_the_walk_bound_is_never_reached(N):
    seeds = _seeds(1000, 7 * N)
    worst = 0
    for some in np.array_split(seeds, 10):  # (every rank of every seed, a hundred seeds at a time)
        _, steps = er.select(some[:, None, :], 0, np.arange(N)[None, :], N, N, return_steps=True)
        worst = max(worst, int(steps.max()))
    print(f"N = {N}: longest walk {worst} applications (bound {er.WALK_BOUND})")
    assert worst <= er.WALK_BOUND
    domain = 1 << int(N - 1).bit_length() if N > 1 else 1
    if domain - N < er.WALK_BOUND:  # a walk leaves [0, N) for at most 2^b - N applications in a row
        assert worst <= domain - N + 1


def test_draws_with_replacement_are_in_range_and_depend_on_the_rank():
    seed = _seeds(1, 9)[0]
    sel = er.select(seed, 3, np.arange(40), 40, 7)
    assert sel.min() >= 0 and sel.max() < 7 and len(np.unique(sel)) == 7
    assert not np.array_equal(sel, er.select(seed, 4, np.arange(40), 40, 7))


BAND = (512 - 118, 512 + 118)  # 6 sigma, sigma = sqrt(2048 * 1/4 * 3/4) = 19.6


def test_picks_are_uniform_over_the_rows():
    """N = 64, 16 dead codes, 2048 heads of one seed: every row is picked 512 +- 118 times."""
    seed = np.array([0x1234567, -0x7654321], dtype=np.int64)
    h, r = np.meshgrid(np.arange(2048), np.arange(16), indexing="ij")
    sel = er.select(seed, h, r, 16, 64)
    assert all(len(np.unique(row)) == 16 for row in sel)
    counts = np.bincount(sel.reshape(-1), minlength=64)
    print("rule: pick counts", counts.min(), "..", counts.max())
    assert counts.min() >= BAND[0] and counts.max() <= BAND[1]


def test_the_band_is_one_torch_randperm_keeps():
    g = torch.Generator().manual_seed(20240607)
    picks = torch.stack([torch.randperm(64, generator=g)[:16] for _ in range(2048)])
    counts = torch.bincount(picks.reshape(-1), minlength=64)
    print("randperm: pick counts", int(counts.min()), "..", int(counts.max()))
    assert int(counts.min()) >= BAND[0] and int(counts.max()) <= BAND[1]
