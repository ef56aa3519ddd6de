"""Host side of the fused codebook diversity loss (no GPU): the C ABI's symbols and argument rules, the documented workspace
layout, the dispatch rule, and the yardstick of tests/test_gpu_diversity.py itself -- the fp64 closed form against torch
autograd of the reference's formula."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from diversity_run import CLAMP, clamp_margin, closed_form64, make_inputs, reference_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vq_diversity_workspace_bytes", "vq_diversity_stats_f32", "vq_diversity_accumulate_f32", "vq_diversity_delta_f32",
           "vq_diversity_backward_x_f32")
E_BADARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from vector_quantization import native

    return native.load()


def test_symbols_declared_listed_and_exported(lib):
    from vector_quantization import native

    header = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in vq_mi355x.h"
        assert name in native.EXPORTED_SYMBOLS and name in native._SIGNATURES
        assert hasattr(lib, name)


# ------------------------------------------------------------------------------------------------ argument validation
def _args(native, M=64, K=40, D=16, H=1):
    """vq_args with fake (never dereferenced: every call below fails validation before a launch) 16-byte aligned pointers."""
    a = native.VqArgs()
    a.H, a.Q, a.M, a.K, a.D, a.metric = H, 1, M, K, D, 0
    a.x, a.x_rs, a.x_hs = 0x1000, D, M * D
    a.cb, a.cb_hs = 0x2000, K * D
    a.packed, a.pk_hs = 0x3000, 0
    return a


P = 0x4000  # a non-null, 16-byte aligned address


def _calls(native, lib, a, T=1.0, N=4, pos_div=1, lse=P, A=P, ws=P, ws_bytes=1 << 40, U=P, delta=P, gx=P):
    r = ctypes.byref(a)
    return {
        "stats": lambda: lib.vq_diversity_stats_f32(r, T, lse, None),
        "accumulate": lambda: lib.vq_diversity_accumulate_f32(r, T, N, pos_div, lse, A, ws, ws_bytes, None),
        "delta": lambda: lib.vq_diversity_delta_f32(r, T, N, pos_div, lse, U, delta, None),
        "backward_x": lambda: lib.vq_diversity_backward_x_f32(r, None, 0, T, N, pos_div, lse, delta, U, gx, 16, 0, None),
    }


@pytest.mark.parametrize("entry", ["stats", "accumulate", "delta", "backward_x"])
def test_bad_arguments_are_rejected_before_any_launch(lib, entry):
    from vector_quantization import native

    a = _args(native)
    for bad_t in (float("nan"), float("inf"), float("-inf")):
        assert _calls(native, lib, a, T=bad_t)[entry]() == E_BADARG and b"T is not finite" in lib.vq_last_error()
    assert _calls(native, lib, a, lse=None)[entry]() == E_BADARG
    assert _calls(native, lib, a, lse=P + 4)[entry]() == E_BADARG and b"16-byte" in lib.vq_last_error()
    assert _calls(native, lib, _args(native, D=257))[entry]() == E_UNSUPPORTED and b"D > 256" in lib.vq_last_error()
    if entry != "stats":
        for n, pd in ((0, 1), (-3, 1), (4, 0), (5, 1), (4, 3), (64, 2)):  # M = 64 rows
            assert _calls(native, lib, a, N=n, pos_div=pd)[entry]() == E_BADARG, (n, pd)
            assert b"multiple of N * pos_div" in lib.vq_last_error()
    if entry == "accumulate":
        assert _calls(native, lib, a, A=None)[entry]() == E_BADARG
        assert _calls(native, lib, a, ws=None)[entry]() == E_BADARG and b"workspace" in lib.vq_last_error()
        need = lib.vq_diversity_workspace_bytes(1, 64, 40, 16, 4)
        assert _calls(native, lib, a, ws_bytes=need - 1)[entry]() == E_BADARG and b"workspace" in lib.vq_last_error()
        b = _args(native)
        b.cb = None
        assert _calls(native, lib, b)[entry]() == E_BADARG and b"cb is null" in lib.vq_last_error()
    if entry in ("delta", "backward_x"):
        assert _calls(native, lib, a, U=None)[entry]() == E_BADARG
        assert _calls(native, lib, a, delta=None)[entry]() == E_BADARG
        b = _args(native)
        b.packed = None
        assert _calls(native, lib, b)[entry]() == E_BADARG and b"packed" in lib.vq_last_error()
    if entry == "backward_x":
        assert _calls(native, lib, a, gx=None)[entry]() == E_BADARG and b"grad_x" in lib.vq_last_error()


@pytest.mark.parametrize("entry", ["stats", "accumulate", "delta", "backward_x"])
def test_no_rows_is_a_valid_empty_call(lib, entry):
    from vector_quantization import native

    assert _calls(native, lib, _args(native, M=0))[entry]() == 0


# ------------------------------------------------------------------------------------------------ workspace layout
def _documented_floats(H, M, K, D, N):
    """The layout in vq_mi355x.h, restated."""
    dp = next(p for p in (32, 64, 128, 256) if D <= p)
    cp = (M // N + 31) // 32 * 32
    tile = 32 * max(1, 256 // dp)
    mp = (N * cp + tile - 1) // tile * tile
    rsk = (K + 255) // 256 * 256
    return H * (mp * (dp + 4) + 2048) + H * mp + H * N * rsk


@pytest.mark.parametrize("shape", [(1, 96, 256, 64, 3), (1, 66, 301, 100, 2), (1, 35, 40, 16, 7), (1, 40, 7, 5, 40), (2, 64, 130, 32, 4),
                                   (1, 96, 512, 256, 3), (4, 256 * 1024, 1024, 256, 1024), (1, 70, 520, 64, 1)])
def test_workspace_size_is_the_documented_layout(lib, shape):
    H, M, K, D, N = shape
    assert lib.vq_diversity_workspace_bytes(H, M, K, D, N) == 4 * _documented_floats(H, M, K, D, N)
    assert lib.vq_gumbel_row_stride(K) == (K + 255) // 256 * 256


def test_workspace_size_rejects_what_the_sweeps_reject(lib):
    ok = (1, 96, 256, 64, 3)
    assert lib.vq_diversity_workspace_bytes(*ok) > 0
    for bad in ((0, 96, 256, 64, 3), (1, 0, 256, 64, 3), (1, 96, 0, 64, 3), (1, 96, 256, 0, 3), (1, 96, 256, 257, 3), (1, 96, 256, 64, 0),
                (1, 96, 256, 64, 5), (1, 1 << 31, 256, 64, 1 << 10), (1, 1 << 24, 256, 256, 1 << 24)):
        assert lib.vq_diversity_workspace_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ dispatch
def test_dispatch_is_a_pure_function_of_the_shape():
    from vector_quantization import losses

    cut = losses.DIVERSITY_FUSED_MIN_ROWS
    assert 1 <= cut <= 32
    for c in (32, 33, 64, 1000):
        assert losses.diversity_runs_fused(c) and losses.diversity_runs_fused(c, heads=4)  # C >= 32 always runs fused
    for c in range(1, 32):
        assert losses.diversity_runs_fused(c) == (c >= cut)
        assert losses.diversity_runs_fused(c, heads=2) == (c // 2 >= cut)  # what is padded are the rows of ONE head
    # monotone: more rows per position never leave the fused path
    runs = [losses.diversity_runs_fused(c) for c in range(1, 80)]
    assert runs == sorted(runs)


def test_fallback_conditions_without_a_device(monkeypatch):
    """CPU tensors, a learnable codebook and VQ_DIVERSITY_NO_FUSED=1 keep the chunked path (here: it is asked for the
    similarities, which a recording backend serves)."""
    from vector_quantization import losses, search

    calls = []

    class Recording:
        @staticmethod
        def similarities(x, cb, *, metric, out=None):
            calls.append("similarities")
            return x @ cb.transpose(-1, -2) if metric == search.DOT else -torch.cdist(x, cb)

        @staticmethod
        def diversity_table(*a, **k):
            raise AssertionError("the fused path must not run here")

        diversity_backward = diversity_supported = diversity_table

    monkeypatch.setattr(search, "_backend", Recording)
    x, c = make_inputs(1, 32, 3, 20, 8, False, 1)
    pos = (torch.arange(96) % 3)
    loss = losses.codebook_diversity_loss(x, c, search.EUCLID, 1.0, lambda: pos, 3, pos_div=1)
    want = closed_form64(x, c, 1.0, 3, 1, False)["loss"]
    assert calls and abs(float(loss) - float(want)) < 1e-5 * abs(float(want))
    assert losses._diversity_fused_backend(x, c, 3, 1) is None  # CPU tensors


# ------------------------------------------------------------------------------------------------ the yardstick itself
CASES = [  # (H, B, N, K, D), metric_dot, T, pos_div, seed
    ((1, 32, 3, 64, 16), False, 1.0, 1, 11),
    ((1, 32, 3, 64, 16), False, 100.0, 1, 11),
    ((1, 33, 2, 50, 12), True, 100.0, 1, 12),
    ((2, 16, 4, 30, 8), False, 1.0, 1, 13),
    ((1, 6, 5, 40, 8), True, 1.0, 2, 14),
    ((1, 6, 5, 40, 8), False, 100.0, 2, 15),
]


@pytest.mark.parametrize("live", [False, True], ids=["plain", "live"])
@pytest.mark.parametrize("shape,dot,T,pos_div,seed", CASES)
def test_closed_form_is_autograd_of_the_reference_formula(shape, dot, T, pos_div, seed, live):
    h, b, n, k, d = shape
    x, c = make_inputs(h, b, n, k, d, dot, seed, pos_div)
    lv = c + 0.05 * torch.randn(c.shape, generator=torch.Generator().manual_seed(seed + 100)) if live else None
    got = closed_form64(x, c, T, n, pos_div, dot, live=lv, g_loss=0.7)
    ref = reference_sequence(x, c, T, n, pos_div, dot, dtype=torch.float64, live=lv, g_loss=0.7)
    assert clamp_margin(got["A"]) > 0.02
    torch.testing.assert_close(got["A"], ref["A"], rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(got["loss"], ref["loss"], rtol=1e-12, atol=0)
    torch.testing.assert_close(got["lse"], ref["lse"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got["gx"], ref["gx"], rtol=1e-9, atol=1e-12 * float(ref["gx"].abs().max()))
    if T == 100.0:  # the clamp is active on some entries and inactive on others: both branches of U are exercised
        assert bool((got["A"] < CLAMP).any()) and bool((got["A"] >= CLAMP).any())
    # delta is what the closed form says it is: the p-weighted mean of U in the row's position
    p = (-T * (x.double() @ c.double().transpose(-1, -2) if dot else -torch.cdist(x.double(), c.double()))).softmax(-1)
    pos = (torch.arange(x.shape[1]) // pos_div) % n
    torch.testing.assert_close(got["delta"], (p * got["U"][pos]).sum(-1), rtol=1e-12, atol=0)


def test_position_rule_matches_the_quantizer_layouts():
    """(m // pos_div) % N is row % N for separate heads / one head and (row // heads) % N for shared heads."""
    from diversity_run import positions

    n, heads, batch = 5, 3, 4
    rows = torch.arange(batch * n)
    assert torch.equal(positions(batch * n, n, 1), rows % n)
    rows = torch.arange(batch * n * heads)
    assert torch.equal(positions(batch * n * heads, n, heads), (rows // heads) % n)
