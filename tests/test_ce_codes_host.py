"""Host side of the cross-entropy loss's fused gradient with respect to a learnable codebook (no GPU): the yardstick of
tests/test_gpu_ce_codes.py itself -- the fp64 closed form of tests/ce_codes_run.py against what the reference recorded in the
tests/golden/data/ce_codes_<case>.npz fixtures and against autograd of the reference's op sequence --, the C ABI's symbols,
argument rules and documented workspace layout, and the dispatch rule of losses._CrossEntropyFn."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from ce_codes_cases import CE_CODES_CASES
from ce_codes_run import EXACT, closed_form, fixture_closed_form, reference_sequence
from gumbel_run import assert_grad_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vq_ce_codes_workspace_bytes", "vq_ce_backward_codes_f32")
E_BADARG, E_UNSUPPORTED = -1, -2
P = 0x4000  # a non-null, 16-byte aligned address


@pytest.fixture(scope="module")
def lib():
    from vector_quantization import native

    return native.load()


# ------------------------------------------------------------------------------------------------ the yardstick itself
@pytest.mark.parametrize("name", list(CE_CODES_CASES))
def test_closed_form_reproduces_the_reference_fixture(name):
    """loss, dL/dx and dL/dcodebook of the fp64 closed form against the reference's recorded fp32 results."""
    arrays, got = fixture_closed_form(name)
    assert float(abs(arrays["gcb"]).max()) > 0 and arrays["gcb"].shape == arrays["cb"].shape
    assert_grad_close(arrays["loss"], got["loss"], f"{name} loss")
    assert_grad_close(arrays["gx"], got["gx"], f"{name} dL/dx")
    assert_grad_close(arrays["gcb"], got["gcb"], f"{name} dL/dcodebook")


def test_fixtures_cover_ignored_rows():
    from helpers import load_golden

    for name in ("commit_mask", "indices_ignore"):
        arrays, _ = load_golden("ce_codes_" + name)
        assert int((arrays["embed_ind"] < 0).sum()) > 0, name


@pytest.mark.parametrize("dot", [False, True], ids=["euclid", "dot"])
def test_closed_form_is_autograd_of_the_reference_sequence(dot):
    g = torch.Generator().manual_seed(5)
    x, c = torch.randn((2, 37, 12), generator=g), torch.randn((2, 19, 12), generator=g)
    target = torch.randint(0, 19, (2, 37), generator=g)
    target[0, ::5] = -1
    target[1, 3], target[1, 4] = 19, 2 ** 32 + 3
    x[0, 5], x[1, 3, 2], x[1, 4, 0] = float("nan"), float("inf"), float("-inf")  # ignored rows: never read
    x[0, 1] = c[0, 7]  # a zero distance, not the target ...
    x[0, 2], target[0, 2] = c[0, 3], 3  # ... and as the target
    got = closed_form(x, c, target, dot, g_loss=0.7)
    # (cdist from the differences on both sides: through the GEMM a zero distance is a cancellation residue, not 0)
    ref = reference_sequence(x, c, target, dot, g_loss=0.7, dtype=torch.float64, compute_mode=EXACT)
    assert got["count"] == ref["count"] == 2 * 37 - 8 - 2
    torch.testing.assert_close(got["loss"], ref["loss"], rtol=1e-12, atol=0)
    for key in ("gx", "gc"):
        assert bool(torch.isfinite(got[key]).all()) and float(ref[key].abs().max()) > 0
        torch.testing.assert_close(got[key], ref[key], rtol=1e-9, atol=1e-12 * float(ref[key].abs().max()))


@pytest.mark.parametrize("dot", [False, True], ids=["euclid", "dot"])
def test_one_code_has_no_gradient(dot):
    g = torch.Generator().manual_seed(6)
    x, c = torch.randn((1, 24, 8), generator=g), torch.randn((1, 1, 8), generator=g)
    target = torch.zeros((1, 24), dtype=torch.int64)
    assert not bool(closed_form(x, c, target, dot, g_loss=0.7)["gc"].any())
    assert not bool(reference_sequence(x, c, target, dot, g_loss=0.7)["gc"].any())


# ------------------------------------------------------------------------------------------------ symbols, arguments
def test_symbols_declared_listed_and_exported(lib):
    from vector_quantization import native

    header = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in vq_mi355x.h"
        assert name in native.EXPORTED_SYMBOLS and name in native._SIGNATURES
        assert hasattr(lib, name)
    assert callable(native.ce_backward_codes) and callable(native.ce_codes_supported)
    assert "Gradient with respect to the codebook is not produced" not in header


def _args(native, M=64, K=40, D=16, H=1):
    """vq_args with fake (never dereferenced: every call below fails validation before a launch) 16-byte aligned pointers."""
    a = native.VqArgs()
    a.H, a.Q, a.M, a.K, a.D, a.metric = H, 1, M, K, D, 0
    a.x, a.x_rs, a.x_hs = 0x1000, D, M * D
    a.cb, a.cb_hs = 0x2000, K * D
    return a


def _call(lib, a, lse=P, target=P, coef=P, gc=P, ws=P, ws_bytes=1 << 40):
    return lib.vq_ce_backward_codes_f32(ctypes.byref(a), lse, target, 1, a.M, coef, gc, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """Fake pointers throughout: every call fails validation before anything is dereferenced or launched."""
    from vector_quantization import native

    a = _args(native)  # M = 64, K = 40, D = 16
    for name in ("lse", "target", "coef", "gc"):
        assert _call(lib, a, **{name: None}) == E_BADARG and b"null argument" in lib.vq_last_error(), name
    b = _args(native)
    b.cb = None
    assert _call(lib, b) == E_BADARG and b"cb" in lib.vq_last_error()
    assert _call(lib, _args(native, D=257)) == E_UNSUPPORTED and b"D > 256" in lib.vq_last_error()
    assert _call(lib, _args(native, M=1 << 31)) == E_UNSUPPORTED and b"too many rows" in lib.vq_last_error()
    assert _call(lib, _args(native, M=(1 << 21) + 1, D=256)) == E_UNSUPPORTED and b"2 GiB" in lib.vq_last_error()
    assert _call(lib, a, ws=None) == E_BADARG and b"workspace" in lib.vq_last_error()
    assert _call(lib, a, ws=P + 8) == E_BADARG and b"workspace" in lib.vq_last_error()
    need = lib.vq_ce_codes_workspace_bytes(1, 64, 40, 16)
    assert need > 0
    assert _call(lib, a, ws_bytes=need - 1) == E_BADARG and b"vq_ce_codes_workspace_bytes" in lib.vq_last_error()
    # an empty call still needs somewhere to write and a coef
    assert _call(lib, _args(native, M=0), gc=None) == E_BADARG and _call(lib, _args(native, M=0), coef=None) == E_BADARG


# ------------------------------------------------------------------------------------------------ workspace layout
def _cus():
    """What the plan divides by: the device's compute units, 256 when there is no device to ask."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def documented_floats(H, M, K, D, cus):
    """The layout in vq_mi355x.h, restated -> (4-byte units, splits)."""
    dp = next(p for p in (32, 64, 128, 256) if D <= p)
    tile = 32 * max(1, 256 // dp)
    mp = (M + tile - 1) // tile * tile
    ntiles = mp // tile
    want = max(1, min(64, ntiles, -(-cus // ((K + 127) // 128 * H))))
    per = -(-ntiles // want)
    splits = -(-ntiles // per)
    rs_m = (M + 255) // 256 * 256
    return H * (mp * (dp + 4) + 2048) + 2 * H * rs_m + (splits * H * K * D if splits > 1 else 0), splits


SIZES = [(1, 33, 301, 100), (1, 5, 40, 16), (1, 1, 7, 5), (1, 24, 1, 8), (1, 72, 1000, 128), (1, 96, 512, 256), (2, 64, 130, 32),
         (1, 2100, 64, 32), (1, 64 * 256, 4096, 64), (4, 256 * 1024, 1024, 256), (1, 64 * 1024, 8192, 64)]


@pytest.mark.parametrize("shape", SIZES)
def test_workspace_size_is_the_documented_layout(lib, shape):
    want, _ = documented_floats(*shape, _cus())
    assert lib.vq_ce_codes_workspace_bytes(*shape) == 4 * want
    H, M, K, D = shape
    assert lib.vq_packed_floats(M, D) * H + 2 * H * lib.vq_gumbel_row_stride(M) <= want


def test_layout_cases_cover_one_split_and_several():
    counts = {documented_floats(*shape, 256)[1] for shape in SIZES}
    assert 1 in counts and max(counts) > 1 and max(counts) <= 64
    # the memory test's shape: a few MiB of image and 8 partials of 1 MiB
    floats, splits = documented_floats(1, 64 * 256, 4096, 64, 256)
    assert splits == 8 and floats * 4 < 16 << 20


def test_workspace_size_rejects_unsupported_shapes(lib):
    for bad in ((0, 96, 256, 64), (1, 0, 256, 64), (1, 96, 0, 64), (1, 96, 256, 0), (1, 96, 256, 257), (1, 1 << 31, 256, 64)):
        assert lib.vq_ce_codes_workspace_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ dispatch
def test_the_cut_is_a_pure_function_of_the_shape():
    from vector_quantization import losses

    assert set(losses.CE_CODES_FUSED_MIN_ROWS) == {32, 64, 128, 256}
    for dp, cut in losses.CE_CODES_FUSED_MIN_ROWS.items():
        assert losses.ce_codes_runs_fused(cut, dp) and not losses.ce_codes_runs_fused(cut - 1, dp)
        assert losses.ce_codes_runs_fused(cut, dp - 31) == losses.ce_codes_runs_fused(cut, dp)
    assert not losses.ce_codes_runs_fused(1 << 20, 257)


def test_backends_without_the_sweep_and_switched_off_calls_keep_the_chunks(monkeypatch):
    """On the CPU with the oracle backend the loss runs on the chunks (helpers.OracleBackend has no codes sweep), and so does
    any call under VQ_CE_CODES_NO_FUSED=1 or with live codes: _ce_codes_fused says no before it asks the backend."""
    from helpers import OracleBackend
    from vector_quantization import losses, search

    assert not hasattr(OracleBackend, "cross_entropy_backward_codes")
    assert hasattr(search._NativeBackend, "cross_entropy_backward_codes")
    x, c = torch.randn(1, 40, 8), torch.randn(1, 9, 8)
    monkeypatch.setattr(search, "get_backend", lambda: OracleBackend)
    assert not losses._ce_codes_fused(x, c, None)

    class OnDevice(torch.Tensor):
        is_cuda = True

    xd = x.as_subclass(OnDevice)
    monkeypatch.setattr(search, "get_backend", lambda: search._NativeBackend)
    assert losses._ce_codes_fused(xd, c, None)
    assert not losses._ce_codes_fused(xd, c, c.clone()), "live codes keep the chunked path"
    monkeypatch.setenv("VQ_CE_CODES_NO_FUSED", "1")
    assert not losses._ce_codes_fused(xd, c, None)
    monkeypatch.delenv("VQ_CE_CODES_NO_FUSED")
    assert not losses._ce_codes_fused(torch.randn(1, 40, 300).as_subclass(OnDevice), c, None), "D > 256 keeps the chunked path"
