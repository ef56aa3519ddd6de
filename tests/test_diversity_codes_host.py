"""Host side of the diversity loss's fused gradient with respect to a learnable codebook (no GPU): the yardstick of
tests/test_gpu_diversity_codes.py itself -- the fp64 closed form of gc against torch autograd of the reference's formula --,
the C ABI's symbols, argument rules and documented workspace layout, and the dispatch of losses.codebook_diversity_loss with
codes that require grad."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from diversity_codes_run import codes_gradient64, reference_sequence_codes
from diversity_run import clamp_margin, make_inputs, positions, similarities
from test_diversity_host import CASES, E_BADARG, E_UNSUPPORTED, P, _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vq_diversity_codes_workspace_bytes", "vq_diversity_backward_codes_f32")
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def lib():
    from vector_quantization import native

    return native.load()


# ------------------------------------------------------------------------------------------------ the yardstick itself
@pytest.mark.parametrize("shape,dot,T,pos_div,seed", CASES)
def test_closed_form_is_autograd_of_the_reference_formula(shape, dot, T, pos_div, seed):
    h, b, n, k, d = shape
    x, c = make_inputs(h, b, n, k, d, dot, seed, pos_div)
    got = codes_gradient64(x, c, T, n, pos_div, dot, g_loss=0.7)
    ref = reference_sequence_codes(x, c, T, n, pos_div, dot, dtype=torch.float64, g_loss=0.7)
    assert clamp_margin(got["A"]) > 0.02
    torch.testing.assert_close(got["loss"], ref["loss"], rtol=1e-12, atol=0)
    torch.testing.assert_close(got["gx"], ref["gx"], rtol=1e-9, atol=1e-12 * float(ref["gx"].abs().max()))
    assert float(ref["gc"].abs().max()) > 0
    torch.testing.assert_close(got["gc"], ref["gc"], rtol=1e-9, atol=1e-12 * float(ref["gc"].abs().max()))


@pytest.mark.parametrize("dot", [False, True], ids=["euclid", "dot"])
def test_one_code_has_no_gradient(dot):
    x, c = make_inputs(1, 8, 3, 1, 8, dot, 1)
    got = codes_gradient64(x, c, 100.0, 3, 1, dot, g_loss=0.7)
    ref = reference_sequence_codes(x, c, 100.0, 3, 1, dot, dtype=torch.float64, g_loss=0.7)
    assert not bool(got["gc"].any()) and float(ref["gc"].abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------ symbols, arguments
def test_symbols_declared_listed_and_exported(lib):
    from vector_quantization import native

    header = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in vq_mi355x.h"
        assert name in native.EXPORTED_SYMBOLS and name in native._SIGNATURES
        assert hasattr(lib, name)
    assert callable(native.diversity_backward_codes) and callable(native.diversity_codes_supported)


def _call(lib, a, T=1.0, N=4, pos_div=1, lse=P, delta=P, U=P, gc=P, ws=P, ws_bytes=1 << 40):
    return lib.vq_diversity_backward_codes_f32(ctypes.byref(a), T, N, pos_div, lse, delta, U, gc, ws, ws_bytes, None)


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """Fake pointers throughout: every call fails validation before anything is dereferenced or launched."""
    from vector_quantization import native

    a = _args(native)  # M = 64, K = 40, D = 16
    for bad_t in (float("nan"), float("inf"), float("-inf")):
        assert _call(lib, a, T=bad_t) == E_BADARG and b"T is not finite" in lib.vq_last_error()
    for name in ("lse", "delta", "U"):
        assert _call(lib, a, **{name: None}) == E_BADARG, name
        assert _call(lib, a, **{name: P + 4}) == E_BADARG and b"16-byte" in lib.vq_last_error(), name
    assert _call(lib, _args(native, D=257)) == E_UNSUPPORTED and b"D > 256" in lib.vq_last_error()
    for n, pd in ((0, 1), (-3, 1), (4, 0), (5, 1), (4, 3), (64, 2)):
        assert _call(lib, a, N=n, pos_div=pd) == E_BADARG, (n, pd)
        assert b"multiple of N * pos_div" in lib.vq_last_error()
    assert _call(lib, a, gc=None) == E_BADARG and b"grad_codes" in lib.vq_last_error()
    b = _args(native)
    b.cb = None
    assert _call(lib, b) == E_BADARG and b"cb" in lib.vq_last_error()
    assert _call(lib, a, ws=None) == E_BADARG and b"workspace" in lib.vq_last_error()
    assert _call(lib, a, ws=P + 8) == E_BADARG and b"workspace" in lib.vq_last_error()
    need = lib.vq_diversity_codes_workspace_bytes(1, 64, 40, 16, 4)
    assert need > 0
    assert _call(lib, a, ws_bytes=need - 1) == E_BADARG and b"workspace" in lib.vq_last_error()
    # (an empty call is rejected on the same grounds before it would clear grad_codes)
    assert _call(lib, _args(native, M=0), gc=None) == E_BADARG and _call(lib, _args(native, M=0), T=float("nan")) == E_BADARG


# ------------------------------------------------------------------------------------------------ workspace layout
def _cus():
    """What the plan divides by: the device's compute units, 256 when there is no device to ask."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _documented_floats(H, M, K, D, N, cus):
    """The layout in vq_mi355x.h, restated."""
    dp = next(p for p in (32, 64, 128, 256) if D <= p)
    cp = (M // N + 31) // 32 * 32
    tile = 32 * max(1, 256 // dp)
    mp = (N * cp + tile - 1) // tile * tile
    ntiles = mp // tile
    want = max(1, min(64, ntiles, -(-cus // ((K + 127) // 128 * H))))
    per = -(-ntiles // want)
    splits = -(-ntiles // per)
    return H * (mp * (dp + 4) + 2048) + 2 * H * mp + (splits * H * K * D if splits > 1 else 0), splits


SIZES = [(1, 96, 256, 64, 3), (1, 66, 301, 100, 2), (1, 35, 40, 16, 7), (1, 40, 7, 5, 40), (2, 64, 130, 32, 4), (1, 96, 512, 256, 3),
         (4, 256 * 1024, 1024, 256, 1024), (1, 70, 520, 64, 1), (1, 140, 64, 32, 70), (1, 240, 64, 64, 6), (1, 64 * 1024, 8192, 64, 1024)]


@pytest.mark.parametrize("shape", SIZES)
def test_workspace_size_is_the_documented_layout(lib, shape):
    want, _ = _documented_floats(*shape, _cus())
    assert lib.vq_diversity_codes_workspace_bytes(*shape) == 4 * want


def test_layout_cases_cover_one_split_and_several():
    counts = {_documented_floats(*shape, 256)[1] for shape in SIZES}
    assert 1 in counts and max(counts) > 1 and max(counts) <= 64


def test_workspace_size_rejects_what_the_accumulate_sizer_rejects(lib):
    assert lib.vq_diversity_codes_workspace_bytes(1, 96, 256, 64, 3) > 0
    for bad in ((0, 96, 256, 64, 3), (1, 0, 256, 64, 3), (1, 96, 0, 64, 3), (1, 96, 256, 0, 3), (1, 96, 256, 257, 3), (1, 96, 256, 64, 0),
                (1, 96, 256, 64, 5), (1, 1 << 31, 256, 64, 1 << 10), (1, 1 << 24, 256, 256, 1 << 24)):
        assert lib.vq_diversity_workspace_bytes(*bad) == 0 and lib.vq_diversity_codes_workspace_bytes(*bad) == 0, bad
    for ok in SIZES:
        assert lib.vq_diversity_workspace_bytes(*ok) > 0 and lib.vq_diversity_codes_workspace_bytes(*ok) > 0, ok


# ------------------------------------------------------------------------------------------------ dispatch
class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda like a device tensor: the dispatch runs as it would on the GPU, the sweeps are the
    CPU stubs below."""

    @property
    def is_cuda(self):
        return True


def _weights(x, cb, u, metric, temperature, n_positions, pos_div):
    from vector_quantization import search

    dot = metric == search.DOT
    x, cb, u = torch.Tensor(x).double(), torch.Tensor(cb).double(), u[:, :cb.shape[1]].double()
    pos = positions(x.shape[1], n_positions, pos_div)
    s = similarities(x, cb, dot)
    p = (-temperature * s).softmax(-1)
    delta = (p * u[pos]).sum(-1, keepdim=True)
    w = -temperature * p * (u[pos] - delta)
    return x, cb, s, (w if dot else torch.where(s == 0, torch.zeros_like(w), w / s)), dot


class _RowsOnly:
    """The backend as it was before the codes sweep: CPU stubs of the forward and of the rows' backward, recording."""
    calls: list = []

    @classmethod
    def similarities(cls, x, cb, *, metric, out=None):
        from vector_quantization import search

        cls.calls.append("similarities")
        return similarities(x, cb, metric == search.DOT)

    @staticmethod
    def diversity_supported(*shape):
        return True

    @classmethod
    def diversity_table(cls, x, cb, *, metric, temperature, n_positions, pos_div):
        from vector_quantization import search

        cls.calls.append("table")
        x, cb = torch.Tensor(x).double(), torch.Tensor(cb).double()
        z = -temperature * similarities(x, cb, metric == search.DOT)
        pos = positions(x.shape[1], n_positions, pos_div)
        table = torch.zeros((n_positions, cb.shape[1]), dtype=torch.float64).index_add_(0, pos, z.softmax(-1).sum(0))
        return (z.logsumexp(-1) * LOG2E).float(), (table / (x.shape[0] * x.shape[1] // n_positions)).float(), None

    @classmethod
    def diversity_backward(cls, x, cb, lse2, u, *, metric, temperature, n_positions, pos_div, packed=None, live=None, live_packed=None):
        cls.calls.append("backward_x")
        x, cb, s, r, dot = _weights(x, cb, u, metric, temperature, n_positions, pos_div)
        l = cb if live is None else torch.Tensor(live).double()
        return (r @ l if dot else x * r.sum(-1, keepdim=True) - r @ l).float()


class _WithCodes(_RowsOnly):
    calls: list = []

    @staticmethod
    def diversity_codes_supported(*shape):
        return True

    @classmethod
    def diversity_backward_codes(cls, x, cb, lse2, u, *, metric, temperature, n_positions, pos_div, packed=None, need_x=True):
        cls.calls.append(("backward_codes", need_x))
        x, cb, s, r, dot = _weights(x, cb, u, metric, temperature, n_positions, pos_div)
        gx = (r @ cb if dot else x * r.sum(-1, keepdim=True) - r @ cb).float() if need_x else None
        gc = r.transpose(-1, -2) @ x if dot else cb * r.sum(-2).unsqueeze(-1) - r.transpose(-1, -2) @ x
        return gx, gc.float()


def _loss_step(monkeypatch, backend, dot, live=None, x_grad=True):
    from vector_quantization import losses, search

    backend.calls.clear()
    monkeypatch.setattr(search, "_backend", backend)
    x, c = make_inputs(1, 32, 3, 20, 8, dot, 1)
    xd = x.clone().as_subclass(_OnDevice).requires_grad_(x_grad)
    cd = c.clone().requires_grad_(True)
    pos = torch.arange(96) % 3
    loss = losses.codebook_diversity_loss(xd, cd, search.DOT if dot else search.EUCLID, 1.0, lambda: pos, 3, live, pos_div=1)
    (loss * 0.7).backward()
    want = codes_gradient64(x, c, 1.0, 3, 1, dot, g_loss=0.7)
    return list(backend.calls), loss.detach(), xd.grad, cd.grad, want


@pytest.mark.parametrize("dot", [False, True], ids=["euclid", "dot"])
def test_learnable_codebook_takes_the_fused_path(monkeypatch, dot):
    calls, loss, gx, gc, want = _loss_step(monkeypatch, _WithCodes, dot)
    assert calls == ["table", ("backward_codes", True)]  # one method serves both gradients: delta is computed once
    torch.testing.assert_close(loss.double(), want["loss"], rtol=1e-5, atol=0)
    torch.testing.assert_close(torch.Tensor(gx).double(), want["gx"], rtol=1e-4, atol=1e-5 * float(want["gx"].abs().max()))
    torch.testing.assert_close(gc.double(), want["gc"], rtol=1e-4, atol=1e-5 * float(want["gc"].abs().max()))
    # only the codes need a gradient: the rows' sweep is not asked for
    calls, _, gx, gc, want = _loss_step(monkeypatch, _WithCodes, dot, x_grad=False)
    assert calls == ["table", ("backward_codes", False)] and gx is None
    torch.testing.assert_close(gc.double(), want["gc"], rtol=1e-4, atol=1e-5 * float(want["gc"].abs().max()))


def test_live_codes_or_an_older_backend_keep_the_chunked_path(monkeypatch):
    from vector_quantization import losses

    # codes that are rewritten before backward (an EMA codebook whose codes require grad for the orthogonal loss)
    live = make_inputs(1, 32, 3, 20, 8, False, 1)[1] + 0.05
    calls, loss, gx, gc, want = _loss_step(monkeypatch, _WithCodes, False, live=live)
    assert calls and set(calls) == {"similarities"}
    assert gc is not None and abs(float(loss) - float(want["loss"])) < 1e-5 * abs(float(want["loss"]))
    # a backend without the codes sweep
    calls, loss, gx, gc, want = _loss_step(monkeypatch, _RowsOnly, False)
    assert calls and set(calls) == {"similarities"}
    torch.testing.assert_close(gc.double(), want["gc"], rtol=1e-4, atol=1e-5 * float(want["gc"].abs().max()))
    # ... which still runs fused for a codebook that needs no gradient, as before
    x, c = make_inputs(1, 32, 3, 20, 8, False, 1)
    xd = x.as_subclass(_OnDevice)
    assert losses._diversity_fused_backend(xd, c, 3, 1) is _RowsOnly
    assert losses._diversity_fused_backend(xd, c, 3, 1, live) is _RowsOnly
    assert losses._diversity_fused_backend(xd, c.clone().requires_grad_(True), 3, 1) is None


def test_row_cut_of_a_learnable_codebook_is_a_pure_function_of_the_shape(monkeypatch):
    from vector_quantization import losses, search

    cuts = losses.DIVERSITY_CODES_FUSED_MIN_ROWS
    assert sorted(cuts) == [32, 64, 128, 256] and all(losses.DIVERSITY_FUSED_MIN_ROWS <= c <= 32 for c in cuts.values())
    assert [cuts[dp] for dp in sorted(cuts)] == sorted(cuts.values()), "wider rows never run fused from fewer rows on"
    for d, dp in ((1, 32), (32, 32), (33, 64), (64, 64), (100, 128), (129, 256), (256, 256)):
        for rows in range(1, 40):
            assert losses.diversity_codes_runs_fused(rows, 1, d) == (rows >= cuts[dp]), (d, rows)
            assert losses.diversity_codes_runs_fused(2 * rows + 1, 2, d) == (rows >= cuts[dp])  # the rows of ONE head are padded
    assert not losses.diversity_codes_runs_fused(31, 1, 257) and losses.diversity_codes_runs_fused(32, 1, 64)
    # the dispatch asks it only for codes that require grad: the cut of a codebook without a gradient does not move
    monkeypatch.setattr(search, "_backend", _WithCodes)
    rows = losses.DIVERSITY_FUSED_MIN_ROWS
    assert rows < cuts[64]
    x, c = torch.zeros((1, rows * 3, 64)).as_subclass(_OnDevice), torch.zeros((1, 20, 64))
    assert losses._diversity_fused_backend(x, c, 3, 1) is _WithCodes
    assert losses._diversity_fused_backend(x, c.clone().requires_grad_(True), 3, 1) is None
    x = torch.zeros((1, cuts[64] * 3, 64)).as_subclass(_OnDevice)
    assert losses._diversity_fused_backend(x, c.clone().requires_grad_(True), 3, 1) is _WithCodes


def test_other_fallback_conditions_hold_for_a_learnable_codebook(monkeypatch):
    from vector_quantization import losses, search

    monkeypatch.setattr(search, "_backend", _WithCodes)
    x, c = make_inputs(1, 32, 3, 20, 8, False, 1)
    xd, cd = x.as_subclass(_OnDevice), c.clone().requires_grad_(True)
    assert losses._diversity_fused_backend(xd, cd, 3, 1) is _WithCodes
    assert losses._diversity_fused_backend(x, cd, 3, 1) is None  # CPU tensors
    assert losses._diversity_fused_backend(xd, cd, 3, None) is None  # no position rule
    monkeypatch.setenv("VQ_DIVERSITY_NO_FUSED", "1")
    assert losses._diversity_fused_backend(xd, cd, 3, 1) is None
    monkeypatch.delenv("VQ_DIVERSITY_NO_FUSED")

    class Narrow(_WithCodes):  # the shape is one the codes sweep does not take (D > 256)
        @staticmethod
        def diversity_codes_supported(*shape):
            return False

    monkeypatch.setattr(search, "_backend", Narrow)
    assert losses._diversity_fused_backend(xd, cd, 3, 1) is None
    assert losses._diversity_fused_backend(xd, c, 3, 1) is Narrow
    with torch.no_grad():  # nothing to differentiate: codes that require grad do not matter
        assert losses._diversity_fused_backend(xd, cd, 3, 1) is Narrow
