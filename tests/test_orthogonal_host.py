"""Host side of the fused orthogonal regularisation loss (no GPU): the yardstick of tests/test_gpu_orthogonal.py itself -- the
fp64 closed form against fp64 autograd of the reference's formula --, the C ABI's symbol and argument rules, and the dispatch
of losses.orthogonal_loss with a recording backend."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from orthogonal_run import closed_form64, make_codes, reference_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "vq_orthogonal_gram_f32"
E_BADARG, E_UNSUPPORTED = -1, -2
P = 0x4000  # a non-null, 16-byte aligned address
DOT = 1
CUT_ONE = {32: {1: 1}, 64: {1: 1}, 128: {1: 1}, 256: {1: 1}}


@pytest.fixture(scope="module")
def lib():
    from vector_quantization import native

    return native.load()


# ------------------------------------------------------------------------------------------------ the yardstick itself
def _special_codes():
    codes = make_codes(2, 60, 24, 7)
    codes[0, 3:8] = 0.0  # five zero rows
    codes[1, 11] = 0.0
    codes[0, 40] = codes[0, 13]  # a duplicated row
    return codes


def _orthonormal():
    q, _ = torch.linalg.qr(make_codes(1, 32, 32, 9)[0].double())
    return q[None, :20].float() * 3.0  # 20 orthogonal rows of 32 dims, norm 3


CODES = {
    "n33": lambda: make_codes(1, 33, 8, 1),
    "h2": lambda: make_codes(2, 100, 32, 2),
    "d200": lambda: make_codes(3, 40, 200, 3),
    "one": lambda: make_codes(1, 1, 8, 4),
    "zero_and_duplicate": _special_codes,
    "orthonormal": _orthonormal,
}


@pytest.mark.parametrize("name", list(CODES))
def test_closed_form_is_autograd_of_the_reference_formula(name):
    codes = CODES[name]()
    got = closed_form64(codes)
    ref = reference_sequence(codes, torch.float64)
    if name == "orthonormal":  # loss = 0 up to rounding: nothing relative to compare
        assert abs(float(got["loss"])) < 1e-15 and abs(float(ref["loss"])) < 1e-15
    else:
        torch.testing.assert_close(got["loss"], ref["loss"], rtol=1e-12, atol=0)
    n = codes.shape[1]
    torch.testing.assert_close(got["loss"] + 1 / n, ref["loss"] + 1 / n, rtol=1e-12, atol=0)  # (the sum itself)
    torch.testing.assert_close(got["grad"], ref["grad"], rtol=1e-9, atol=1e-12 * got["grad_scale"])
    torch.testing.assert_close(got["rowsq"], ref["rowsq"], rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(got["G"], ref["G"], rtol=1e-9, atol=1e-12 * float(ref["G"].abs().max()))
    if name == "zero_and_duplicate":
        assert not bool(got["rowsq"][0, 3:8].any()) and not bool(got["G"][0, 3:8].any()) and not bool(got["grad"][0, 3:8].any())
    if name == "one":  # cos = [[1]]: loss = 1 - 1 = 0, and the normalisation removes the radial gradient
        assert float(got["loss"]) == 0.0 and float(got["grad"].abs().max()) < 1e-15 * got["grad_scale"]


# ------------------------------------------------------------------------------------------------ symbols, arguments
def test_symbol_declared_listed_and_exported(lib):
    from vector_quantization import native, search

    header = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    assert re.search(rf"\b{ENTRY}\s*\(", header), f"{ENTRY} is not declared in vq_mi355x.h"
    assert ENTRY in native.EXPORTED_SYMBOLS and ENTRY in native._SIGNATURES
    assert hasattr(lib, ENTRY)
    assert callable(native.orthogonal_gram) and callable(search._NativeBackend.orthogonal_gram)


def _args(native, n=40, D=16, H=1, metric=DOT):
    """vq_args with fake (never dereferenced: every call below fails validation before a launch) 16-byte aligned pointers."""
    a = native.VqArgs()
    a.H, a.Q, a.M, a.K, a.D, a.metric = H, 1, n, n, D, metric
    a.x, a.x_rs, a.x_hs = 0x1000, D, n * D
    a.packed, a.pk_hs = 0x3000, 0
    return a


def _call(lib, a, rowsq=P, gram=P, g_rs=16, g_hs=0):
    return lib.vq_orthogonal_gram_f32(ctypes.byref(a), rowsq, gram, g_rs, g_hs, None)


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """Fake pointers throughout: every call fails validation before anything is dereferenced or launched."""
    from vector_quantization import native

    assert lib.vq_orthogonal_gram_f32(None, P, P, 16, 0, None) == E_BADARG
    a = _args(native)
    assert _call(lib, a, rowsq=None) == E_BADARG and b"rowsq" in lib.vq_last_error()
    assert _call(lib, a, rowsq=P + 4) == E_BADARG and b"rowsq" in lib.vq_last_error() and b"16-byte" in lib.vq_last_error()
    assert _call(lib, a, gram=P + 8) == E_BADARG and b"gram" in lib.vq_last_error() and b"16-byte" in lib.vq_last_error()
    for kw in (dict(H=0), dict(H=-1), dict(n=0), dict(n=-5), dict(D=0), dict(D=-2)):
        assert _call(lib, _args(native, **kw)) == E_BADARG, kw
        assert b"must be positive" in lib.vq_last_error(), kw
    assert _call(lib, _args(native, metric=0)) == E_BADARG and b"metric" in lib.vq_last_error()
    assert _call(lib, _args(native, metric=7)) == E_BADARG and b"metric" in lib.vq_last_error()
    b = _args(native)
    b.packed = None
    assert _call(lib, b) == E_BADARG and b"packed" in lib.vq_last_error()
    b = _args(native)
    b.x = None
    assert _call(lib, b) == E_BADARG and b"x is null" in lib.vq_last_error()
    assert _call(lib, _args(native, D=257)) == E_UNSUPPORTED and b"D > 256" in lib.vq_last_error()
    # (a null gram is legal -- rowsq only -- so it is rejected on other grounds alone)
    assert _call(lib, _args(native, D=257), gram=None) == E_UNSUPPORTED
    for msg in (b"vq_orthogonal_gram",):
        assert msg in lib.vq_last_error()


# ------------------------------------------------------------------------------------------------ dispatch
class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda like a device tensor: the dispatch runs as it would on the GPU, the sweep is the CPU
    stub below."""

    @property
    def is_cuda(self):
        return True


class _Recording:
    """orthogonal_gram from the fp64 closed form, recording (n, d, want_g) of every call."""
    calls: list = []

    @classmethod
    def orthogonal_gram(cls, x, *, want_g=True):
        from orthogonal_run import gram64

        cls.calls.append((x.shape[1], x.shape[2], want_g))
        assert not x.requires_grad
        rowsq, G = gram64(torch.Tensor(x))
        return rowsq.float(), (G.float() if want_g else None)


class _Older:
    """A backend from before the sweep."""


def _loss(monkeypatch, codes, backend=_Recording, cut=CUT_ONE, on_device=True, grad=True, upstream=0.7):
    from vector_quantization import losses, search

    _Recording.calls.clear()
    monkeypatch.setattr(search, "_backend", backend)
    monkeypatch.setattr(losses, "ORTHOGONAL_FUSED_MIN_CODES", dict(cut))
    leaf = codes.clone()
    if on_device:
        leaf = leaf.as_subclass(_OnDevice)
    leaf.requires_grad_(grad)
    loss = losses.orthogonal_loss(leaf)
    if grad:
        (loss * upstream).backward()
    return list(_Recording.calls), loss.detach(), (torch.Tensor(leaf.grad) if grad else None)


def test_cpu_codes_never_call_the_backend(monkeypatch):
    codes = make_codes(2, 50, 16, 5)
    calls, loss, grad = _loss(monkeypatch, codes, on_device=False)
    assert calls == []
    want = closed_form64(codes)
    torch.testing.assert_close(loss.double(), want["loss"], rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(grad.double(), 0.7 * want["grad"], rtol=1e-4, atol=1e-5 * float(want["grad"].abs().max()))


def test_fused_path_and_its_backward(monkeypatch):
    """The backward is 4 * G * upstream (times the 1 / (h n^2) that stays in autograd, through F.normalize): with a backend that
    returns the fp64 closed form, loss and gradient are the closed form's."""
    codes = make_codes(2, 50, 16, 5)
    calls, loss, grad = _loss(monkeypatch, codes)
    assert calls == [(50, 16, True)]
    want = closed_form64(codes)
    torch.testing.assert_close(loss.double(), want["loss"], rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(grad.double(), 0.7 * want["grad"], rtol=1e-4, atol=1e-5 * float(want["grad"].abs().max()))


def test_function_backward_is_four_g_times_upstream(monkeypatch):
    from vector_quantization import losses

    normed = F.normalize(make_codes(1, 20, 8, 6), dim=-1).requires_grad_(True)
    _Recording.calls.clear()
    total = losses._OrthogonalFn.apply(normed, _Recording)
    (total * -1.5).backward()
    rowsq, G = _Recording.orthogonal_gram(normed.detach())
    assert total.dtype == torch.float32 and total.dim() == 0
    torch.testing.assert_close(total, rowsq.sum(dtype=torch.float64).float(), rtol=0, atol=0)
    torch.testing.assert_close(normed.grad, -1.5 * 4 * G, rtol=1e-6, atol=0)


def test_the_cut_is_respected(monkeypatch):
    cut = {32: {1: 40}, 64: {1: 10}, 128: {}, 256: {1: 30, 3: 12}}
    assert _loss(monkeypatch, make_codes(1, 39, 32, 1), cut=cut)[0] == []
    assert _loss(monkeypatch, make_codes(1, 40, 32, 1), cut=cut)[0] == [(40, 32, True)]
    assert _loss(monkeypatch, make_codes(1, 39, 33, 1), cut=cut)[0] == [(39, 33, True)]  # (padded width 64: its own cut)
    assert _loss(monkeypatch, make_codes(1, 9, 64, 1), cut=cut)[0] == []
    assert _loss(monkeypatch, make_codes(1, 500, 100, 1), cut=cut)[0] == []  # (no entry: the width keeps the GEMM)
    assert _loss(monkeypatch, make_codes(1, 30, 129, 1), cut=cut)[0] == [(30, 129, True)]
    assert _loss(monkeypatch, make_codes(1, 29, 256, 1), cut=cut)[0] == []
    # the cut of the listed head counts <= h: two heads take the one-head cut, three and more the lower one
    assert _loss(monkeypatch, make_codes(2, 29, 256, 1), cut=cut)[0] == []
    assert _loss(monkeypatch, make_codes(3, 12, 256, 1), cut=cut)[0] == [(12, 256, True)]
    assert _loss(monkeypatch, make_codes(5, 11, 256, 1), cut=cut)[0] == []


def test_default_cut_is_a_table_per_padded_width_and_head_count():
    from vector_quantization import losses

    assert sorted(losses.ORTHOGONAL_FUSED_MIN_CODES) == [32, 64, 128, 256]
    for by_heads in losses.ORTHOGONAL_FUSED_MIN_CODES.values():
        assert all(isinstance(hh, int) and hh >= 1 and isinstance(c, int) and c >= 1 for hh, c in by_heads.items())
    # the measured table: one codebook of 8 192 wide codes keeps the GEMM, eight of them run fused; narrow codes from 256 on
    assert not losses.orthogonal_runs_fused(8192, 128) and not losses.orthogonal_runs_fused(8192, 256, 7)
    assert losses.orthogonal_runs_fused(8192, 128, 8) and losses.orthogonal_runs_fused(8192, 256, 8)
    assert losses.orthogonal_runs_fused(16384, 256) and losses.orthogonal_runs_fused(256, 64) and not losses.orthogonal_runs_fused(255, 32)
    assert not losses.orthogonal_runs_fused(1 << 20, 257)


def test_switch_width_dtype_and_older_backends_keep_the_gemm(monkeypatch):
    codes = make_codes(1, 40, 16, 2)
    monkeypatch.setenv("VQ_ORTHOGONAL_NO_FUSED", "1")
    assert _loss(monkeypatch, codes)[0] == []
    monkeypatch.delenv("VQ_ORTHOGONAL_NO_FUSED")
    assert _loss(monkeypatch, codes)[0] == [(40, 16, True)]  # (read per call)
    assert _loss(monkeypatch, make_codes(1, 12, 257, 2))[0] == []
    assert _loss(monkeypatch, make_codes(1, 12, 256, 2))[0] == [(12, 256, True)]
    assert _loss(monkeypatch, codes.double())[0] == []
    calls, loss, grad = _loss(monkeypatch, codes, backend=_Older)
    assert calls == [] and grad is not None
    torch.testing.assert_close(loss.double(), closed_form64(codes)["loss"], rtol=1e-5, atol=1e-8)


def test_no_gradient_no_gram(monkeypatch):
    codes = make_codes(1, 40, 16, 2)
    calls, loss, _ = _loss(monkeypatch, codes, grad=False)  # codes that do not require grad
    assert calls == [(40, 16, False)]
    torch.testing.assert_close(loss.double(), closed_form64(codes)["loss"], rtol=1e-5, atol=1e-8)
    from vector_quantization import losses, search

    monkeypatch.setattr(search, "_backend", _Recording)
    monkeypatch.setattr(losses, "ORTHOGONAL_FUSED_MIN_CODES", dict(CUT_ONE))
    _Recording.calls.clear()
    with torch.no_grad():
        losses.orthogonal_loss(codes.clone().as_subclass(_OnDevice).requires_grad_(True))
    assert _Recording.calls == [(40, 16, False)]
