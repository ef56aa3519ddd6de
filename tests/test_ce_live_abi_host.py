"""Host checks of vq_ce_backward_live_f32 (the cross-entropy backward with live codes): the symbol, the return code and the
start of vq_last_error() for every argument fault.  Every case returns before a kernel launch, the pointers are fake (aligned
integers that nothing dereferences), so no GPU is needed.

Order of the checks: vq_args itself, the live pair, the arrays of vq_ce_backward_f32, a->packed (the searched codes), D, and
only then M == 0.  a->cb is not read by this entry (the finalize takes the target's row from live_cb).
"""
from __future__ import annotations

import ctypes

import pytest

ENTRY = "vq_ce_backward_live_f32"
BADARG, UNSUPPORTED = -1, -2
H, M, K, D = 2, 33, 7, 5
P = 0x10000  # fake pointers: P + 256 * i, all 16-byte aligned
# the arguments after vq_args and before the stream, in the order of the prototype
NAMES = ("live_cb", "live_cb_hs", "live_packed", "live_pk_hs", "lse", "target_logit", "target", "tgt_rs", "tgt_hs", "coef", "grad_x",
         "gx_rs", "gx_hs")
POINTERS = ("live_cb", "live_packed", "lse", "target_logit", "target", "coef", "grad_x")


def _args(**over):
    from vector_quantization import native

    a = native.VqArgs()
    a.H, a.Q, a.M, a.K, a.D, a.metric, a.flags = H, 1, M, K, D, 0, 0
    a.x, a.x_rs, a.x_hs = P, D, M * D
    a.cb, a.cb_hs, a.cb_qs = P + 256, K * D, 0
    a.packed, a.pk_hs, a.pk_qs = P + 512, 1024, 0
    for name, value in over.items():
        setattr(a, name, value)
    return a


def _call(a=None, **over):
    """One call with valid fake arguments except what `over` replaces.  -> (return code, vq_last_error())."""
    from vector_quantization import native

    lib = native.load()
    values = {"live_cb_hs": K * D, "live_pk_hs": 1024, "tgt_rs": 1, "tgt_hs": M, "gx_rs": D, "gx_hs": M * D}
    for i, name in enumerate(POINTERS):
        values[name] = P + 4096 + 256 * i
    values.update(over)
    a = _args() if a is None else a
    rc = getattr(lib, ENTRY)(None if a is False else ctypes.byref(a), *[values[n] for n in NAMES], None)
    return rc, lib.vq_last_error().decode()


def _expect(got, rc, start):
    assert got[0] == rc and (rc == 0 or got[1].startswith(start)), (got, rc, start)


def test_symbol_is_exported():
    from vector_quantization import native

    assert ENTRY in native.EXPORTED_SYMBOLS
    assert hasattr(native.load(), ENTRY)


def test_null_args():
    _expect(_call(a=False), BADARG, "vq: null args")


@pytest.mark.parametrize("name", POINTERS)
def test_each_null_argument(name):
    got = _call(**{name: None})
    _expect(got, BADARG, "vq_ce_backward_live: null argument")
    assert name in got[1]


def test_null_searched_image():
    _expect(_call(a=_args(packed=None)), BADARG, "vq_ce_backward_live: packed codebook is null")


def test_natural_searched_codebook_is_not_needed():
    """a->cb is not read: a call without it passes every check (shown on the empty call, which returns after them)."""
    _expect(_call(a=_args(cb=None, M=0, x=None)), 0, "")


@pytest.mark.parametrize("d", [257, 600])
def test_rows_wider_than_256(d):
    _expect(_call(a=_args(D=d)), UNSUPPORTED, "vq_ce_backward_live: D > 256")
    _expect(_call(a=_args(D=d, M=0, x=None)), UNSUPPORTED, "vq_ce_backward_live: D > 256")  # M == 0 comes after the checks
    _expect(_call(a=_args(D=d), live_packed=None), BADARG, "vq_ce_backward_live: null argument")  # null comes before D


def test_empty_call():
    _expect(_call(a=_args(M=0, x=None)), 0, "")
    _expect(_call(a=_args(M=0, x=None, D=256)), 0, "")
    _expect(_call(a=_args(M=0, x=None), grad_x=None), BADARG, "vq_ce_backward_live: null argument")
    _expect(_call(a=_args(M=0, x=None, K=0)), BADARG, "vq: non-positive size")


def test_same_images_are_legal_arguments():
    """live_cb == a->cb with live_packed == a->packed passes the checks (the result is the non-live one: the GPU suite)."""
    a = _args(M=0, x=None)
    _expect(_call(a=a, live_cb=a.cb, live_packed=a.packed), 0, "")
