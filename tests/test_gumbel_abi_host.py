"""Host checks of the seven Gumbel backward entries of the C ABI (vq_gumbel_*_f32, vq_gumbel_reinmax_*_f32): the return
code and one keyword of vq_last_error() for every argument fault, pinned entry by entry.  Every case returns before a kernel
launch or a memset, the pointers are fake (aligned integers that nothing dereferences), so no GPU is needed.

Where the two families differ (observed, and kept as it is):
  * tau = +inf: the straight-through entries accept it (the call goes on to the next check), the reinmax entries reject it;
  * M == 0: the straight-through stats / backward_x return 0 before they look at anything else; the reinmax entries check g,
    tau, D and their own pointers (ind / grad_x / grad_codes) first and only then return 0 -- the statistics arrays, cb and the
    workspace of an empty call are never looked at; vq_gumbel_backward_codes checks grad_codes AND cb before M == 0;
  * order: the straight-through entries report a null statistics array together with a null g, before tau and D; the reinmax
    entries report it with the alignment, after tau and D (so a null array at D = 257 is BADARG there, UNSUPPORTED here);
  * a misaligned array is "16-byte aligned" in both, a null one "null argument" (straight-through) or "null or not 16-byte
    aligned" (reinmax).
"""
from __future__ import annotations

import ctypes

import pytest

BADARG, UNSUPPORTED = -1, -2
H, M, K, D = 2, 33, 7, 5
P = 0x10000  # fake pointers: P + 256 * i, all 16-byte aligned
INF, NAN = float("inf"), float("nan")


def _args(**over):
    """vq_args of a valid call without the packed codebook: an entry that takes a->packed ends at 'packed codebook is
    null', the last check before its launch."""
    from vector_quantization import native

    a = native.VqArgs()
    a.H, a.Q, a.M, a.K, a.D, a.metric, a.flags = H, 1, M, K, D, 0, 0
    a.x, a.x_rs, a.x_hs = P, D, M * D
    a.cb, a.cb_hs, a.cb_qs = P + 256, K * D, 0
    for name, value in over.items():
        setattr(a, name, value)
    return a


# entry -> (family, the names of its arguments after (a, g, g_rs, g_hs, tau) and before the stream, its statistics arrays)
ENTRIES = {
    "vq_gumbel_stats_f32": ("st", ("lse2", "delta"), ("lse2", "delta")),
    "vq_gumbel_backward_x_f32": ("st", ("lse2", "delta", "grad_x", "gx_rs", "gx_hs"), ("lse2", "delta")),
    "vq_gumbel_backward_codes_f32": ("st", ("lse2", "delta", "grad_codes", "workspace", "workspace_bytes"), ("lse2", "delta")),
    "vq_gumbel_reinmax_stats_f32": ("rm", ("lse2_tau", "lse2_one", "delta0"), ("lse2_tau", "lse2_one", "delta0")),
    "vq_gumbel_reinmax_columns_f32": ("rm", ("lse2_tau", "ind", "ind_rs", "ind_hs", "col", "e", "workspace", "workspace_bytes"),
                                      ("lse2_tau", "col", "e")),
    "vq_gumbel_reinmax_backward_x_f32": ("rm", ("lse2_tau", "lse2_one", "delta0", "ind", "ind_rs", "ind_hs", "col", "e", "grad_x",
                                                "gx_rs", "gx_hs"), ("lse2_tau", "lse2_one", "delta0", "col", "e")),
    "vq_gumbel_reinmax_backward_codes_f32": ("rm", ("lse2_tau", "lse2_one", "delta0", "col", "e", "grad_codes", "workspace",
                                                    "workspace_bytes"), ("lse2_tau", "lse2_one", "delta0", "col", "e")),
}
CODES = ("vq_gumbel_backward_codes_f32", "vq_gumbel_reinmax_columns_f32", "vq_gumbel_reinmax_backward_codes_f32")
OWN_POINTERS = ("ind", "grad_x", "grad_codes")
STRIDES = {"gx_rs": D, "gx_hs": M * D, "ind_rs": 1, "ind_hs": M}


def _call(entry, a=None, **over):
    """One call of `entry` with valid fake arguments except what `over` replaces (a: the vq_args, None = _args()).  The
    workspace of a codes-resident entry is NULL unless given, so a call that passes every other check ends at 'workspace'.
    -> (return code, vq_last_error())."""
    from vector_quantization import native

    lib = native.load()
    values = {"g": P + 512, "g_rs": D, "g_hs": M * D, "tau": 1.0, "workspace": None, "workspace_bytes": 0, **STRIDES}
    for i, name in enumerate(ENTRIES[entry][1]):
        values.setdefault(name, P + 1024 + 256 * i)
    values.update(over)
    a = _args() if a is None else a
    argv = [None if a is False else ctypes.byref(a)] + [values[n] for n in ("g", "g_rs", "g_hs", "tau") + ENTRIES[entry][1]] + [None]
    rc = getattr(lib, entry)(*argv)
    return rc, lib.vq_last_error().decode()


def _expect(got, rc, keyword):
    assert got[0] == rc and (rc == 0 or keyword in got[1]), (got, rc, keyword)


def _end(entry):
    """Where a call with no fault ends here: the rows-resident entries at the missing packed codebook, the codes-resident
    ones at the missing workspace."""
    return (BADARG, "workspace") if entry in CODES else (BADARG, "packed codebook is null")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_call_without_a_fault_reaches_the_last_check(entry):
    _expect(_call(entry), *_end(entry))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_args_and_null_g(entry):
    family = ENTRIES[entry][0]
    _expect(_call(entry, a=False), BADARG, "null args")
    _expect(_call(entry, g=None), BADARG, "null argument (g / lse2 / delta)" if family == "st" else "g is null")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_tau(entry):
    for tau in (0.0, -1.0, NAN, -INF):
        _expect(_call(entry, tau=tau), BADARG, "tau must be positive")
    if ENTRIES[entry][0] == "st":  # +inf passes the straight-through check: the call goes on to its last check
        _expect(_call(entry, tau=INF), *_end(entry))
    else:
        _expect(_call(entry, tau=INF), BADARG, "tau must be positive and finite")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_rows_wider_than_256(entry):
    _expect(_call(entry, a=_args(D=257)), UNSUPPORTED, "D > 256")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_statistics_arrays(entry):
    family, _, stats = ENTRIES[entry]
    for name in stats:
        _expect(_call(entry, **{name: None}), BADARG, "null argument" if family == "st" else "statistics array is null or not")
        _expect(_call(entry, **{name: P + 4096 + 4}), BADARG, "16-byte aligned")
        # the order of the checks: a null array comes before tau and D (straight-through) or after them (reinmax)
        _expect(_call(entry, tau=0.0, **{name: None}), BADARG, "null argument" if family == "st" else "tau")
        if family == "st":
            _expect(_call(entry, a=_args(D=257), **{name: None}), BADARG, "null argument")
        else:
            _expect(_call(entry, a=_args(D=257), **{name: None}), UNSUPPORTED, "D > 256")
    _expect(_call(entry, a=_args(D=257), **{stats[0]: P + 4096 + 4}), UNSUPPORTED, "D > 256")  # alignment: after D in both


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_own_pointers(entry):
    want = {
        ("vq_gumbel_backward_x_f32", "grad_x"): "grad_x is null",
        ("vq_gumbel_backward_codes_f32", "grad_codes"): "null argument (grad_codes / cb)",
        ("vq_gumbel_reinmax_columns_f32", "ind"): "ind is null",
        ("vq_gumbel_reinmax_backward_x_f32", "ind"): "null argument (ind / grad_x)",
        ("vq_gumbel_reinmax_backward_x_f32", "grad_x"): "null argument (ind / grad_x)",
        ("vq_gumbel_reinmax_backward_codes_f32", "grad_codes"): "grad_codes is null",
    }
    names = [n for n in ENTRIES[entry][1] if n in OWN_POINTERS]
    assert sorted((entry, n) for n in names) == sorted(k for k in want if k[0] == entry)
    for name in names:
        _expect(_call(entry, **{name: None}), BADARG, want[(entry, name)])


@pytest.mark.parametrize("entry", CODES)
def test_codes_resident_natural_codebook_and_row_count(entry):
    _expect(_call(entry, a=_args(cb=None)), BADARG, "null argument (grad_codes / cb)" if ENTRIES[entry][0] == "st" else "cb is null")
    _expect(_call(entry, a=_args(M=2 ** 31, x_hs=2 ** 31 * D), g_hs=2 ** 31 * D), UNSUPPORTED, "too many rows")


@pytest.mark.parametrize("entry", CODES)
def test_codes_resident_workspace(entry):
    from vector_quantization import native

    lib = native.load()
    sizer = lib.vq_gumbel_workspace_bytes if ENTRIES[entry][0] == "st" else lib.vq_gumbel_reinmax_workspace_bytes
    need = int(sizer(H, M, K, D))
    assert need > 0 and need % 4 == 0
    ws = P + (1 << 20)
    _expect(_call(entry, workspace=None, workspace_bytes=need), BADARG, "workspace too small or misaligned")
    _expect(_call(entry, workspace=ws + 4, workspace_bytes=need + 64), BADARG, "workspace too small or misaligned")
    _expect(_call(entry, workspace=ws, workspace_bytes=need - 1), BADARG, "workspace too small or misaligned")
    _expect(_call(entry, workspace=ws, workspace_bytes=0), BADARG, "workspace too small or misaligned")
    assert ("vq_gumbel_workspace_bytes" if ENTRIES[entry][0] == "st" else "vq_gumbel_reinmax_workspace_bytes") in \
        _call(entry, workspace=ws, workspace_bytes=need - 1)[1]


def test_empty_call_straight_through_rows():
    """M == 0: vq_gumbel_stats / vq_gumbel_backward_x return 0 before any other check (only vq_args itself is checked)."""
    bad = dict(g=None, tau=NAN, lse2=None, delta=P + 4)
    empty = dict(M=0, x=None)
    _expect(_call("vq_gumbel_stats_f32", a=_args(**empty), **bad), 0, "")
    _expect(_call("vq_gumbel_backward_x_f32", a=_args(**empty), grad_x=None, **bad), 0, "")
    _expect(_call("vq_gumbel_stats_f32", a=_args(D=257, **empty), **bad), 0, "")
    _expect(_call("vq_gumbel_stats_f32", a=_args(K=0, **empty), **bad), BADARG, "non-positive")


def test_empty_call_straight_through_codes():
    """M == 0: vq_gumbel_backward_codes checks grad_codes and cb first (then it clears grad_codes: the GPU suite)."""
    entry = "vq_gumbel_backward_codes_f32"
    _expect(_call(entry, a=_args(M=0, x=None), grad_codes=None), BADARG, "null argument (grad_codes / cb)")
    _expect(_call(entry, a=_args(M=0, x=None, cb=None)), BADARG, "null argument (grad_codes / cb)")


@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e][0] == "rm"])
def test_empty_call_reinmax(entry):
    """M == 0: the reinmax entries still check g, tau, D and their own pointers; the statistics arrays (null or misaligned),
    cb and the workspace are not looked at.  (vq_gumbel_reinmax_backward_codes then clears grad_codes: the GPU suite.)"""
    empty = dict(M=0, x=None, cb=None)
    stats = {name: (None if i % 2 else P + 4) for i, name in enumerate(ENTRIES[entry][2])}
    _expect(_call(entry, a=_args(**empty), g=None, **stats), BADARG, "g is null")
    _expect(_call(entry, a=_args(**empty), tau=INF, **stats), BADARG, "tau must be positive and finite")
    _expect(_call(entry, a=_args(D=257, **empty), **stats), UNSUPPORTED, "D > 256")
    for name in (n for n in ENTRIES[entry][1] if n in OWN_POINTERS):
        _expect(_call(entry, a=_args(**empty), **{name: None}, **stats), BADARG, "null")
    if entry != "vq_gumbel_reinmax_backward_codes_f32":
        _expect(_call(entry, a=_args(**empty), **stats), 0, "")
