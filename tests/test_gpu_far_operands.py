"""GPU: every native call with one operand whose rows span more than 2^31 elements (tests/input_poison.FarPlacer), over the
table of cases the two poison suites share (tests/native_cases.py).

Every entry of the C ABI takes its row, head, stage and group strides as ``long long``; a kernel that forms ``row * stride`` in
an ``int`` or ``unsigned`` passes every other test, whose operands are a few MiB long.  Here each case runs
  once             with everything placed plainly: the baseline outputs, and the count n of its far-able placements (every
                   ``place(..., role="rows")`` of a non-empty tensor, every ``dest(...)``);
  once per k < n   with the k-th of those placements far (input_poison.far_layout: the payload stays tiny, only the strides
                   grow) inside ONE arena of FAR_ARENA_BYTES filled with the NaN pattern, everything else plain.
After a far run every output equals the baseline bit for bit over its defined extent (alloc_poison.defined_mask; the far
layout keeps every row's address class modulo 16, so the launch plan and the load path are the baseline's and there is no
LOAD_PATH_SUMS exception), and once the far operand's own elements are overwritten with the poison, every byte a 32-bit
truncated or wrapped offset could have reached (input_poison.far_reach_bytes: the guard bands, the gap rows and all that lies
between the rows included) holds the poison.  The arena is refilled over that reach before every run.

The far pointer must reach a kernel: native._call, the one helper every ctypes call goes through, is wrapped for the
duration of a run, and an address inside the arena must be among the arguments of at least one call.  An operand for which
that does not hold (the wrapper copies it), or that has no axis to stride (one row and one head), stands in FAR_EXEMPT.
"""
from __future__ import annotations

import ctypes
import fnmatch
import time

import pytest
import torch

import input_poison as ip
import native_cases as nc
from native_cases import DEV, TABLE, Case, _native
from test_gpu_input_extents import _compare, _run

pytestmark = pytest.mark.gpu

# What the wrappers allocate beside the arena in a far run: quantize lays ``best`` out with the strides of idx, four heads of
# 2^31 floats when a four-head idx destination is the far operand.
HEADROOM_BYTES = 40 << 30

NO_AXIS = "one row and one head: no axis to stride"
# "case pattern:operand" (rows<i> / dest<i>: the i-th far-able input / destination of the case, in call order) -> NO_AXIS, or
# the line of native.py ("function: text") because of which the operand's far address reaches no kernel.
FAR_EXEMPT: dict[str, str] = {
    "keys-one-row:rows0": NO_AXIS,  # x [1, 1, 20]
    # the target [1, 50] of rows wider than 512 dims: torch takes the logits of each row chunk, no kernel of the library reads it
    "softmax_stats-wide-rows:rows1": "_softmax_stats_wide: picked = torch.gather(logits, 2, t.clamp(0, K - 1)[..., None])[..., 0]",
    "fsq_quantize-backward-decode:rows2": "fsq_decode: indices = indices.contiguous()",  # the indices [N, Q] of the decode
}

# case name -> {operand label: (dtype, "far" | "exempt")}
DONE: dict[str, dict[str, tuple]] = {}
SECONDS: dict[str, float] = {}


@pytest.fixture(scope="module")
def arena():
    free, _ = torch.cuda.mem_get_info()
    need = ip.FAR_ARENA_BYTES + HEADROOM_BYTES
    if free < need:
        pytest.skip(f"less free device memory than the arena plus {HEADROOM_BYTES >> 30} GiB ({free} < {need} bytes)")
    box = {"arena": torch.empty(ip.FAR_ARENA_BYTES, dtype=torch.uint8, device=DEV)}
    ip.arena_fill(box["arena"])
    yield box
    try:
        errors = ip.arena_errors(box["arena"])
    finally:
        _drop_far_placements()
        del box["arena"]
        torch.cuda.empty_cache()
    assert not errors, f"after the last run: {errors[0]}"


def _drop_far_placements():
    """native_cases keeps the screened sweep's placed inputs per hook: those of a far run are views of the arena."""
    for key in [k for k in nc._screen_placed if isinstance(k, tuple) and k[0] == "far"]:
        del nc._screen_placed[key]


def _exempt(case_name: str, label: str):
    return [k for k in FAR_EXEMPT if k.endswith(":" + label) and fnmatch.fnmatchcase(case_name, k.rsplit(":", 1)[0])]


def _addresses(args):
    """The integers among the arguments of one native call, those inside a ``vq_args`` included."""
    for a in args:
        if isinstance(a, int):
            yield a
        elif isinstance(a, ctypes.Structure):
            for name, _ in a._fields_:
                v = getattr(a, name)
                if isinstance(v, int):
                    yield v


def _spied_run(c: Case, placer: ip.FarPlacer, monkeypatch):
    """-> (outputs, True when an address inside the arena was among the arguments of a native call)."""
    native = _native()
    lo = placer.arena.data_ptr()
    hi = lo + placer.arena.numel()
    seen = []
    call = native._call

    def spy(name, device, *args, **kw):
        seen.append(any(lo <= v < hi for v in _addresses(args)))
        return call(name, device, *args, **kw)

    with monkeypatch.context() as m:
        m.setattr(native, "_call", spy)
        out = _run(c, placer, monkeypatch)
    return out, any(seen)


def _far_runs(c: Case, arena: torch.Tensor, monkeypatch):
    first = ip.FarPlacer(arena, None)
    base, _ = _spied_run(c, first, monkeypatch)
    assert base
    done = {}
    for k, op in enumerate(first.operands):
        listed = _exempt(c.name, op.label)
        if op.layout is None:
            assert listed and FAR_EXEMPT[listed[0]] == NO_AXIS, f"{c.name}: {op.describe()} is not listed in FAR_EXEMPT"
            done[op.label] = (op.dtype, "exempt")
            continue
        placer = ip.FarPlacer(arena, k)
        what = f"operand {op.describe()} far"
        reach = op.reach(arena.numel())
        ip.arena_fill(arena, reach)
        try:
            out, reached = _spied_run(c, placer, monkeypatch)
            assert placer.far is not None and [o.label for o in placer.operands] == [o.label for o in first.operands], \
                f"{c.name} ({what}): the case placed other operands than in its plain run"
            assert list(out) == list(base), f"{c.name} ({what}): the outputs' names changed"
            for name in base:
                _compare(c, name, base[name], out[name], what, odd=False)
            del out
        finally:  # (whatever the run did, the operand's own elements leave the arena: what remains was written outside it)
            if placer.far is not None:
                placer.wipe()
        errors = ip.arena_errors(arena, reach)
        assert not errors, f"{c.name} ({what}): a call wrote outside the operand: {errors[0]}"
        if reached:
            assert not listed, f"{c.name}: {op.describe()} reached a kernel, yet FAR_EXEMPT lists it ({listed})"
        else:
            assert listed and FAR_EXEMPT[listed[0]] != NO_AXIS, \
                f"{c.name}: the far address of {op.describe()} was among the arguments of no native call, and FAR_EXEMPT does not list it"
        done[op.label] = (op.dtype, "far" if reached else "exempt")
        del placer
        _drop_far_placements()
        if torch.cuda.memory_reserved() > arena.numel() + (8 << 30):
            torch.cuda.empty_cache()  # (a ``best`` laid out like a far idx: tens of GiB nobody asks for again)
    DONE[c.name] = done


@pytest.mark.parametrize("c", TABLE, ids=[c.name for c in TABLE])
def test_results_do_not_depend_on_how_far_apart_the_rows_lie(c, arena, monkeypatch):
    t0 = time.perf_counter()
    _far_runs(c, arena["arena"], monkeypatch)
    SECONDS[c.name] = time.perf_counter() - t0
    d = DONE[c.name]
    print(f"  {c.name}: {sum(v[1] == 'far' for v in d.values())} far run(s), {sum(v[1] == 'exempt' for v in d.values())} operand(s) "
          f"exempt; {SECONDS[c.name]:.2f} s")


def test_every_operand_went_far_or_is_listed(arena, monkeypatch):
    """The counts.  Cases the parametrised test above did not run in this session (a selection with -k) are run here."""
    for c in TABLE:
        if c.name not in DONE:
            _far_runs(c, arena["arena"], monkeypatch)
    names = [c.name for c in TABLE]
    assert sorted(DONE) == sorted(names) and len(DONE) == len(TABLE), f"ran {len(DONE)} of {len(TABLE)} cases"
    used = set()
    per_dtype: dict[str, int] = {}
    exempt = 0
    for name, done in DONE.items():
        for label, (dtype, how) in done.items():
            if how == "far":
                per_dtype[str(dtype).replace("torch.", "")] = per_dtype.get(str(dtype).replace("torch.", ""), 0) + 1
            else:
                exempt += 1
                used.update(_exempt(name, label))
    print(f"far operands: {sum(per_dtype.values())} in {sum(1 for d in DONE.values() if 'far' in [v[1] for v in d.values()])} of "
          f"{len(TABLE)} cases, per dtype {dict(sorted(per_dtype.items()))}; exempt (FAR_EXEMPT): {exempt}; cases without a "
          f"row-strided operand or destination: {sorted(n for n, d in DONE.items() if not d)}")
    assert sum(per_dtype.values()) > 0 and {"float32", "int64"} <= set(per_dtype)
    stale = sorted(set(FAR_EXEMPT) - used)
    assert not stale, f"FAR_EXEMPT entries that match no operand that stayed near: {stale}"
    if SECONDS:
        slow = sorted(SECONDS.items(), key=lambda kv: -kv[1])[:5]
        print(f"wall time of the {len(SECONDS)} parametrised cases: {sum(SECONDS.values()):.1f} s; the slowest: "
              + ", ".join(f"{n} {s:.1f} s" for n, s in slow))


def test_the_listed_binding_lines_exist():
    """FAR_EXEMPT quotes native.py: each line stands in the function it names."""
    import inspect

    native = _native()
    for key, line in FAR_EXEMPT.items():
        if line == NO_AXIS:
            continue
        fn, text = line.split(": ", 1)
        assert text in inspect.getsource(getattr(native, fn)), (key, line)
