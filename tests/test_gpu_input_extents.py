"""GPU: every native call on inputs embedded in poisoned buffers (tests/input_poison.py), the input-side counterpart of
tests/test_gpu_uninitialised_memory.py, over the same table of cases (tests/native_cases.py).

Every prologue pads on the fly: the kernels widen D to Dp, repeat row M - 1 for the rows past M of a wave's 32-row block,
tile K in 32-code groups, and the per-element kernels handle their own ragged tails.  A float4 load that crosses D, a lane
that reads row M where it should clamp, or an index read one past the end is silent as long as the neighbouring memory is
another head's finite rows or allocator slack that holds zeros.  Here each case runs
  once     plain: the baseline outputs;
  3 times  guarded: every input dense inside [256 B poison][payload][256 B poison], the float poisons of
           alloc_poison.PATTERNS in turn, integer poison alternating between the operand's own minimum and maximum, mask
           poison alternating -- same contiguity and alignment class, so the launch plan is the baseline's;
  6 times  padded: every row-strided operand with poisoned pads behind each row and a poisoned gap row behind each head, with
           the vector-preserving pad where it applies (3 runs) and with an odd pad that forces the scalar row loads (3
           runs); the run with the NaN poison also hands the wrappers that take one a poisoned padded DESTINATION.
After every run every band, pad and gap row still holds its poison (Placer.check_untouched) and every output equals the
baseline bit for bit over its defined extent (alloc_poison.defined_mask).  The one exception: with the odd pad, a float
REDUCTION whose summation order the project ties to the vector / scalar load path is compared under the bound of the direct
test named in LOAD_PATH_SUMS.  Indices, distances, keys and row outputs are never in that registry.
"""
from __future__ import annotations

import fnmatch
import time

import pytest
import torch

import alloc_poison as ap
import input_poison as ip
import native_cases as nc
from native_cases import DEV, TABLE, Case, _native

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# Float reductions whose summation order follows the load path: "case pattern:output" -> (the sentence of the project
# that ties the order to the path, the existing direct test whose bound is borrowed, that bound as a relative tolerance).
# Compared with the baseline under the bound in the odd-pad runs only; bit for bit everywhere else.  Float reductions only.
# ---------------------------------------------------------------------------------------------------------------------
_LAUNCH_PLANS = ("the rtol = 1e-6 of tests/test_gpu_launch_plans.py::test_planned_launches_equal_scalar_kernel, which compares the "
                 "sums of two kernels with different chains")
LOAD_PATH_SUMS: dict[str, tuple[str, str, float]] = {
    # the epilogue of the fused search kernels (vq_search.inc / vq_search_pair.inc, the p.vec_fin branches); quantize-simple
    # and the K-split plans end in vq_finalize_kernel, the entry below
    "quantize-*:quantize.sq_err": (
        "the fused kernels' epilogue sums a row's squared error along the same two lane layouts as `vq_finalize_kernel`",
        _LAUNCH_PLANS, 1e-6),
    "keys-*:finalize_keys.sq_err": (
        "`L` fmaf steps per row and lane — `⌈D/64⌉` scalar, `4⌈D/256⌉` float4 — over `R` rows per wave",
        _LAUNCH_PLANS, 1e-6),
}

# ---------------------------------------------------------------------------------------------------------------------
# Cases without a row-strided operand: every tensor they take must be contiguous.  case pattern -> the binding line of
# native.py that requires it.
# ---------------------------------------------------------------------------------------------------------------------
NO_STRIDED_OPERANDS = {
    "ema_update": "ema_update: assert t.dtype == torch.float32 and t.is_contiguous()",
    "affine_apply-both-modes": "affine_apply: assert src.dtype == torch.float32 and src.dim() == 3 and src.is_contiguous()",
    "pack_codebooks-*": "pack_codebooks: assert cb.dtype == torch.float32 and cb.is_contiguous()",
    "pack_screen-two-heads": "pack_codebooks: assert cb.dtype == torch.float32 and cb.is_contiguous()",
    # (its one row-strided operand is the destination the case lays out itself, 144 MiB between two rows: the hook places
    #  nothing but the dense x and cb; the line is the one that takes such a view as it lies)
    "quantize-resident-wide-out-stride": "quantize: assert out.dtype == torch.float32 and tuple(out.shape) == (H, M, D)",
}

# (mode, pad) of the poisoned runs, three variants each; destinations are handed over in the NaN-poison run of the padded modes
MODES = (("guarded", "odd"), ("padded", "vec"), ("padded", "odd"))
MODE_IDS = ("guarded", "padded-vec", "padded-odd")
DEST_VARIANT = 1

# per mode id: case name -> (operands guarded, operands padded, destinations padded), summed over the three variants
STATS: dict[str, dict[str, tuple[int, int, int]]] = {m: {} for m in MODE_IDS}
SECONDS: dict[str, float] = {}


def _listed(name: str):
    return [k for k in NO_STRIDED_OPERANDS if fnmatch.fnmatchcase(name, k)]


def _load_path_sum(case_name: str, output: str):
    for key, entry in LOAD_PATH_SUMS.items():
        pattern, out = key.split(":")
        if out == output and fnmatch.fnmatchcase(case_name, pattern):
            return entry
    return None


def _run(c: Case, placer: ip.Placer, monkeypatch):
    """-> the outputs of one run of the case with every input placed by ``placer``; the device is idle afterwards."""
    native = _native()
    with monkeypatch.context() as m, nc.placing(placer):
        for k, v in c.env.items():
            m.setenv(k, v)
        try:
            out = c.call(native, lambda shape, dtype: placer.buffer(shape, dtype))
            torch.cuda.synchronize()
        except RuntimeError as e:  # a device fault poisons the process: nothing more may run on the card from here
            if "HIP error" in str(e) or "illegal memory access" in str(e):
                pytest.exit(f"{c.name} ({placer.mode}, pad {placer.pad}, variant {placer.variant}): {e}", returncode=3)
            raise
    return out


def _first(differ: torch.Tensor):
    return torch.nonzero(differ)[0].tolist()


def _compare(c: Case, name: str, base: torch.Tensor, got: torch.Tensor, what: str, odd: bool):
    wrapper, output = name.split(".", 1)
    assert got.shape == base.shape and got.dtype == base.dtype, f"{c.name}: {name} ({what})"
    defined = ap.defined_mask(wrapper, output, base, c.dims)
    differ = (ap.bits(got) != ap.bits(base)).reshape(base.shape) & defined
    n = int(differ.sum())
    if n == 0:
        return
    entry = _load_path_sum(c.name, name) if odd else None
    at = tuple(_first(differ))
    if entry is None:
        raise AssertionError(f"{c.name}: {name} {list(base.shape)} differs from the plain run in {n} defined element(s) with the "
                             f"inputs {what}; the first at {list(at)}: {base[at].item()!r} (plain) vs {got[at].item()!r}")
    assert base.dtype in (torch.float32, torch.float64), "LOAD_PATH_SUMS holds float reductions only"
    rtol = entry[2]
    b, g = base.double()[defined], got.double()[defined]
    rel = ((g - b).abs() / b.abs().clamp_min(1e-300)).max().item()
    print(f"  {c.name}: {name} ({what}): {n} element(s) differ, largest relative difference {rel:.3e} (bound {rtol:.3e}, {entry[1]})")
    assert bool(torch.isfinite(g).eq(torch.isfinite(b)).all()) and rel <= rtol, \
        f"{c.name}: {name} ({what}) differs from the plain run by {rel:.3e} relative, more than {rtol:.3e} ({entry[1]})"


def _check_destinations(c: Case, out: dict, placer: ip.Placer, what: str):
    """An output that lies in a buffer the CALLER handed over: the elements outside its defined extent still hold the poison
    (its pads, gap rows and bands are check_untouched's)."""
    for name, t in out.items():
        p = placer.find(t)
        if p is None or p.poison.kind != "float" or t.element_size() % 4:
            continue
        wrapper, output = name.split(".", 1)
        defined = ap.defined_mask(wrapper, output, t, c.dims)
        if bool(defined.all()):
            continue
        touched = ~ap.holds_pattern(t, p.poison.value) & ~defined
        assert not bool(touched.any()), (f"{c.name}: {name} ({what}): {int(touched.sum())} element(s) outside the defined extent "
                                         f"were written; the first at {_first(touched)}")


def _poisoned_runs(c: Case, monkeypatch, base: dict, modes=MODE_IDS):
    for (mode, pad), mode_id in zip(MODES, MODE_IDS):
        if mode_id not in modes:
            continue
        total = (0, 0, 0)
        for variant in range(3):
            dests = mode == "padded" and variant == DEST_VARIANT
            placer = ip.Placer(mode, variant, pad, device=DEV, dests=dests)
            what = f"{mode_id}, poison {ip.PATTERN_IDS[variant]}" + (", padded destinations" if dests else "")
            out = _run(c, placer, monkeypatch)
            try:
                placer.check_untouched()
            except AssertionError as e:
                raise AssertionError(f"{c.name} ({what}): {e}") from None
            assert list(out) == list(base), f"{c.name} ({what}): the outputs' names changed"
            for name in base:
                _compare(c, name, base[name], out[name], what, odd=(mode_id == "padded-odd"))
            _check_destinations(c, out, placer, what)
            total = tuple(a + b for a, b in zip(total, placer.counts()))
            del out, placer
        STATS[mode_id][c.name] = total


@pytest.mark.parametrize("c", TABLE, ids=[c.name for c in TABLE])
def test_results_do_not_depend_on_what_lies_around_the_inputs(c, monkeypatch):
    t0 = time.perf_counter()
    base = _run(c, ip.Placer("plain", 0, device=DEV), monkeypatch)
    assert base
    _poisoned_runs(c, monkeypatch, base)
    SECONDS[c.name] = time.perf_counter() - t0
    g, pv, po = (STATS[m][c.name] for m in MODE_IDS)
    print(f"  {c.name}: guarded {g[0]} operand placements; padded-vec {pv[1]} padded + {pv[0]} guarded, {pv[2]} destination(s); "
          f"padded-odd {po[1]} padded + {po[0]} guarded, {po[2]} destination(s); {SECONDS[c.name]:.2f} s")


def test_every_case_ran_guarded_and_is_padded_or_listed(monkeypatch):
    """The counts per mode.  Cases the parametrised test above did not run in this session (a selection with -k) are run here."""
    for c in TABLE:
        if any(c.name not in STATS[m] for m in MODE_IDS):
            _poisoned_runs(c, monkeypatch, _run(c, ip.Placer("plain", 0, device=DEV), monkeypatch))
    names = [c.name for c in TABLE]
    for mode_id in MODE_IDS:
        s = STATS[mode_id]
        assert sorted(s) == sorted(names) and len(s) == len(TABLE), f"{mode_id}: ran {len(s)} of {len(TABLE)} cases"
        cases_padded = sum(1 for v in s.values() if v[1])
        print(f"{mode_id}: {len(s)} of {len(TABLE)} cases; operand placements guarded {sum(v[0] for v in s.values())}, "
              f"padded {sum(v[1] for v in s.values())} (in {cases_padded} cases), destinations padded {sum(v[2] for v in s.values())}")
    guarded = STATS["guarded"]
    assert len(guarded) == len(TABLE) and all(v[0] > 0 and v[1] == 0 for v in guarded.values()), "no case is exempt from the guarded mode"
    odd = STATS["padded-odd"]
    padded = [n for n in names if odd[n][1] > 0]
    listed = [n for n in names if _listed(n)]
    both = sorted(set(padded) & set(listed))
    neither = sorted(set(names) - set(padded) - set(listed))
    print(f"cases padded in at least one operand: {len(padded)}; listed in NO_STRIDED_OPERANDS: {len(listed)}; table: {len(names)}")
    assert not neither, f"cases that are neither padded in any operand nor listed in NO_STRIDED_OPERANDS: {neither}"
    assert not both, f"NO_STRIDED_OPERANDS lists cases that do have a row-strided operand: {both}"
    assert all(any(fnmatch.fnmatchcase(n, k) for n in names) for k in NO_STRIDED_OPERANDS), "a NO_STRIDED_OPERANDS pattern matches no case"
    assert all(any(fnmatch.fnmatchcase(n, k.split(":")[0]) for n in names) for k in LOAD_PATH_SUMS), "a LOAD_PATH_SUMS pattern matches no case"
    assert sum(v[2] for v in odd.values()) > 0 and sum(v[2] for v in STATS["padded-vec"].values()) > 0, "no padded destination was handed over"
    if SECONDS:
        slow = sorted(SECONDS.items(), key=lambda kv: -kv[1])[:5]
        print(f"wall time of the {len(SECONDS)} parametrised cases: {sum(SECONDS.values()):.1f} s; the slowest: "
              + ", ".join(f"{n} {s:.1f} s" for n, s in slow))


def test_the_listed_binding_lines_exist():
    """NO_STRIDED_OPERANDS quotes native.py: each line stands in the function it names."""
    import inspect

    native = _native()
    for case_pattern, line in NO_STRIDED_OPERANDS.items():
        fn, text = line.split(": ", 1)
        assert text in inspect.getsource(getattr(native, fn)), (case_pattern, line)


def test_the_load_path_sentences_stand_in_the_design_document():
    import os

    text = " ".join(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read().split())
    for key, (sentence, test, rtol) in LOAD_PATH_SUMS.items():
        assert key.endswith("sq_err"), "float reductions only: indices, distances and row outputs never enter the registry"
        assert " ".join(sentence.split()) in text, key
        assert "tests/" in test and 0.0 < rtol <= 1e-6
