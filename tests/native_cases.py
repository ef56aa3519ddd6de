"""The table of native calls that tests/test_gpu_uninitialised_memory.py (poisoned workspaces and outputs),
tests/test_gpu_input_extents.py (poisoned surroundings of the inputs) and tests/test_gpu_far_operands.py (one operand whose rows
span more than 2^31 elements) share: one small, path-selecting case per wrapper and launch path of vector_quantization.native.
A plain module: it holds no test, and every case stands here, so that the three suites see one table in any selection.

Every device tensor a case hands to a wrapper comes from ONE hook, ``place(cpu_tensor, role)``: the inputs are built on the
host and placed, so that a test can decide where they lie in device memory.  The default hook is ``.to(DEV)``; a test installs
another one with ``placing(hook)`` (tests/input_poison.Placer).  ``role`` says what the operand is: "rows" for a row-strided
operand whose strides the wrapper forwards to the kernels (``row_dims``: how many trailing dims make up one contiguous row: 1
for [H, M, D] rows, 0 for an [H, M] operand with one element per row, 2 for LFQ's [N, C, d] and the decode tables), "dense"
otherwise.  ``dest(shape, dtype)`` asks the hook for a caller-side strided destination where a wrapper accepts one (None:
the wrapper allocates its own, as in every plain run).

Float atomics (the non-deterministic EMA scatter-adds) run on train_dense.exact_inputs / grid-valued codebooks, whose sums
are exact in any order, so those cases can be compared bit for bit as well.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch

import input_poison as ip
import train_dense as td

DEV = "cuda:0"


def _native():
    from vector_quantization import native

    native.load()
    return native


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    return int(_native().device_info().split()[-2])  # "<arch> <n> CUs"


# ------------------------------------------------------------------------------------------------------- the placement hook
class PlainPlacement:
    """The default hook: the tensor as torch puts it on the device, no destinations of the caller's."""

    key = "plain"
    forces_scalar_loads = False  # (a hook that puts rows off the 16-byte grid says so: a case that asserts its launch path asks)

    def __call__(self, t, role="dense", row_dims=1, name=None):
        return t.to(DEV)

    def dest(self, shape, dtype, row_dims=1, name=None):
        return None

    def adopt(self, placements):
        pass

    placements = ()


_hook = [PlainPlacement()]


@contextlib.contextmanager
def placing(hook):
    """Every place() / dest() of the cases goes through ``hook`` inside the block."""
    _hook.append(hook)
    try:
        yield hook
    finally:
        _hook.pop()


def place(t: torch.Tensor, role: str = "dense", row_dims: int = 1, name: str | None = None) -> torch.Tensor:
    assert role in ("rows", "dense")
    return _hook[-1](t, role, row_dims, name)


def dest(shape, dtype=torch.float32, row_dims: int = 1, name: str | None = None):
    return _hook[-1].dest(tuple(shape), dtype, row_dims, name)


def lend(nbytes: int):
    """``nbytes`` of poisoned device memory (uint8, all ones) for a case that lays out a destination of its own: the hook's
    when it has an arena to lend (tests/input_poison.FarPlacer), else a fresh buffer."""
    lender = getattr(_hook[-1], "lend", None)
    if lender is not None:
        return lender(nbytes)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ip.arena_fill(buf)
    return buf


ROWS = dict(role="rows")                       # [.., M, D]: rows of D contiguous elements
PER_ROW = dict(role="rows", row_dims=0)        # [H, M]: one element per row (idx, target, ind, mask)
TABLES = dict(role="rows", row_dims=2)         # [.., K, D] / [N, C, d]: the last two dims are one contiguous row


@functools.lru_cache(maxsize=8)
def _cpu_randn(shape, seed, scale=1.0):
    """(kept for the next run of the same case: the result is shared, nobody writes to it)"""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _cpu_randint(lo, hi, shape, seed, dtype=torch.int64):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _randn(shape, seed, scale=1.0, **where):
    return place(_cpu_randn(shape, seed, scale), **where)


def _randint(lo, hi, shape, seed, dtype=torch.int64, **where):
    return place(_cpu_randint(lo, hi, shape, seed, dtype), **where)


def _grid(shape, seed, **where):
    """Integers in [-15, 15] times 2^-3: sums and differences of a few thousand of them are exact in fp32 in any order."""
    return place(torch.randint(-15, 16, shape, generator=torch.Generator().manual_seed(seed)).float() / 8.0, **where)


class Case:
    """One row of the table.  ``call(native, poisoned)`` -> dict "wrapper.output" -> tensor; ``poisoned(shape, dtype)`` gives
    a caller-side buffer the call must fill.  ``dims``: what the extents of alloc_poison.EXTENTS need.  ``env``: environment
    variables that select the launch path (the library reads them per call)."""

    def __init__(self, name, call, dims=None, env=None):
        self.name, self.call, self.dims, self.env = name, call, dims or {}, env or {}


# case name (or its prefix up to a "*") -> (kernels the case must launch, kernels it must not): the launch path a case is in
# the table for, checked by test_every_kernel_is_reached on the device kernel names of that case alone
PATHS = {
    "quantize-simple": (["vq_search_simple"], ["vq_search_mfma"]),
    "quantize-one_block_*": (["vq_search_mfma", "vq_loss_reduce_kernel"], ["vq_search_persist", "vq_finalize_kernel"]),
    "quantize-wave_pairs-*": (["vq_search_pair512", "vq_loss_reduce_kernel"], ["vq_search_mfma"]),
    "quantize-persistent*": (["vq_search_persist"], ["vq_search_mfma", "vq_resolve_rows_kernel"]),
    "quantize-one_block-ste-sq_err": (["vq_search_mfma"], ["vq_search_persist"]),
    "quantize-resident-dp*": (["vq_search_resident"], ["vq_search_mfma"]),
    # (the contiguous call of the case takes the resident kernel; the one whose destination rows lie 144 MiB apart the
    #  one-block tile-streaming kernel: describe_call keeps a call whose 32 rows of out span 2^32 bytes off the resident one)
    "quantize-resident-wide-out-stride": (["vq_search_resident", "vq_search_mfma"], []),
    "quantize-force_split": (["vq_search_mfma", "vq_finalize_kernel", "vq_loss_reduce_kernel"], []),
    "quantize-per_head-overrules-force_split": (["vq_search_mfma", "vq_loss_reduce_kernel"], ["vq_finalize_kernel"]),
    "quantize-k_split-few_rows": (["vq_search_mfma", "vq_finalize_kernel", "vq_loss_reduce_kernel"], ["vq_keys_init_kernel"]),
    "quantize-main_and_tail": (["vq_search_mfma", "vq_finalize_kernel", "vq_loss_reduce_kernel"], []),
    "quantize-wide-rows*": (["vq_search_mfma|vq_search_pair512"], ["vq_search_simple"]),
    "quantize-lse-pair": (["vq_search_pair512"], []),
    "quantize-residual-fused*": (["vq_search_mfma"], ["vq_finalize_kernel"]),
    "quantize-residual-pair": (["vq_search_pair512"], ["vq_finalize_kernel"]),
    "quantize-residual-remainder-*": (["vq_search_mfma", "vq_finalize_kernel"], []),
    "quantize-screened-own-image": (["vq_pack_scr_kernel", "vq_search_persist", "vq_resolve_rows_kernel"], []),
    "quantize-screened-cached-image": (["vq_search_persist", "vq_resolve_rows_kernel"], []),
    "keys-init-search-*": (["vq_keys_init_kernel", "vq_finalize_kernel"], []),
    "keys-planes-*": (["vq_finalize_kernel"], ["vq_keys_init_kernel"]),
    "similarities-mfma*": (["vq_sweep_aux"], ["vq_sims_simple"]),
    "similarities-simple": (["vq_sims_simple"], ["vq_sweep_aux"]),
    "similarities-wide": (["vq_search_mfma|vq_search_pair512"], ["vq_sims_simple"]),
    "similarities-wide-simple": (["vq_sims_simple"], []),
    "ce_backward-one-wave*": (["vq_ce_backward"], ["vq_ce_backward_roles", "vq_ce_backward_roles512"]),
    "ce_backward-roles-dp256": (["vq_ce_backward_roles"], []),
    "ce_backward-roles512": (["vq_ce_backward_roles512"], []),
    "ce_backward-live*": (["vq_ce_backward"], ["vq_ce_backward_roles"]),
    "gumbel-1x4150x130x256": (["vq_gumbel_pack_rows", "vq_gumbel_sweep", "vq_gumbel_reduce_parts"], []),
    "reinmax-1x4150x130x256": (["vq_gumbel_pack_ind", "vq_gumbel_reduce_cols", "vq_gumbel_reduce_parts"], []),
    "diversity-splits*": (["vq_diversity_reduce_heads", "vq_gumbel_reduce_parts"], []),
    "ema_accumulate-atomic-owner-path": (["vq_ema_accumulate_owner_kernel"], ["vq_ema_reduce_parts_kernel", "vq_ema_accumulate_kernel"]),
    "ema_accumulate-atomic-atomic-path": (["vq_ema_accumulate_kernel"], ["vq_ema_accumulate_owner_kernel"]),
    "ema_accumulate-det-*": (["vq_ema_accumulate_owner_kernel", "vq_ema_reduce_parts_kernel"], ["vq_ema_accumulate_kernel"]),
    "ema_accumulate_residual-atomic*": (["vq_ema_accumulate_residual_kernel"], []),
    "column_stats-*": (["vq_affine_stats_kernel", "vq_affine_merge_kernel"], []),
    "lfq_quantize-commit": (["lfq_quantize_kernel", "lfq_sum_kernel"], []),
    "lfq_entropy*-split": (["lfq_avg_prob_kernel", "lfq_avg_reduce_kernel", "lfq_sum_kernel"], []),
    "lq_quantize-*": (["lq_quantize_kernel", "lq_loss_kernel", "lq_backward_kernel"], []),
    "decode_codes-*": (["vq_decode_vec_kernel", "vq_decode_scalar_kernel"], []),
}


def _paths_of(name):
    import fnmatch

    return [v for k, v in PATHS.items() if fnmatch.fnmatchcase(name, k)]


TABLE: list[Case] = []


def case(name, dims=None, env=None):
    def add(fn):
        TABLE.append(Case(name, fn, dims, env))
        return fn
    return add


# ----------------------------------------------------------------------------------------------------------- quantize
def _quantize_case(name, shape, seed, env=None, x_dtype=None, **kw):
    def call(native, poisoned):
        h, m, k, d = shape(_cus()) if callable(shape) else shape
        q = kw.get("Q", 1)
        x = _cpu_randn((h, m, d), seed)
        x = place(x if x_dtype is None else x.to(x_dtype), **ROWS)
        cb = place(torch.stack([_cpu_randn((h, k, d), seed + 1 + i, 2.0 ** (-i / 2.0)) for i in range(q)], dim=1).contiguous())
        args = {a: b for a, b in kw.items() if a != "Q"}
        r = native.quantize(x, cb, out=dest((h, m, d)), idx=dest((h, m, q), torch.int64), **args)
        return {f"quantize.{n}": t for n, t in r.items() if t is not None}

    TABLE.append(Case(name, call, env=env))


_quantize_case("quantize-simple", (2, 300, 100, 48), 11, flags=2, ste=True, want_sq_err=True)
# the shapes of test_gpu_launch_plans._sq_err_cases (H = 2, a ragged 37-row remainder), the total and the per-head sums
for _kind, _shape in (("one_block_4_waves", lambda cus: (2, 337, 120, 100)),
                      ("one_block_8_waves", lambda cus: (2, cus // 2 * 256 + 37, 200, 64)),
                      ("wave_pairs", lambda cus: (2, (cus // 4 + 2) * 128 + 37, 256, 512)),
                      ("persistent_train", lambda cus: (2, (cus - 1) * 256 + 37, 1024, 256))):
    _quantize_case(f"quantize-{_kind}-sq_err_total", _shape, 21, want_sq_err=True)
    _quantize_case(f"quantize-{_kind}-sq_err_per_head", _shape, 21, want_sq_err=True, sq_err_per_head=True)
_persist = lambda cus: (2, (cus - 1) * 256 + 37, 1024, 256)  # noqa: E731
_quantize_case("quantize-persistent-plain", _persist, 22)
_quantize_case("quantize-persistent-ste-sq_err", _persist, 22, ste=True, want_sq_err=True)
_quantize_case("quantize-one_block-ste-sq_err", _persist, 22, ste=True, want_sq_err=True, env={"VQ_NO_PERSIST_TRAIN": "1"})
_quantize_case("quantize-resident-dp32", (1, 140077, 256, 32), 23)
_quantize_case("quantize-resident-dp64", (1, 140000, 100, 48), 24)
_quantize_case("quantize-resident-dp128", (1, 150001, 256, 128), 25)
_quantize_case("quantize-force_split", (2, 3001, 1000, 64), 26, flags=4, ste=True, want_sq_err=True)
# (per-head sums exist on the fused path only: the flag is overruled)
_quantize_case("quantize-per_head-overrules-force_split", (2, 3001, 1000, 64), 26, flags=4, want_sq_err=True, sq_err_per_head=True)
_quantize_case("quantize-k_split-few_rows", (1, 300, 4096, 128), 27, want_sq_err=True)
_quantize_case("quantize-main_and_tail", (1, 70000, 1024, 256), 28, ste=True, want_sq_err=True)
_quantize_case("quantize-wide-rows", (1, 300, 1000, 520), 29)
_quantize_case("quantize-wide-rows-train", (2, 100, 64, 640), 30, ste=True, want_sq_err=True)
_quantize_case("quantize-wide-rows-two-code-chunks", (1, 33, 4100, 516), 31)
_quantize_case("quantize-lse", (4, 130, 520, 64), 32, want_lse=True)
_quantize_case("quantize-lse-pair", (1, 300, 300, 400), 33, want_lse=True)
_quantize_case("quantize-fp16-rows", (1, 5000, 300, 64), 34, x_dtype=torch.float16)
_quantize_case("quantize-bf16-rows", (1, 5000, 300, 320), 35, x_dtype=torch.bfloat16)
_quantize_case("quantize-residual-fused", (2, 3000, 256, 64), 36, Q=3, env={"VQ_NO_RESIDUAL_TAIL": "1"})
_quantize_case("quantize-residual-fused-train", (2, 3000, 256, 64), 36, Q=3, ste=True, want_sq_err=True,
               env={"VQ_NO_RESIDUAL_TAIL": "1"})
_quantize_case("quantize-residual-fused-per_head", (2, 3000, 256, 64), 36, Q=3, ste=True, want_sq_err=True, sq_err_per_head=True)
_quantize_case("quantize-residual-pair", (1, 1000, 1000, 300), 37, Q=3, ste=True, want_sq_err=True, env={"VQ_NO_RESIDUAL_TAIL": "1"})
_quantize_case("quantize-residual-remainder-eval", (2, 36000, 1024, 128), 38, Q=3)
_quantize_case("quantize-residual-remainder-train", (2, 36000, 1024, 128), 38, Q=3, ste=True, want_sq_err=True)

WIDE_OUT_RS = 36 << 20  # floats between two rows of the destination: 31 rows of it are more than 2^32 bytes


@case("quantize-resident-wide-out-stride")
def _resident_wide_out_stride(native, poisoned):
    """A shape the resident-codebook kernel takes (H * M reaches its rows-per-CU threshold), contiguous x, and a destination
    view [H, M, D] with strides (D, WIDE_OUT_RS, 1): the heads interleaved inside each of 32 rows that lie 144 MiB apart, a span
    of 4.7 GiB.  out and idx equal the contiguous call's bit for bit, and the buffer around the view keeps its poison (a store
    whose 32-bit byte offset wrapped lands at a lower address of the same buffer)."""
    H, M, K, D = -(-512 * _cus() // 32), 32, 64, 32
    x = place(_cpu_randn((H, M, D), 45))
    cb = place(_cpu_randn((H, 1, K, D), 46))
    want = native.quantize(x, cb, want_best=False)
    span = (M - 1) * WIDE_OUT_RS + (H - 1) * D + D
    front = 256
    buf = lend(front + span * 4 + 256)
    shape, strides = (H, M, D), (D, WIDE_OUT_RS, 1)
    out = buf[front:front + span * 4].view(torch.float32).as_strided(shape, strides)
    got = native.quantize(x, cb, want_best=False, out=out)
    torch.cuda.synchronize()
    assert got["out"].data_ptr() == out.data_ptr()
    dense = out.contiguous()
    buf.as_strided((*shape, 4), (*(4 * s for s in strides), 1), front).fill_(0xFF)
    errors = ip.arena_errors(buf)
    assert not errors, f"a store outside the destination view [H, M, D] with strides {strides}: {errors[0]}"
    assert torch.equal(got["idx"], want["idx"]), "idx differs from the contiguous call's"
    differ = dense.view(torch.int32) != want["out"].view(torch.int32)
    assert not bool(differ.any()), (f"out differs from the contiguous call's in {int(differ.sum())} element(s), the first at "
                                    f"{torch.nonzero(differ)[0].tolist()}")
    return {"quantize.out": dense, "quantize.idx": got["idx"]}


SCR_M, SCR_K, SCR_D = 131072, 1024, 256
SCR_TILES = SCR_K // 32
SCR_IMAGE_BYTES = SCR_TILES * (32 * 528 + 128) + (5 * SCR_TILES + 2) * 4  # the tiles, the five per-tile arrays, two exponents
SCR_CTRL_BYTES = 16384


@functools.lru_cache(maxsize=None)
def _screen_inputs_cpu():
    """Rows for the screened sweep with BOTH second-pass lists non-empty: midpoints of two codes (near ties: rescored) and
    rows the screen cannot bound (NaN, +-inf, a magnitude outside its range: searched in full)."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn((1, SCR_M, SCR_D), generator=g)
    cb = torch.randn((1, 1, SCR_K, SCR_D), generator=g)
    for i, row in enumerate(range(100, SCR_M, 997)):
        a, b = (7 * i) % SCR_K, (7 * i + 13) % SCR_K
        x[0, row] = 0.5 * (cb[0, 0, a] + cb[0, 0, b])
    x[0, 0, 0] = float("nan")
    x[0, 70001, 5] = float("inf")
    x[0, SCR_M - 1, 251] = -float("inf")
    x[0, 4242] *= 1e18
    return x, cb


_screen_placed: dict = {}


def _screen_inputs():
    """_screen_inputs_cpu on the device, placed once per mode of the hook (a hook of the same key takes the placements over)."""
    hook = _hook[-1]
    if hook.key not in _screen_placed:
        before = len(hook.placements)
        x, cb = _screen_inputs_cpu()
        placed = (place(x, **ROWS), place(cb))
        _screen_placed[hook.key] = (placed, list(hook.placements[before:]))
    else:
        hook.adopt(_screen_placed[hook.key][1])
    return _screen_placed[hook.key][0]


@case("quantize-screened-own-image")
def _screened_own(native, poisoned):
    x, cb = _screen_inputs()
    r = native.quantize(x, cb, want_best=False, out=dest(x.shape), idx=dest((1, SCR_M, 1), torch.int64))
    return {"quantize.out": r["out"], "quantize.idx": r["idx"]}


@case("quantize-screened-cached-image", dims=dict(H=1, image_bytes=SCR_IMAGE_BYTES, ctrl_bytes=SCR_CTRL_BYTES))
def _screened_cached(native, poisoned):
    x, cb = _screen_inputs()
    packed = native.pack_codebooks(cb, 0)
    screen = native.pack_screen(packed, 1, SCR_K, SCR_D, 0)
    assert screen is not None and screen.numel() == native.screen_image_bytes(1, SCR_K, SCR_D, 0)
    before = screen.clone()
    r = native.quantize(x, cb, want_best=False, packed=packed, screen=screen, out=dest(x.shape),
                        idx=dest((1, SCR_M, 1), torch.int64))
    ctrl = screen[-SCR_CTRL_BYTES:].view(torch.int32)
    full, rescore = int(ctrl[4]), int(ctrl[5])  # the two counts of the call just made (no kernel reads them)
    # (rows whose stride rules the float4 loads out are not screened at all -- choose_search wants p.vec_x && p.vec_fin)
    assert (full > 0 and rescore > 0) or _hook[-1].forces_scalar_loads, \
        f"the second pass had {full} rows to search in full and {rescore} to rescore: both lists must be used"
    # what the next call relies on: both counts, the exit ticket and the 160 row tickets from word 8 on are zero again
    assert not bool(ctrl[:3].any()) and not bool(ctrl[8:168].any()), "the call leaves its counts and tickets zeroed for the next"
    return {"pack_codebooks.packed": packed, "pack_screen.screen": before, "quantize.out": r["out"], "quantize.idx": r["idx"]}


# --------------------------------------------------------------------------------------------------------------- keys
def _keys_case(name, shape, seed, planes):
    def call(native, poisoned):
        H, M, K, D = shape
        x, cb = _randn((H, M, D), seed, **ROWS), _randn((H, K, D), seed + 1)
        out = {}
        if planes:
            keys = native.search_key_planes(x, cb)
            assert keys.shape[0] > 1, "few rows and many codes: K must have been split over several planes"
            out["search_key_planes.keys"] = keys
        else:
            keys = poisoned((H, M), torch.int64)
            native.keys_init(keys)
            out["keys_init.keys"] = keys.clone()
            native.search_keys(x, cb, keys)
            out["search_keys.keys"] = keys
        fin = native.finalize_keys(x, cb, keys, ste=True, want_sq_err=True)
        out.update({f"finalize_keys.{n}": t for n, t in fin.items()})
        plain = native.finalize_keys(x, cb, keys)
        out.update({f"finalize_keys.plain_{n}": t for n, t in plain.items() if t is not None})
        return out

    TABLE.append(Case(name, call))


_keys_case("keys-init-search-finalize-one-plane", (2, 501, 2048, 64), 51, False)
_keys_case("keys-planes-finalize-several-planes", (1, 300, 4096, 128), 52, True)
_keys_case("keys-one-plane-wide-rows", (1, 200, 300, 700), 53, False)
_keys_case("keys-one-row", (1, 1, 300, 20), 54, False)


# ------------------------------------------------------------------------------- similarities, softmax, cross entropy
def _sims_case(name, shape, seed, **kw):
    def call(native, poisoned):
        H, M, K, D = shape
        return {"similarities.out": native.similarities(_randn((H, M, D), seed, **ROWS), _randn((H, K, D), seed + 1),
                                                        out=dest((H, M, K)), **kw)}

    TABLE.append(Case(name, call))


_sims_case("similarities-mfma", (4, 130, 520, 64), 61)
_sims_case("similarities-mfma-scalar-stores", (1, 111, 301, 100), 62, metric=1)
_sims_case("similarities-simple", (2, 33, 7, 5), 63, flags=2)
_sims_case("similarities-wide", (2, 100, 64, 640), 64)
_sims_case("similarities-wide-simple", (1, 50, 40, 600), 65, flags=2)


def _ce_case(name, shape, seed, targets=True, backward=True, live=False, env=None):
    def call(native, poisoned):
        H, M, K, D = shape
        x, cb = _randn((H, M, D), seed, **ROWS), _randn((H, K, D), seed + 1)
        target = None
        if targets:
            target = _cpu_randint(0, K, (H, M), seed + 2)
            target[:, ::7] = -1  # ignored rows
            target = place(target, **PER_ROW)
        lse, tl = native.softmax_stats(x, cb, target=target)
        out = {"softmax_stats.lse": lse}
        if targets:
            out["softmax_stats.target_logit"] = tl
        if backward and targets:
            coef = place(torch.tensor([0.37]))
            kw = dict(live=place(_cpu_randn((H, K, D), seed + 1) + 0.05 * _cpu_randn((H, K, D), seed + 3))) if live else {}
            out["ce_backward.grad_x"] = native.ce_backward(x, cb, lse, tl, target, coef, **kw)
        return out

    TABLE.append(Case(name, call, env=env))


_ce_case("softmax_stats-no-targets", (1, 111, 301, 100), 71, targets=False)
_ce_case("softmax_stats-wide-rows", (1, 50, 40, 600), 72, backward=False)
_ce_case("ce_backward-one-wave", (4, 130, 520, 64), 73)
_ce_case("ce_backward-one-wave-dp256", (2, 333, 1030, 200), 74, env={"VQ_CE_NO_ROLES": "1"})
_ce_case("ce_backward-roles-dp256", (2, 333, 1030, 200), 74)
_ce_case("ce_backward-roles512", (2, 150, 300, 400), 75)
_ce_case("ce_backward-live", (1, 300, 256, 64), 76, live=True)
_ce_case("ce_backward-live-dp256", (2, 133, 300, 200), 77, live=True)


# ------------------------------------------------------------------------------------------------------------- gumbel
def _gumbel_case(name, shape, seed, metric=0):
    H, M, K, D = shape

    def call(native, poisoned):
        x, cb = _randn((H, M, D), seed, 0.25 if metric else 1.0, **ROWS), _randn((H, K, D), seed + 1)
        g = _randn((H, M, D), seed + 2, **ROWS)
        lse2, delta = native.gumbel_stats(x, cb, g, metric=metric, tau=1.3)
        gx = native.gumbel_backward_x(x, cb, g, lse2, delta, metric=metric, tau=1.3, out=dest((H, M, D)))
        gc = native.gumbel_backward_codes(x, cb, g, lse2, delta, metric=metric, tau=1.3)
        return {"gumbel_stats.lse2": lse2, "gumbel_stats.delta": delta, "gumbel_backward_x.grad_x": gx,
                "gumbel_backward_codes.grad_codes": gc}

    TABLE.append(Case(name, call, dims=dict(M=M, K=K)))


def _reinmax_case(name, shape, seed, metric=0):
    H, M, K, D = shape

    def call(native, poisoned):
        x, cb = _randn((H, M, D), seed, 0.25 if metric else 1.0, **ROWS), _randn((H, K, D), seed + 1)
        g = _randn((H, M, D), seed + 2, **ROWS)
        ind = _randint(0, K, (H, M), seed + 3, **PER_ROW)
        stats = native.gumbel_reinmax_stats(x, cb, g, metric=metric, tau=2.0)
        col, e, ws = native.gumbel_reinmax_columns(x, cb, g, stats[0], ind, metric=metric, tau=2.0)
        gx = native.gumbel_reinmax_backward_x(x, cb, g, stats, ind, col, e, metric=metric, tau=2.0, out=dest((H, M, D)))
        gc = native.gumbel_reinmax_backward_codes(x, cb, g, stats, col, e, ws, metric=metric, tau=2.0)
        return {"gumbel_reinmax_stats.lse2_tau": stats[0], "gumbel_reinmax_stats.lse2_one": stats[1],
                "gumbel_reinmax_stats.delta0": stats[2], "gumbel_reinmax_columns.col": col, "gumbel_reinmax_columns.e": e,
                "gumbel_reinmax_backward_x.grad_x": gx, "gumbel_reinmax_backward_codes.grad_codes": gc}

    TABLE.append(Case(name, call, dims=dict(M=M, K=K)))


# the multi-tile shapes of test_gpu_gumbel_edges.py / test_gpu_reinmax.py: several tiles per split, the rows split over blockIdx.z
for _i, _s in enumerate([(1, 4150, 130, 256), (4, 2565, 1030, 64), (1, 2130, 130, 200)]):
    _gumbel_case("gumbel-" + "x".join(map(str, _s)), _s, 81 + 3 * _i, metric=_i % 2)
    _reinmax_case("reinmax-" + "x".join(map(str, _s)), _s, 91 + 4 * _i, metric=_i % 2)
_gumbel_case("gumbel-one-split-2x33x7x5", (2, 33, 7, 5), 89)
_reinmax_case("reinmax-one-split-2x33x7x5", (2, 33, 7, 5), 99)


# ---------------------------------------------------------------------------------------------------------- diversity
def _diversity_case(name, hbnkd, pos_div, seed, metric=0, live=False):
    H, B, N, K, D = hbnkd
    M = B * N * pos_div

    def call(native, poisoned):
        from vector_quantization import losses

        x, cb = _randn((H, M, D), seed, 0.25 / max(1.0, D ** 0.5) if metric else 1.0, **ROWS), _randn((H, K, D), seed + 1)
        T = 1.0
        packed = native.pack_codebooks(cb, metric)
        lse2 = native.diversity_stats(x, cb, metric=metric, temperature=T, packed=packed)
        A = native.diversity_accumulate(x, cb, lse2, metric=metric, temperature=T, n_positions=N, pos_div=pos_div)
        U, _ = losses.diversity_upstream(A, 0.7, N, H * M // N, K)
        U = place(U.cpu())  # (torch made it from A: placed like an input of the caller's)
        kw = dict(metric=metric, temperature=T, n_positions=N, pos_div=pos_div)
        delta = native.diversity_delta(x, cb, lse2, U, packed=packed, **kw)
        lv = place(_cpu_randn((H, K, D), seed + 1) + 0.05 * _cpu_randn((H, K, D), seed + 2)) if live else None
        gx = native.diversity_backward_x(x, cb, lse2, delta, U, packed=packed, live=lv, out=dest((H, M, D)), **kw)
        gc = native.diversity_backward_codes(x, cb, lse2, delta, U, **kw)
        assert not bool(A[:, K:].any()), "the entries of A past K are written as 0"
        return {"pack_codebooks.packed": packed, "diversity_stats.lse2": lse2, "diversity_accumulate.A": A,
                "diversity_delta.delta": delta, "diversity_backward_x.grad_x": gx, "diversity_backward_codes.grad_codes": gc}

    TABLE.append(Case(name, call, dims=dict(M=M, K=K)))


_diversity_case("diversity-splits", (1, 2, 70, 64, 32), 1, 101)
_diversity_case("diversity-splits_spp2", (1, 40, 6, 64, 64), 1, 102, metric=1)
_diversity_case("diversity-heads2", (2, 16, 4, 130, 32), 1, 103, live=True)
_diversity_case("diversity-shared2", (1, 6, 5, 90, 40), 2, 104)
_diversity_case("diversity-dp256", (1, 32, 3, 512, 256), 1, 105)


def _orthogonal_case(name, h, n, d, seed):
    def call(native, poisoned):
        x = place(torch.nn.functional.normalize(_cpu_randn((h, n, d), seed), dim=-1), **ROWS)
        stride = int(native.load().vq_gumbel_row_stride(n))
        padded = poisoned((h, stride), torch.float32)
        rowsq, G = native.orthogonal_gram(x, rowsq_out=padded)
        own, _ = native.orthogonal_gram(x, want_g=False)
        return {"orthogonal_gram.rowsq_padded": padded, "orthogonal_gram.G": G, "orthogonal_gram.rowsq": own.contiguous()}

    TABLE.append(Case(name, call, dims=dict(n=n)))


_orthogonal_case("orthogonal-several-tiles-h2", 2, 389, 64, 111)
_orthogonal_case("orthogonal-dp256-h3", 3, 133, 256, 112)
_orthogonal_case("orthogonal-dp32-h2", 2, 261, 20, 113)


@case("sample_codes-and-gumbel_noise")
def _sample(native, poisoned):
    seed = place(torch.tensor([123456789, -987654321], dtype=torch.int64))
    x, cb = _randn((2, 300, 64), 121, **ROWS), _randn((2, 520, 64), 122)
    idx = native.sample_codes(x, cb, tau=0.8, seed=seed)
    wide = native.sample_codes(_randn((1, 70, 400), 123, **ROWS), _randn((1, 300, 400), 124), tau=1.0, seed=seed, metric=1)
    noise, bits = native.gumbel_noise(seed, 2, 37, 70, want_bits=True)
    return {"sample_codes.idx": idx, "sample_codes.idx_dp512": wide, "gumbel_noise.noise": noise, "gumbel_noise.bits": bits}


# ------------------------------------------------------------------------------------------------------ EMA and affine
def _ema_case(name, shape, deterministic, masked=False):
    def call(native, poisoned):
        H, M, K, D = shape
        x, idx = td.exact_inputs(H, M, K, D, td.acc_seed(H, M, K, D), "uniform")
        mask = place(td.acc_mask(H, M, 5)) if masked else None  # (the wrapper makes a contiguous uint8 copy of it)
        counts, sums = native.ema_accumulate(place(x, **ROWS), place(idx, **PER_ROW), K, mask, deterministic=deterministic)
        return {"ema_accumulate.counts": counts, "ema_accumulate.sums": sums}

    TABLE.append(Case(name, call))


for _det in (False, True):
    _tag = "det" if _det else "atomic"
    _ema_case(f"ema_accumulate-{_tag}-owner-path", (2, 4500, 70, 20), _det, masked=True)
    _ema_case(f"ema_accumulate-{_tag}-atomic-path", (2, 1000, 256, 64), _det)
    _ema_case(f"ema_accumulate-{_tag}-wide", (1, 3100, 7, 600), _det)
    _ema_case(f"ema_accumulate-{_tag}-many-codes", (1, 300, 8192, 16), _det)


def _ema_residual_case(name, deterministic, share):
    def call(native, poisoned):
        H, M, K, D, Q = 2, 1500, 40, 24, 3
        x = _grid((H, M, D), 131, **ROWS)
        cb = _grid((H, 1 if share else Q, K, D), 132)
        idx = _cpu_randint(0, K, (H, M, Q), 133)
        idx[:, ::5, 1:] = -1  # dropped stages end a row's chain
        idx = place(idx, **ROWS)
        counts, sums = native.ema_accumulate_residual(x, cb, idx, ste=False, stages_share_codebook=share, deterministic=deterministic)
        return {"ema_accumulate_residual.counts": counts, "ema_accumulate_residual.sums": sums}

    TABLE.append(Case(name, call))


_ema_residual_case("ema_accumulate_residual-atomic", False, False)
_ema_residual_case("ema_accumulate_residual-atomic-shared", False, True)
_ema_residual_case("ema_accumulate_residual-det", True, False)


@case("ema_update")
def _ema_update(native, poisoned):
    out = {}
    for l2norm in (False, True):
        old, avg, counts, sums = (place(t) for t in td.ema_inputs(3, 257, 100, 7001))
        emb = poisoned(tuple(avg.shape), torch.float32)  # overwritten as a whole
        native.ema_update(old, avg, emb, counts, sums, 0.8, 1e-5, l2norm)
        out.update({f"ema_update.cluster_size_{l2norm}": old, f"ema_update.embed_avg_{l2norm}": avg, f"ema_update.embeddings_{l2norm}": emb})
    return out


@case("quantize_backward")
def _quantize_backward(native, poisoned):
    out = {}
    for D, Q, per_head in ((65, 2, False), (256, 1, False), (1028, 3, True)):
        H, M, K = 3, 37, 11
        x, cb = _randn((H, M, D), 141 + D, **ROWS), _randn((H, Q, K, D), 142 + D, 0.5)
        idx = _randint(0, K, (H, M, Q), 143 + D, **ROWS)
        go = _randn((H, M, D), 144 + D, **ROWS)
        ge = place(torch.linspace(-1.0, 1.0, H * Q if per_head else Q, dtype=torch.float64))
        out[f"quantize_backward.grad_x_d{D}"] = native.quantize_backward(x, cb, idx, go, ge, ste=True, sq_err_per_head=per_head)
        out[f"quantize_backward.grad_x_d{D}_loss_only"] = native.quantize_backward(x, cb, idx, None, ge, ste=False, sq_err_per_head=per_head)
    return out


@case("column_stats-masked-several-partials")
def _column_stats(native, poisoned):
    H, M, D = 2, 4099, 70
    x = place(_cpu_randn((H, M, D), 151) * 2.0 + 1.0, **ROWS)
    mask = place(td.acc_mask(H, M, 6), **PER_ROW)
    count, mean, m2 = native.column_stats(x, mask)
    c0, mean0, m20 = native.column_stats(x[:, :1], None)
    return {"column_stats.count": count, "column_stats.mean": mean, "column_stats.m2": m2,
            "column_stats.count_one_row": c0, "column_stats.mean_one_row": mean0, "column_stats.m2_one_row": m20}


@case("affine_apply-both-modes")
def _affine_apply(native, poisoned):
    H, K, D = 2, 257, 70
    src = _randn((H, K, D), 161)
    stats = [_randn((H, 1, D), 162), place(_cpu_randn((H, 1, D), 163).abs() + 0.1), _randn((H, 1, D), 164),
             place(_cpu_randn((H, 1, D), 165).abs() + 0.1)]
    hits = place(_cpu_randint(0, 4, (H, K), 166).float())
    return {"affine_apply.mode0": native.affine_apply(src, *stats, mode=0),
            "affine_apply.mode1": native.affine_apply(src, *stats, mode=1, hits=hits)}


# -------------------------------------------------------------------------------------- scalar quantisers and decoders
@case("lfq_quantize-commit")
def _lfq_quantize(native, poisoned):
    N, C, d = 5003, 2, 6
    v, xa = _randn((N, C, d), 171, **TABLES), _randn((N, C, d), 172, **TABLES)
    mask = place(_cpu_randint(0, 2, (N,), 173).bool())
    q, out, idx, commit = native.lfq_quantize(v, 1.0, xa=xa, mask=mask, want_commit=True)
    q2, _, idx2, _ = native.lfq_quantize(v, 0.5)
    return {"lfq_quantize.q": q, "lfq_quantize.out": out, "lfq_quantize.idx": idx, "lfq_quantize.commit": commit,
            "lfq_quantize.q_plain": q2, "lfq_quantize.idx_plain": idx2}


def _lfq_entropy_case(name, N, C, d, with_rows, seed):
    def call(native, poisoned):
        v = _randn((N, C, d), seed, **TABLES)
        rows = place(torch.arange(0, N, 3)) if with_rows else None
        ps, avg = native.lfq_entropy_forward(v, rows, 1.0, 100.0)
        w_ps = place(torch.tensor(0.3))
        w_cb = _randn((C, 1 << d), seed + 1)
        gv = native.lfq_entropy_backward(v, rows, 1.0, 100.0, w_ps, w_cb)
        return {"lfq_entropy_forward.per_sample_sum": ps, "lfq_entropy_forward.avg_prob": avg, "lfq_entropy_backward.grad_v": gv}

    TABLE.append(Case(name, call))


_lfq_entropy_case("lfq_entropy-all-rows-split", 20011, 2, 6, False, 181)
_lfq_entropy_case("lfq_entropy-row-list", 6001, 1, 10, True, 182)
_lfq_entropy_case("lfq_entropy-few-rows", 37, 3, 3, False, 183)


def _lfq_staged_case(name, T, N, d, rows_kind, seed):
    def call(native, poisoned):
        v = _randn((T, N, d), seed, **ROWS)
        rows = None
        if rows_kind == "shared":
            rows = place(torch.arange(0, N, 2))
        elif rows_kind == "per_stage":
            rows = place(torch.stack([torch.arange(t, N - 4 + t, 4) for t in range(T)]))
        scale = [1.0, 0.5, 0.25][:T]
        ps, avg = native.lfq_entropy_staged_forward(v, rows, scale, 50.0)
        gv = native.lfq_entropy_staged_backward(v, rows, scale, 50.0, _randn((T,), seed + 1), _randn((T, 1 << d), seed + 2))
        return {"lfq_entropy_staged_forward.per_sample_sum": ps, "lfq_entropy_staged_forward.avg_prob": avg,
                "lfq_entropy_staged_backward.grad_v": gv}

    TABLE.append(Case(name, call))


_lfq_staged_case("lfq_entropy_staged-all-rows-split", 3, 20011, 6, None, 191)
_lfq_staged_case("lfq_entropy_staged-per-stage-rows", 3, 6001, 8, "per_stage", 192)
_lfq_staged_case("lfq_entropy_staged-shared-rows", 2, 501, 4, "shared", 193)


@case("rlfq_quantize-and-backward")
def _rlfq(native, poisoned):
    G, N, d, S = 2, 5003, 7, 3
    x = _randn((G, N, d), 201, **ROWS)
    qmag = [1.0, 0.5, 0.25]
    clamp = [None, 2.0, None]
    mask = place(_cpu_randint(0, 2, (N,), 202).bool())
    out, idx, v_all, commit = native.rlfq_quantize(x, qmag, clamp, qmag, mask=mask, want_v=True, want_commit=True)
    o2, i2, _, _ = native.rlfq_quantize(x, qmag, clamp, qmag, spherical=True, ste=False)
    gx = native.rlfq_backward(x, qmag, clamp, qmag, mask=mask, g_out=_randn((G, N, d), 203, **ROWS),
                              w_commit=place(_cpu_randn((G, S), 204).double()), g_ent=_randn((G, S, N, d), 205))
    return {"rlfq_quantize.out": out, "rlfq_quantize.idx": idx, "rlfq_quantize.v_all": v_all, "rlfq_quantize.commit": commit,
            "rlfq_quantize.out_spherical": o2, "rlfq_quantize.idx_spherical": i2, "rlfq_backward.grad_x": gx}


@case("fsq_quantize-backward-decode")
def _fsq(native, poisoned):
    from vector_quantization.finite_scalar_quantization import kernel_consts

    levels, G, N, Q = [8, 5, 5, 5], 2, 5003, 3
    d = len(levels)
    lv = torch.tensor(levels, dtype=torch.float32)
    scales_cpu = torch.stack([(lv - 1) ** -q for q in range(Q)])
    scales = place(scales_cpu)
    consts = place(kernel_consts(torch.tensor(levels, dtype=torch.int32), scales_cpu).contiguous())
    x = _randn((G, N, d), 211, **ROWS)
    out, idx = native.fsq_quantize(x, levels, consts)
    gx = native.fsq_backward(x, levels, consts, _randn((G, N, d), 212, **ROWS))
    one = place(kernel_consts(torch.tensor(levels, dtype=torch.int32), None).contiguous())
    o1, i1 = native.fsq_quantize(x, levels, one)
    # (the decode's indices are the quantizer's own output of this run, placed like an input of the caller's)
    codes_sum, all_codes = native.fsq_decode(place(idx[0].cpu(), **ROWS), levels, scales, want_sum=True, want_all=True)
    return {"fsq_quantize.out": out, "fsq_quantize.idx": idx, "fsq_backward.grad_x": gx, "fsq_quantize.out_one_stage": o1,
            "fsq_quantize.idx_one_stage": i1, "fsq_decode.codes_sum": codes_sum, "fsq_decode.all_codes": all_codes}


@case("lq_quantize-loss-and-backward")
def _lq(native, poisoned):
    levels, C = [5, 4, 3], 2
    B, P, W = 3, 2003, C * len(levels)
    tables = place(torch.cat([torch.linspace(-0.5, 0.5, n) for n in levels]))
    z_cpu = _cpu_randn((B, P, W), 221, 0.4)
    z = place(z_cpu, **ROWS)
    codes, idx, loss = native.lq_quantize(z, levels, tables, C, loss_weights=(0.25, 0.1), out=dest((B, P, W)))
    channel_first = place(z_cpu.permute(0, 2, 1).contiguous().permute(0, 2, 1))  # (dense, the last dim strided: no row to pad)
    c2, _, _ = native.lq_quantize(channel_first, levels, tables, C, want_idx=False)
    gx = native.lq_backward(z, codes, _randn((B, P, W), 222, **ROWS), place(torch.tensor(0.7)), 2.0 / z.numel(),
                            grad_x=dest((B, P, W)))
    return {"lq_quantize.codes": codes, "lq_quantize.idx": idx, "lq_quantize.loss": loss, "lq_quantize.codes_channel_first": c2,
            "lq_backward.grad_x": gx}


@case("decode_codes-vector-and-scalar-kernel")
def _decode(native, poisoned):
    out = {}
    for tag, D in (("vec", 64), ("scalar", 5)):
        G, Q, K, N = 2, 3, 70, 1003
        cb = _randn((G, Q, K, D), 231 + D, **TABLES)
        idx = _randint(-1, K, (G, N, Q), 232 + D, **ROWS)
        s, a = native.decode_codes(cb, idx, want_sum=True, want_all=True, sum_out=dest((G, N, D)), all_out=dest((Q, G, N, D)))
        out[f"decode_codes.codes_sum_{tag}"], out[f"decode_codes.all_codes_{tag}"] = s, a
    return out


@case("lfq_decode")
def _lfq_decode(native, poisoned):
    G, N, Q, d = 2, 1003, 3, 7
    idx_cpu = _cpu_randint(-1, 1 << d, (G, N, Q), 241)
    idx = place(idx_cpu, **ROWS)
    s, a = native.lfq_decode(idx, [1.0, 0.5, 0.25], d, want_sum=True, want_all=True, sum_out=dest((G, N, d)),
                             all_out=dest((Q, G, N, d)))
    s32, _ = native.lfq_decode(place(idx_cpu.to(torch.int32), **ROWS)[..., :2], [1.0, 0.5, 0.25], d)
    return {"lfq_decode.codes_sum": s, "lfq_decode.all_codes": a, "lfq_decode.codes_sum_int32": s32}


# ------------------------------------------------------------------------------------------------------- packed images
def _pack_case(name, n, K, D, metric, seed):
    def call(native, poisoned):
        packed = native.pack_codebooks(_randn((n, K, D), seed), metric)
        assert tuple(packed.shape) == (n, native.packed_floats(K, D))
        return {"pack_codebooks.packed": packed}  # every float of packed_floats(K, D) is defined, the slack included

    TABLE.append(Case(name, call))


_pack_case("pack_codebooks-euclid-dp256", 2, 1000, 256, 0, 251)
_pack_case("pack_codebooks-dot-ragged-k", 3, 301, 100, 1, 252)
_pack_case("pack_codebooks-dims-not-a-multiple-of-4", 1, 7, 5, 0, 253)
_pack_case("pack_codebooks-dp32-one-code", 1, 1, 16, 0, 254)
_pack_case("pack_codebooks-wide-rows", 2, 333, 1030, 0, 255)
_pack_case("pack_codebooks-dp512", 1, 100, 384, 1, 256)


@case("pack_screen-two-heads", dims=dict(H=2, image_bytes=SCR_IMAGE_BYTES, ctrl_bytes=SCR_CTRL_BYTES))
def _pack_screen(native, poisoned):
    cb = _randn((2, SCR_K, SCR_D), 261)
    packed = native.pack_codebooks(cb, 0)
    screen = native.pack_screen(packed, 2, SCR_K, SCR_D, 0)
    assert not bool(screen[-SCR_CTRL_BYTES:].any()), "vq_pack_screen_image_f32 zeroes the control block"
    return {"pack_screen.screen": screen}




# ------------------------------------------------------------------------------------------------------- dead-code expiry
EXPIRE_SEED = (0x0123456789ABCDEF, -0x0FEDCBA987654321)


@case("expire_codes")
def _expire_case(native, poisoned):
    """Pool rows (row-strided: the poison suites pad them), a residual chain, and the normalisation; the three buffers are the
    caller's, picked and the workspace the binding's."""
    H, K, D, N = 2, 1100, 12, 300
    g = torch.Generator().manual_seed(70)
    sizes = torch.rand((H, K), generator=g) * 4.0
    seed = place(torch.tensor(list(EXPIRE_SEED), dtype=torch.int64))
    out = {}
    for l2norm in (False, True):
        cs, avg, emb = place(sizes.clone()), place(torch.randn((H, K, D), generator=g)), place(torch.randn((H, K, D), generator=g))
        pool = place(torch.randn((H, N, D), generator=g), **ROWS)
        n, picked = native.expire_codes(cs, avg, emb, pool, threshold=2.0, reset_cluster_size=2.0, l2norm=l2norm, seed=seed,
                                        want_picked=True)
        out.update({f"expire_codes.cluster_size_{l2norm}": cs, f"expire_codes.embed_avg_{l2norm}": avg,
                    f"expire_codes.embeddings_{l2norm}": emb, f"expire_codes.n_expired_{l2norm}": n,
                    f"expire_codes.picked_{l2norm}": picked})
    Q, Kc, M = 3, 40, 200
    x = place(torch.randn((1, M, D), generator=g), **ROWS)
    codes = place(torch.randn((Q, Kc, D), generator=g) * 0.5)
    idx = place(torch.randint(0, Kc, (1, M, Q), generator=g), **ROWS)
    cs = place((torch.rand((1, Kc), generator=g) * 4.0))
    avg, emb = place(torch.randn((1, Kc, D), generator=g)), place(torch.randn((1, Kc, D), generator=g))
    n, picked = native.expire_codes(cs, avg, emb, None, chain=(x, codes, idx), stage=2, threshold=2.0, reset_cluster_size=2.0,
                                    l2norm=False, seed=seed, want_picked=True)
    out.update({"expire_codes.chain_cluster_size": cs, "expire_codes.chain_embed_avg": avg, "expire_codes.chain_embeddings": emb,
                "expire_codes.chain_n_expired": n, "expire_codes.chain_picked": picked})
    return out


# ------------------------------------------------------------------------- the cross-entropy loss's codebook gradient
def _ce_codes_case(name, shape, seed, metric=0):
    @case(name)
    def call(native, poisoned):
        H, M, K, D = shape
        x, cb = place(_cpu_randn((H, M, D), seed), **ROWS), place(_cpu_randn((H, K, D), seed + 1))
        target = _cpu_randint(0, K, (H, M), seed + 2)
        target[:, ::7] = -1  # ignored rows
        target = place(target, **PER_ROW)
        lse, _ = native.softmax_stats(x, cb, metric=metric, target=target)
        coef = place(torch.tensor([0.37]))
        return {"ce_backward_codes.grad_codes": native.ce_backward_codes(x, cb, lse, target, coef, metric=metric)}


# one per launch path: one row split, several
_ce_codes_case("ce_backward_codes-one-split", (2, 33, 300, 20), 111)
_ce_codes_case("ce_backward_codes-splits", (1, 2100, 64, 32), 112, metric=1)


# ------------------------------------------------------------------------------------- the masked residual stack's pass
RESIDUAL_MASK_K = 11


def _residual_mask_rows(kind, M, rng):
    if kind == "all":
        return np.ones(M, dtype=bool)
    if kind == "none":
        return np.zeros(M, dtype=bool)
    if kind == "alternating":
        return (np.arange(M) % 2 == 0)
    if kind == "boundary":  # a ragged length: the boundary falls inside a wave's group of rows whatever the rows per access
        return np.arange(M) < (M * 2 + 2) // 3
    m = rng.random(M) < 0.6
    m[M // 2] = False  # the row that holds the non-finite element
    return m


def residual_mask_inputs(G, M, D, Qn, share, kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((G, M, D)).astype(np.float32)
    cb = (rng.standard_normal((G, 1 if share else Qn, RESIDUAL_MASK_K, D)) * 0.5).astype(np.float32)
    idx = rng.integers(0, RESIDUAL_MASK_K, (G, M, Qn))
    zero_idx = rng.integers(0, RESIDUAL_MASK_K, (G, Qn))
    mask = _residual_mask_rows(kind, M, rng)
    if kind == "nonfinite":
        x[:, M // 2, D // 2] = np.inf if seed % 2 else np.nan
    return x, cb, idx, zero_idx, mask


@case("residual_mask-forward-and-backward")
def _residual_mask_case(native, poisoned):
    """Both lane mappings (one slice per lane, two slices), per-group and total sums; x, idx and grad_out row-strided (the
    poison suites pad them), out the caller's."""
    out = {}
    for tag, (G, M, D, Qn, per_group) in (("d48", (2, 301, 48, 3, True)), ("d260", (1, 77, 260, 2, False))):
        x, cb, idx, zero_idx, mask = residual_mask_inputs(G, M, D, Qn, False, "nonfinite", 31 + D)
        xp = place(torch.from_numpy(x), **ROWS)
        cbp = place(torch.from_numpy(cb))
        idxp = place(torch.from_numpy(idx), **ROWS)
        maskp, zp = place(torch.from_numpy(mask)), place(torch.from_numpy(zero_idx))
        o, e = native.residual_mask(xp, cbp, idxp, maskp, zp, train=True, want_sq_err=True, sq_err_per_group=per_group,
                                    out=dest((G, M, D)))
        go = place(torch.randn((G, M, D), generator=torch.Generator().manual_seed(D)), **ROWS)
        ge = place(torch.linspace(-1.0, 1.0, G * Qn if per_group else Qn, dtype=torch.float64))
        gx = native.residual_mask_backward(xp, cbp, idxp, maskp, go, ge, train=True, sq_err_per_group=per_group)
        out.update({f"residual_mask.out_{tag}": o, f"residual_mask.sq_err_{tag}": e, f"residual_mask.idx_{tag}": idxp,
                    f"residual_mask_backward.grad_x_{tag}": gx})
    return out


# ------------------------------------------------------------------------------------------- the rotation trick's backward
@case("rotate_backward-per-head-and-total")
def _rotate_backward_case(native, poisoned):
    """x, idx and grad_out row-strided (the poison suites pad them).  Both widths are no multiple of 4, so that the scalar
    variants run wherever the rows are placed: the vector variants add a row's products in another order, and the suites
    compare the runs bit for bit."""
    out = {}
    for tag, (H, M, D, Q, per_head) in (("d50", (2, 301, 50, 3, True)), ("d261", (1, 77, 261, 2, False))):
        x, cb, idx, go, ge = td.backward_inputs(H, M, D, Q, td.BWD_K, 31 + D, per_head=per_head)
        out[f"rotate_backward.grad_x_{tag}"] = native.rotate_backward(place(x, **ROWS), place(cb), place(idx, **ROWS),
                                                                      place(go, **ROWS), place(ge), sq_err_per_head=per_head)
    return out
