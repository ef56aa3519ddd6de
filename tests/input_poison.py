"""Poisoned placements for the INPUTS of vector_quantization.native, the counterpart of tests/alloc_poison.py: a tensor a test
hands to a wrapper becomes a view into a larger uint8 buffer whose every other byte holds a poison.

What that buys a test (tests/test_gpu_input_extents.py):
  * a kernel that READS outside the extent the header gives an input (a float4 load across D, a lane that reads row M
    where it should clamp, an index one past the end) computes from the poison, so its result differs from the plain run's
    or between two poisons (the neighbouring memory is otherwise another head's finite rows, or allocator slack that holds
    zeros, and 0 * finite = 0);
  * a kernel that WRITES outside an in/out operand or a destination the caller handed over lands in a pad, a gap row or a
    guard band, and check_untouched() names the operand and the first byte.

Three placements (Placer.mode):
  plain    t.to(device), nothing else.
  guarded  the tensor keeps its strides inside [GUARD bytes of poison][payload][GUARD bytes of poison]: same contiguity and
           the same 16-byte alignment class as the plain placement, so every vec4_ok decision and launch plan is the plain
           run's.
  padded   (role "rows" only; every other operand is guarded) the last ``row_dims`` dims are one contiguous row of ``cols``
           elements, the row stride is cols + pad, the stride of the axis in front of the rows is one whole poisoned row
           longer than rows * (cols + pad), guard bands in front and behind.  pad = "vec": the smallest p > 0 with
           (cols + p) * itemsize % 16 == 0, used when cols * itemsize % 16 == 0 (the float4 / 8-byte row loads stay
           eligible; an operand it does not apply to is guarded); pad = "odd": 3 elements, which forces the scalar row loads.

A fourth placement, far (FarPlacer, tests/test_gpu_far_operands.py): ONE row-strided operand of a run becomes a view into a
large arena whose strides carry its last rows past 2^31 elements from its first (far_layout); everything else is placed
plainly.  The arena rule: the operand's first element lies FAR_FRONT * itemsize bytes into the arena and its span ends inside
it, so an element or byte offset that some kernel truncates to 32 bits, or wraps into a signed 32-bit value, still addresses
the arena (far_wraps_fit): a wrong load reads the poison, a wrong store lands in memory the test owns and checks.

Poisons (Placer.variant = 0, 1, 2):
  floats    the three words of alloc_poison.PATTERNS: zeros (a zero code can win a search), all ones (NaN in fp32, fp16, bf16
            and fp64), 0x40E00000 (finite in all four).
  integers  only values that occur in the tensor itself: its minimum (variants 0, 2) or its maximum (variant 1).  A stray read
            yields a VALID index that changes counts, sums or gathers and can never send a gather or scatter out of range:
            the test cannot cause a fault the plain call would not cause.
  masks     (bool / uint8) all zeros (variants 0, 2) or all ones (variant 1).
"""
from __future__ import annotations

import math

import torch

from alloc_poison import GUARD, PATTERNS, PATTERN_IDS, _pattern_bytes, holds_pattern  # noqa: F401  (re-exported)

MODES = ("plain", "guarded", "padded")
PAD_ODD = 3
FLOATS = (torch.float32, torch.float16, torch.bfloat16, torch.float64)
MASKS = (torch.bool, torch.uint8)


def pad_vec(cols: int, itemsize: int):
    """The pad that keeps the vector row loads eligible, or None where rows of ``cols`` elements never were."""
    if cols * itemsize % 16:
        return None
    p = 1
    while (cols + p) * itemsize % 16:
        p += 1
    return p


def padded_layout(shape, row_dims: int, pad: int):
    """-> (strides in elements, elements of storage) of the padded placement of ``shape``: the last ``row_dims`` dims dense
    (one row), the dim in front of them strided by cols + pad, the one in front of that by (rows + 1) * (cols + pad), any
    further dims dense over that."""
    lead, row = tuple(shape[:len(shape) - row_dims]), tuple(shape[len(shape) - row_dims:])
    assert lead, "a padded operand needs an axis of rows"
    cols = math.prod(row)
    rs = cols + pad
    strides = []
    acc = 1
    for n in reversed(row):
        strides.append(acc)
        acc *= n
    strides.append(rs)
    acc = (lead[-1] + 1) * rs
    for n in reversed(lead[:-1]):
        strides.append(acc)
        acc *= n
    return tuple(reversed(strides)), acc


FAR_FRONT = 1 << 31          # elements in front of a far operand's first element, and the distance its last rows must pass
FAR_ARENA_BYTES = 82 << 30   # the largest operand of the table: an int64 [4, M] per-row operand, 16 GiB in front + 4 heads of 16 GiB
FAR_POISON = PATTERNS[1]     # all ones: NaN in every float type, -1 as an index, true as a mask byte


def far_layout(shape, row_dims: int, itemsize: int):
    """-> (strides in elements, elements of storage) of the far placement of ``shape``, or None where the operand has no axis
    to stride (one row and nothing of size >= 2 in front of it).  As padded_layout: the last ``row_dims`` dims are one dense
    row of ``cols`` elements and ``rows`` is the dim in front of them.
      rows >= 2  the row stride rs is the smallest value >= cols and >= ceil((2^31 + cols) / (rows - 1)) with
                 (rs - cols) * itemsize % 16 == 0: row r begins at the address class modulo 16 it has when the operand is
                 contiguous, so every vec4_ok decision and launch plan is the plain run's.  The axis in front strides over
                 rows * rs plus one gap row, rounded up so that each block begins in its contiguous class too.
      rows == 1  and the axes in front hold n >= 2 blocks: the block stride is the smallest value >= 2 * cols and
                 >= ceil((2^31 + cols) / (n - 1)) in the same class.
    Any further dims in front are dense over the block stride."""
    lead, row = tuple(shape[:len(shape) - row_dims]), tuple(shape[len(shape) - row_dims:])
    assert lead, "a far operand needs an axis of rows"
    cols, rows, blocks = math.prod(row), lead[-1], math.prod(lead[:-1])
    if cols == 0 or rows == 0 or blocks == 0 or (rows == 1 and blocks == 1):
        return None
    step = 16 // math.gcd(16, itemsize)  # strides change in steps that keep addresses in their class modulo 16

    def in_class(least, of):  # the smallest value >= least that is congruent to ``of`` modulo step
        return least + (of - least) % step

    if rows >= 2:
        rs = in_class(max(cols, -(-(FAR_FRONT + cols) // (rows - 1))), cols)
        hs = in_class((rows + 1) * rs, rows * cols)
    else:
        rs = cols
        hs = in_class(max(2 * cols, -(-(FAR_FRONT + cols) // (blocks - 1))), cols)
    strides = []
    acc = 1
    for n in reversed(row):
        strides.append(acc)
        acc *= n
    strides.append(rs)
    acc = hs
    for n in reversed(lead[:-1]):
        strides.append(acc)
        acc *= n
    strides = tuple(reversed(strides))
    return strides, 1 + sum((n - 1) * s for n, s in zip(shape, strides))


def far_reach_bytes(span: int, itemsize: int) -> int:
    """Bytes of the arena, from its start, that an access to a far operand of ``span`` elements can touch when an offset is cut
    to 32 bits: the front margin, the span itself or 2^32 bytes (a byte offset as uint32), and a guard band."""
    return FAR_FRONT * itemsize + max(span * itemsize, 1 << 32) + GUARD


def far_wraps_fit(offset: int, itemsize: int, arena_bytes: int) -> bool:
    """The element at ``offset`` (elements from the operand's first): its element offset and its byte offset, each truncated to
    uint32 and each wrapped to int32, address bytes of the arena."""
    base = FAR_FRONT * itemsize

    def u32(v):
        return v & 0xFFFFFFFF

    def i32(v):
        return u32(v) - (1 << 32) if u32(v) & 0x80000000 else u32(v)

    starts = [base + w(offset) * itemsize for w in (u32, i32)] + [base + w(offset * itemsize) for w in (u32, i32)]
    return all(0 <= s and s + itemsize <= arena_bytes for s in starts)


def _dense_strides(t: torch.Tensor):
    """t's own strides when its elements fill their span without gaps (contiguous or a permutation of it), else None."""
    if t.numel() == 0:
        return None
    span = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return tuple(t.stride()) if span == t.numel() else None


class Poison:
    """What the bytes around a payload hold: ``kind`` "float" (a 32-bit pattern), "int" (one element value), "mask" (one byte)."""

    def __init__(self, kind: str, value: int, dtype):
        self.kind, self.value, self.dtype = kind, value, dtype

    def fill(self, nbytes: int, device) -> torch.Tensor:
        """A fresh uint8 buffer of ``nbytes`` (a multiple of 16) that holds nothing but the poison."""
        if self.kind == "float":
            return _pattern_bytes(self.value, nbytes, device).clone()
        if self.kind == "mask":
            return torch.full((nbytes,), self.value, dtype=torch.uint8, device=device)
        return torch.full((nbytes // self.dtype.itemsize,), self.value, dtype=self.dtype, device=device).view(torch.uint8)

    def __repr__(self):
        return f"{self.kind} poison {self.value:#x}" if self.kind != "int" else f"int poison {self.value}"


def poison_for(t: torch.Tensor, variant: int) -> Poison:
    if t.dtype in FLOATS:
        return Poison("float", PATTERNS[variant], t.dtype)
    if t.dtype in MASKS:
        return Poison("mask", 0xFF if variant % 2 else 0x00, t.dtype)
    assert t.dtype in (torch.int64, torch.int32, torch.int16, torch.int8), t.dtype
    value = 0 if t.numel() == 0 else int(t.max() if variant % 2 else t.min())
    return Poison("int", value, t.dtype)


class Placement:
    """One operand: ``base`` = [GUARD][span of the view, pads and gap rows included][GUARD, rounded up to 16 bytes]."""

    def __init__(self, name, base, view, poison, kind, pad):
        self.name, self.base, self.view, self.poison, self.kind, self.pad = name, base, view, poison, kind, pad
        span = 0 if view.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(view.shape, view.stride()))
        self.span_bytes = span * view.element_size()

    def describe(self) -> str:
        v = self.view
        return (f"{self.name}: {self.kind} {str(v.dtype).replace('torch.', '')}{list(v.shape)} strides {list(v.stride())}, "
                f"{self.poison!r}")

    def outside(self) -> torch.Tensor:
        """bool per byte of ``base``: the byte is not part of the payload and no longer holds the poison."""
        want = self.poison.fill(self.base.numel(), self.base.device)
        bad = self.base != want
        v = self.view
        if v.numel():
            isz = v.element_size()
            bad.as_strided((*v.shape, isz), (*(s * isz for s in v.stride()), 1), GUARD).fill_(False)
        return bad

    def errors(self):
        bad = torch.nonzero(self.outside()).flatten()
        if not bad.numel():
            return []
        first = int(bad[0])
        if first < GUARD:
            where = f"{GUARD - first} byte(s) in front of its start (guard band)"
        elif first >= GUARD + self.span_bytes:
            where = f"{first - GUARD - self.span_bytes} byte(s) past its end (guard band)"
        else:
            where = f"byte {first - GUARD} of its storage (a pad or a gap row)"
        return [f"{self.describe()}: {int(bad.numel())} byte(s) outside the payload changed, the first at {where}"]


class Placer:
    """The hook tests/native_cases.py places every device tensor through.  ``placer(cpu_tensor, role, row_dims)`` -> the
    tensor on ``device`` in this placer's mode; ``dest(shape, dtype, row_dims)`` -> a poisoned destination for a wrapper's
    ``out=`` (None unless ``dests``: the wrapper then allocates its own); ``buffer(shape, dtype)`` -> a dense, guarded,
    poisoned caller-side buffer.  Everything handed out is remembered for check_untouched()."""

    def __init__(self, mode: str = "plain", variant: int = 0, pad: str = "odd", device="cpu", dests: bool = False):
        assert mode in MODES and variant in (0, 1, 2) and pad in ("vec", "odd")
        self.mode, self.variant, self.pad, self.device, self.dests = mode, variant, pad, torch.device(device), dests
        self.placements: list[Placement] = []

    @property
    def key(self):
        """What a cache of placed inputs is keyed by."""
        return (self.mode, self.variant, self.pad if self.mode == "padded" else None, str(self.device))

    @property
    def forces_scalar_loads(self) -> bool:
        """Row-strided operands get rows that begin off the 16-byte grid: a case that asserts its launch path may ask."""
        return self.mode == "padded" and self.pad == "odd"

    @property
    def pattern(self) -> int:
        return PATTERNS[self.variant]

    # -- placements ---------------------------------------------------------------------------------------------------
    def __call__(self, t: torch.Tensor, role: str = "dense", row_dims: int = 1, name: str | None = None) -> torch.Tensor:
        assert role in ("rows", "dense") and t.device.type == "cpu", "cases build their inputs on the host"
        if self.mode == "plain" or t.numel() == 0:
            return t.to(self.device)
        name = name or f"input {len(self.placements)} ({role})"
        poison = poison_for(t, self.variant)
        pad = self._pad(t.shape, t.element_size(), role, row_dims)
        if pad is None:
            strides = _dense_strides(t)
            if strides is None:
                t = t.contiguous()
                strides = tuple(t.stride())
            return self._make(name, t, tuple(t.shape), strides, t.numel(), poison, "guarded", 0)
        strides, span = padded_layout(t.shape, row_dims, pad)
        return self._make(name, t, tuple(t.shape), strides, span, poison, "padded", pad)

    def dest(self, shape, dtype, row_dims: int = 1, name: str | None = None):
        if not self.dests or self.mode != "padded" or math.prod(shape) == 0:
            return None
        name = name or f"destination {len(self.placements)}"
        proto = torch.empty(0, dtype=dtype)
        pad = self._pad(shape, proto.element_size(), "rows", row_dims)
        if pad is None:
            return self.buffer(shape, dtype, name)
        strides, span = padded_layout(shape, row_dims, pad)
        return self._make(name, None, tuple(shape), strides, span, self._dest_poison(dtype), "padded destination", pad)

    def buffer(self, shape, dtype, name: str | None = None) -> torch.Tensor:
        """A dense caller-side buffer the call must fill: poisoned and guarded (plain mode: poisoned, no bands to check)."""
        name = name or f"buffer {len(self.placements)}"
        shape = tuple(shape)
        strides = tuple(torch.empty(shape, dtype=dtype, device="meta").stride())
        return self._make(name, None, shape, strides, math.prod(shape), self._dest_poison(dtype), "guarded buffer", 0)

    def _dest_poison(self, dtype) -> Poison:
        """Destinations hold no values of their own: the 32-bit pattern whatever the type (as alloc_poison fills them)."""
        return Poison("float", self.pattern, dtype)

    def _pad(self, shape, itemsize, role, row_dims):
        if self.mode != "padded" or role != "rows":
            return None
        assert 0 <= row_dims < len(shape)
        if self.pad == "odd":
            return PAD_ODD
        return pad_vec(math.prod(shape[len(shape) - row_dims:]), itemsize)

    def _make(self, name, src, shape, strides, span, poison, kind, pad):
        isz = torch.empty(0, dtype=poison.dtype).element_size()
        total = (GUARD + span * isz + GUARD + 15) // 16 * 16
        base = poison.fill(total, self.device)
        assert base.data_ptr() % 16 == 0
        view = base[GUARD:GUARD + span * isz].view(poison.dtype).as_strided(shape, strides)
        if src is not None:
            view.copy_(src)
        self.placements.append(Placement(name, base, view, poison, kind, pad))
        return view

    def adopt(self, placements):
        """Take over placements another placer of the same key made (cached inputs): they are checked with this one's."""
        self.placements.extend(placements)

    # -- counts and checks --------------------------------------------------------------------------------------------
    def counts(self):
        """-> (operands guarded, operands padded, destinations padded)."""
        k = [p.kind for p in self.placements]
        return k.count("guarded") + k.count("guarded buffer"), k.count("padded"), k.count("padded destination")

    def find(self, t: torch.Tensor):
        """The placement whose view ``t`` is (same storage, offset, shape and strides), or None."""
        for p in self.placements:
            v = p.view
            if v.data_ptr() == t.data_ptr() and v.shape == t.shape and v.stride() == t.stride() and v.dtype == t.dtype:
                return p
        return None

    def errors(self):
        return [e for p in self.placements for e in p.errors()]

    def check_untouched(self):
        """Call after the device is idle: every guard band, pad and gap row of every placement still holds its poison."""
        errors = self.errors()
        assert not errors, "a call wrote outside an operand it was given:\n  " + "\n  ".join(errors)


# ------------------------------------------------------------------------------------------------------ the far placement
class FarOperand:
    """One far-able call of a run: ``label`` ("rows<i>" / "dest<i>", counted per kind in call order), what was asked for, and
    -- for the one that went far -- its view and strides."""

    def __init__(self, label, shape, dtype, row_dims):
        self.label, self.shape, self.dtype, self.row_dims = label, tuple(shape), dtype, row_dims
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        self.layout = far_layout(self.shape, row_dims, self.itemsize)
        self.view = None

    def reach(self, arena_bytes: int) -> int:
        """Bytes from the arena's start that an access to this operand, placed far, can touch (far_reach_bytes, in whole words)."""
        return min(arena_bytes, (far_reach_bytes(self.layout[1], self.itemsize) + 15) // 16 * 16)

    def describe(self) -> str:
        s = f"{self.label} {str(self.dtype).replace('torch.', '')}{list(self.shape)}"
        return s + (f" strides {list(self.layout[0])}" if self.layout else " (no axis to stride)")


class FarPlacer:
    """The hook of a far run (same interface as Placer).  Every ``place(..., role="rows")`` of a non-empty tensor and every
    ``dest(...)`` of a non-empty shape is counted; the ``k``-th of them (``k`` = None: none, the baseline run) becomes a view
    into ``arena`` (uint8, FAR_ARENA_BYTES, filled with FAR_POISON) by far_layout, its first element FAR_FRONT * itemsize bytes
    in; everything else is placed as Placer("plain") places it, destinations of the caller's not handed over."""

    mode, pad, variant, forces_scalar_loads = "far", None, 1, False

    def __init__(self, arena: torch.Tensor, k: int | None = None):
        assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.data_ptr() % 16 == 0
        self.arena, self.k, self.device = arena, k, arena.device
        self.plain = Placer("plain", self.variant, device=arena.device)
        self.operands: list[FarOperand] = []
        self.far: FarOperand | None = None
        self.placements: list = []

    @property
    def key(self):
        return ("far", self.k, id(self))  # (nothing a far run placed is kept for another run)

    def adopt(self, placements):
        pass

    def buffer(self, shape, dtype, name=None):
        return self.plain.buffer(shape, dtype, name)

    def lend(self, nbytes: int) -> torch.Tensor:
        """The first ``nbytes`` of the arena, all poison, for a case that lays out a destination of its own."""
        assert self.k is None and nbytes <= self.arena.numel()
        return self.arena[:nbytes]

    def __call__(self, t: torch.Tensor, role: str = "dense", row_dims: int = 1, name: str | None = None) -> torch.Tensor:
        assert role in ("rows", "dense") and t.device.type == "cpu", "cases build their inputs on the host"
        if role != "rows" or t.numel() == 0:
            return t.to(self.device)
        view = self._next("rows", tuple(t.shape), t.dtype, row_dims)
        if view is None:
            return t.to(self.device)
        view.copy_(t)
        return view

    def dest(self, shape, dtype, row_dims: int = 1, name: str | None = None):
        if math.prod(shape) == 0:
            return None
        return self._next("dest", tuple(shape), dtype, row_dims)

    def _next(self, kind, shape, dtype, row_dims):
        op = FarOperand(f"{kind}{sum(o.label.startswith(kind) for o in self.operands)}", shape, dtype, row_dims)
        self.operands.append(op)
        if len(self.operands) - 1 != self.k or op.layout is None:
            return None
        strides, span = op.layout
        isz, total = op.itemsize, self.arena.numel()
        assert far_reach_bytes(span, isz) <= total, f"{op.describe()}: needs {far_reach_bytes(span, isz)} bytes of arena"
        last = sum((n - 1) * s for n, s in zip(shape, strides))
        assert last >= FAR_FRONT and far_wraps_fit(last, isz, total) and far_wraps_fit(FAR_FRONT, isz, total)
        front = FAR_FRONT * isz
        op.view = self.arena[front:front + span * isz].view(dtype).as_strided(shape, strides)
        self.far = op
        return op.view

    # -- the arena around the far operand ---------------------------------------------------------------------------------
    def wipe(self):
        """Overwrite the far operand's own elements with the poison: what then differs from the poison was written outside it."""
        op = self.far
        isz = op.itemsize
        self.arena.as_strided((*op.shape, isz), (*(s * isz for s in op.view.stride()), 1), FAR_FRONT * isz).fill_(0xFF)


def arena_fill(arena: torch.Tensor, nbytes: int | None = None):
    """One fill kernel: the first ``nbytes`` (all) of the arena hold FAR_POISON."""
    assert FAR_POISON == 0xFFFFFFFF
    n = arena.numel() if nbytes is None else nbytes
    arena[:n].view(torch.int64).fill_(-1)


def arena_errors(arena: torch.Tensor, nbytes: int | None = None, chunk: int = 1 << 30):
    """-> [] when the first ``nbytes`` (all) of the arena hold the poison, else one sentence that names the first byte that
    does not.  Compared in chunks of 1 GiB, one synchronisation at the end."""
    n = arena.numel() if nbytes is None else nbytes
    words = arena[:n].view(torch.int64)
    bad = [(words[i:i + chunk // 8] != -1).any() for i in range(0, words.numel(), chunk // 8)]
    bad = torch.stack(bad).cpu()
    if not bool(bad.any()):
        return []
    i = int(torch.nonzero(bad)[0]) * chunk
    first = i + int(torch.nonzero(arena[i:min(n, i + chunk)] != 0xFF)[0])
    return [f"byte {first} of the arena (the far operand begins at FAR_FRONT * itemsize) no longer holds the poison"]
