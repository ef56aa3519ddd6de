"""Poisoned allocations for vector_quantization.native: every torch.empty / empty_like / empty_strided the binding makes
becomes a view into a larger uint8 buffer that is filled, guard bands included, with one 32-bit pattern.

What that buys a test (tests/test_gpu_uninitialised_memory.py):
  * a kernel that READS a workspace word or an output element nothing wrote in this call computes from the pattern, so its
    result differs between two patterns (the caching allocator otherwise hands back zeros, or the previous call's answer);
  * a kernel that LEAVES an element of an output unwritten leaves the pattern there, which differs between patterns too;
  * a kernel that writes outside the bytes it asked for lands in a guard band, and check_guards() names the allocation.

Nothing in the package changes: the stand-in replaces the NAME ``torch`` inside native.py for the duration of a test
(``monkeypatch.setattr(native, "torch", proxy)``) and forwards everything else.  torch.zeros is left alone: the "caller zeroes"
contracts of counts / sums / grad_v belong to the wrappers.

The registry EXTENTS lists, per (wrapper, output), the elements a call must write where that is NOT all of them, each with
the sentence of include/vq_mi355x.h that grants the exception.
"""
from __future__ import annotations

import sys

import torch

GUARD = 256  # bytes in front of and behind every buffer; 256 keeps every alignment-dependent path choice (vec4_ok) as it is

# 0: what fresh memory usually holds.  All ones: NaN as a float, -1 as an int64, the largest uint32.  0x40E00000: 7.0f, a
# plausible finite value and a large positive integer.
PATTERNS = (0x00000000, 0xFFFFFFFF, 0x40E00000)
PATTERN_IDS = ("zeros", "ones", "seven")


def _pattern_bytes(pattern: int, nbytes: int, device, phase: int = 0) -> torch.Tensor:
    """``nbytes`` uint8 of the little-endian ``pattern``, beginning ``phase`` bytes into a word."""
    word = torch.tensor([(pattern >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8, device=device)
    reps = (nbytes + phase + 3) // 4
    return word.repeat(reps)[phase:phase + nbytes]


def _signed(pattern: int) -> int:
    return pattern - (1 << 32) if pattern & 0x80000000 else pattern


class Allocation:
    """One buffer the proxy handed out: ``base`` = [guard][nbytes of payload][guard (+ up to 3 bytes of rounding)]."""

    def __init__(self, base, view, nbytes, site, pattern):
        self.base, self.view, self.nbytes, self.site, self.pattern = base, view, nbytes, site, pattern

    def describe(self) -> str:
        return f"{self.site}: {str(self.view.dtype).replace('torch.', '')}{list(self.view.shape)} strides {list(self.view.stride())}"

    def guard_errors(self):
        """Descriptions of the guard bytes that no longer hold the pattern (empty: both bands are intact)."""
        errors = []
        bands = (("before", self.base[:GUARD], 0), ("after", self.base[GUARD + self.nbytes:], self.nbytes % 4))
        for name, band, phase in bands:
            want = _pattern_bytes(self.pattern, band.numel(), band.device, phase)
            bad = torch.nonzero(band != want).flatten()
            if bad.numel():
                first = int(bad[0])
                where = first - GUARD if name == "before" else first
                errors.append(f"{self.describe()}: {int(bad.numel())} guard byte(s) {name} the buffer overwritten, the first "
                              f"{abs(where)} byte(s) {'in front of its start' if name == 'before' else 'past its end'}")
        return errors


class TorchProxy:
    """Stands in for the module ``torch`` inside native.py.  Forwards every attribute but the three uninitialised
    allocators, which return pattern-filled views with guard bands and are remembered for check_guards()."""

    def __init__(self, pattern: int):
        assert 0 <= pattern <= 0xFFFFFFFF
        self.pattern = pattern
        self.allocations: list[Allocation] = []

    def __getattr__(self, name):  # (only reached for what the instance does not define itself)
        return getattr(torch, name)

    # -- the three allocators -------------------------------------------------------------------------------------
    def empty(self, *size, **kw):
        kw.pop("out", None)
        device = kw.pop("device", None)
        meta = torch.empty(*size, device="meta", **kw)
        return self._make(meta, device)

    def empty_like(self, t, **kw):
        device = kw.pop("device", None)
        meta = torch.empty_like(t, device="meta", **kw)
        return self._make(meta, t.device if device is None else device)

    def empty_strided(self, size, stride, **kw):
        device = kw.pop("device", None)
        meta = torch.empty_strided(tuple(size), tuple(stride), device="meta", **kw)
        return self._make(meta, device)

    # -- internals ------------------------------------------------------------------------------------------------
    @staticmethod
    def _site() -> str:
        """The function and line of native.py that allocated (the innermost frame of that file on the stack)."""
        f = sys._getframe(2)
        while f is not None:
            if f.f_code.co_filename.endswith("native.py"):
                return f"native.{f.f_code.co_name}:{f.f_lineno}"
            f = f.f_back
        f = sys._getframe(3)
        return f"{f.f_code.co_name}:{f.f_lineno}"

    def _make(self, meta, device):
        device = torch.device("cpu" if device is None else device)
        shape, stride, dtype = tuple(meta.shape), tuple(meta.stride()), meta.dtype
        itemsize = meta.element_size()
        span = 0 if meta.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(shape, stride))  # elements of storage touched
        nbytes = span * itemsize
        total = (GUARD + nbytes + GUARD + 3) // 4 * 4
        base = torch.empty(total, dtype=torch.uint8, device=device)
        base.view(torch.int32).fill_(_signed(self.pattern))
        view = base[GUARD:GUARD + nbytes].view(dtype).as_strided(shape, stride)
        self.allocations.append(Allocation(base, view, nbytes, self._site(), self.pattern))
        return view

    # -- checks ---------------------------------------------------------------------------------------------------
    def guard_errors(self):
        return [e for a in self.allocations for e in a.guard_errors()]

    def check_guards(self):
        """Call after torch.cuda.synchronize(): every guard band of every buffer handed out still holds the pattern."""
        errors = self.guard_errors()
        assert not errors, "a call wrote outside a buffer it was given:\n  " + "\n  ".join(errors)

    def sites(self):
        return [a.describe() for a in self.allocations]


def holds_pattern(t: torch.Tensor, pattern: int) -> torch.Tensor:
    """-> bool tensor of t's shape: the element still holds the fill.  ``t`` comes from a proxy allocation (its storage begins
    on a word boundary); a byte tensor must be dense so that an element's place in its word is its linear index."""
    if t.element_size() % 4 == 0:
        words = t.clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.int32).reshape(*t.shape, t.element_size() // 4)
        return (words == _signed(pattern)).all(dim=-1)
    assert t.element_size() == 1 and t.is_contiguous(), "byte tensors: dense only"
    want = _pattern_bytes(pattern, t.numel(), t.device, int(t.storage_offset() - GUARD) % 4)
    return (t.reshape(-1).view(torch.uint8) == want).reshape(t.shape)


def bits(t: torch.Tensor) -> torch.Tensor:
    """t viewed as integers, for bit-for-bit comparison (NaN == NaN, -0.0 != +0.0)."""
    t = t.clone(memory_format=torch.contiguous_format).reshape(-1)
    if t.dtype in (torch.float32,):
        return t.view(torch.int32)
    if t.dtype in (torch.float64,):
        return t.view(torch.int64)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# Defined extents: which elements of an output a call must write.  Default: all of them.  An entry maps (wrapper, output)
# to (function(tensor, dims) -> bool mask of the tensor's shape, True = defined; the header sentence that grants it).
# ---------------------------------------------------------------------------------------------------------------------
def _first_cols(key):
    def mask(t, dims):
        m = torch.zeros(t.shape, dtype=torch.bool, device=t.device)
        m[..., :dims[key]] = True
        return m
    return mask


def _screen_image(t, dims):
    """The fp16 image fills the front of each head's room; the control block at the end is written (zeroed) as a whole."""
    m = torch.zeros(t.shape, dtype=torch.bool, device=t.device)
    room = (t.numel() - dims["ctrl_bytes"]) // dims["H"]
    for h in range(dims["H"]):
        m[h * room:h * room + dims["image_bytes"]] = True
    m[t.numel() - dims["ctrl_bytes"]:] = True
    return m


_STAT_M = "lse2, delta: [H][vq_gumbel_row_stride(M)] floats (columns past M are not written and reach no result)"
_GUMBEL_M = "lse2 / delta: [H][vq_gumbel_row_stride(M)] floats, 16-byte aligned; columns past M are not written and reach no result"
_REINMAX_M = ("Per-row arrays lse2_tau / lse2_one / delta0: [H][vq_gumbel_row_stride(M)] floats (columns past M are not written and reach no "
              "result)")
EXTENTS = {
    ("gumbel_stats", "lse2"): (_first_cols("M"), _GUMBEL_M),
    ("gumbel_stats", "delta"): (_first_cols("M"), _GUMBEL_M),
    ("gumbel_reinmax_stats", "lse2_tau"): (_first_cols("M"), _REINMAX_M),
    ("gumbel_reinmax_stats", "lse2_one"): (_first_cols("M"), _REINMAX_M),
    ("gumbel_reinmax_stats", "delta0"): (_first_cols("M"), _REINMAX_M),
    ("diversity_stats", "lse2"): (_first_cols("M"), _STAT_M),
    ("diversity_delta", "delta"): (_first_cols("M"), _STAT_M),
    ("orthogonal_gram", "rowsq_padded"): (_first_cols("n"), "rowsq: [H][vq_gumbel_row_stride(n)] floats ...; entries past n are not written"),
    ("pack_screen", "screen"): (_screen_image, "the fp16 image fills about half of it and the rest is unused (never written, never read)"),
    # (grad_v of lfq_entropy_backward / lfq_entropy_staged_backward needs no entry: "other rows of grad_v are not written", so
    #  the wrappers hand the kernels a torch.zeros tensor, which is not poisoned, and every element of the result is defined)
}


def defined_mask(wrapper: str, output: str, t: torch.Tensor, dims: dict) -> torch.Tensor:
    entry = EXTENTS.get((wrapper, output))
    if entry is None:
        return torch.ones(t.shape, dtype=torch.bool, device=t.device)
    return entry[0](t, dims)
