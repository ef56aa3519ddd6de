"""Host: the far placement of tests/input_poison.py (far_layout, the arena rule) on the operands of every case of
tests/native_cases.py -- what tests/test_gpu_far_operands.py relies on before it hands a kernel such a view.

The cases build their inputs on the CPU, so a recording hook and a stand-in for ``native`` whose calls raise suffice: every
``place(..., role="rows")`` and ``dest(...)`` up to a case's first native call is recorded with its shape, row_dims and dtype
(FarPlacer asserts the same fit again, on the device, for every operand it places, the later ones included).  For each
recorded operand that can go far (not one row and one head):
  * its last element lies past 2^31 elements from its first, and no two elements share an address;
  * every row begins in the address class modulo 16 it has when the operand is contiguous;
  * the front margin and the span fit the arena (far_reach_bytes <= FAR_ARENA_BYTES);
  * for EVERY element, its element offset and its byte offset, each truncated to uint32 and each wrapped to int32, address
    bytes of the arena.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import input_poison as ip
import native_cases as nc

CUS = 256  # the compute units of an MI355X: the shapes that follow the device are the ones the GPU suite runs there


class _Stop(Exception):
    pass


class _NoNative:
    """Stands in for vector_quantization.native: the arguments of the first call are evaluated (its dest(...) among them),
    then the case ends."""

    def __getattr__(self, name):
        def call(*a, **k):
            raise _Stop(name)
        return call


class _Recorder:
    key, forces_scalar_loads, placements = "record", False, ()

    def __init__(self):
        self.seen = []

    def __call__(self, t, role="dense", row_dims=1, name=None):
        if role == "rows" and t.numel():
            self.seen.append((tuple(t.shape), row_dims, t.dtype))
        return t

    def dest(self, shape, dtype, row_dims=1, name=None):
        if math.prod(shape):
            self.seen.append((tuple(shape), row_dims, dtype))
        return None

    def adopt(self, placements):
        pass


@pytest.fixture(scope="module")
def operands():
    """(shape, row_dims, dtype) -> the cases that place such an operand before their first native call."""
    found: dict = {}
    cus = nc._cus
    nc._cus = lambda: CUS
    try:
        for c in nc.TABLE:
            hook = _Recorder()
            with nc.placing(hook):
                try:
                    c.call(_NoNative(), lambda shape, dtype: torch.empty(shape, dtype=dtype))
                except _Stop:
                    pass
            for op in hook.seen:
                found.setdefault(op, []).append(c.name)
    finally:
        nc._cus = cus
        nc._screen_placed.pop("record", None)
    return found


def _offsets(shape, strides):
    off = np.zeros(shape, dtype=np.int64)
    for axis, (n, s) in enumerate(zip(shape, strides)):
        off += (np.arange(n, dtype=np.int64) * s).reshape([-1 if a == axis else 1 for a in range(len(shape))])
    return off


def _check(shape, row_dims, itemsize, arena_bytes=ip.FAR_ARENA_BYTES):
    """The four properties of the module docstring for one operand -> its reach in bytes, or None when it cannot go far."""
    layout = ip.far_layout(shape, row_dims, itemsize)
    lead = shape[:len(shape) - row_dims]
    if layout is None:
        assert lead[-1] <= 1 and math.prod(lead[:-1]) <= 1 or math.prod(shape) == 0, (shape, "only one row and one head stays near")
        return None
    strides, span = layout
    off = _offsets(shape, strides)
    assert off.max() == span - 1 and off.max() >= ip.FAR_FRONT, (shape, strides, "the last element lies past 2^31 elements")
    flat = np.sort(off.reshape(-1))
    assert (np.diff(flat) > 0).all(), (shape, strides, "two elements share an address")
    dense = _offsets(shape, torch.empty(shape, device="meta").stride())
    row0 = (slice(None),) * len(lead) + (0,) * row_dims
    assert (((off[row0] - dense[row0]) * itemsize) % 16 == 0).all(), (shape, strides, "a row left its address class modulo 16")
    assert (ip.FAR_FRONT * itemsize) % 16 == 0
    reach = ip.far_reach_bytes(span, itemsize)
    assert reach <= arena_bytes, (shape, strides, f"needs {reach} bytes of arena")
    base = ip.FAR_FRONT * itemsize
    for what, v in (("element", off), ("byte", off * itemsize)):
        scale = itemsize if what == "element" else 1
        u32 = v & 0xFFFFFFFF
        i32 = ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        for wrapped in (u32, i32):
            start = base + wrapped * scale
            assert start.min() >= 0 and start.max() + itemsize <= reach - ip.GUARD, (shape, strides, what, "a wrapped offset leaves the arena")
    probe = int(off.max())
    assert ip.far_wraps_fit(probe, itemsize, arena_bytes) and ip.far_wraps_fit(ip.FAR_FRONT, itemsize, arena_bytes)
    return reach


def test_every_operand_of_the_table_fits_the_arena(operands):
    assert len(operands) > 60 and sum(len(v) for v in operands.values()) >= len(nc.TABLE), "the recording hook saw too little"
    dtypes = {op[2] for op in operands}
    assert {torch.float32, torch.int64, torch.float16, torch.bfloat16, torch.bool} <= dtypes, dtypes
    worst, near = (0, None), []
    for (shape, row_dims, dtype), cases in sorted(operands.items(), key=str):
        reach = _check(shape, row_dims, torch.empty(0, dtype=dtype).element_size())
        if reach is None:
            near.append((cases, shape))
        elif reach > worst[0]:
            worst = (reach, (shape, row_dims, dtype, cases[0]))
    print(f"{len(operands)} distinct operands; the largest reach {worst[0] / 2 ** 30:.2f} GiB of {ip.FAR_ARENA_BYTES >> 30} GiB: {worst[1]}; "
          f"no axis to stride: {near}")
    assert near == [(["keys-one-row"], (1, 1, 20))]
    assert worst[0] > ip.FAR_ARENA_BYTES - (4 << 30), "the arena is larger than the table needs: shrink FAR_ARENA_BYTES"


@pytest.mark.parametrize("itemsize", [1, 2, 4, 8])
@pytest.mark.parametrize("shape,row_dims", [((2, 5), 0), ((1, 2, 3), 1), ((4, 2, 1), 1), ((3, 1, 20), 1), ((2, 2, 1, 7), 1), ((1, 37, 5), 1),
                                            ((2, 33, 50), 1), ((3, 7, 6), 2), ((2, 3, 5, 4), 2), ((1, 3, 1, 1), 2), ((3, 1000), 0), ((1000,), 0)])
def test_layout_edges(shape, row_dims, itemsize):
    """Two rows, one row under several heads, odd widths in every item size, a third axis in front, tables."""
    assert _check(shape, row_dims, itemsize, arena_bytes=1 << 40) is not None


def test_one_row_and_one_head_cannot_go_far():
    for shape, row_dims in (((1, 1, 20), 1), ((1, 20), 1), ((1,), 0), ((1, 1), 0), ((1, 4, 5), 2)):
        assert ip.far_layout(shape, row_dims, 4) is None


def test_the_stated_row_stride():
    """The rule as the layout's docstring states it, on the operands of the rotation case and of a per-row index operand."""
    (hs, rs, one), span = ip.far_layout((2, 301, 50), 1, 4)
    least = -(-(ip.FAR_FRONT + 50) // 300)
    assert one == 1 and least <= rs < least + 4 and (rs - 50) % 4 == 0 and 302 * rs <= hs < 302 * rs + 4 and (hs - 301 * 50) % 4 == 0
    assert span == hs + 300 * rs + 50
    (hs, rs), _ = ip.far_layout((4, 130), 0, 8)
    assert rs == -(-(ip.FAR_FRONT + 1) // 129) + (0 if (-(-(ip.FAR_FRONT + 1) // 129)) % 2 else 1) and hs >= 131 * rs
