"""Host checks of the fused reinmax Gumbel backward: its C-ABI symbols, the documented workspace layout, and the dispatch of
gumbel.relaxed_gather for a backend without the kernels (no compute on a GPU here)."""
from __future__ import annotations

import os
import re

import pytest
import torch

from gumbel_run import assert_grad_close, closed_form64
from helpers import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vq_gumbel_reinmax_workspace_bytes", "vq_gumbel_reinmax_stats_f32", "vq_gumbel_reinmax_columns_f32",
           "vq_gumbel_reinmax_backward_x_f32", "vq_gumbel_reinmax_backward_codes_f32")


def test_symbols_are_declared_listed_and_exported():
    from vector_quantization import native

    text = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vq_[a-z0-9_]+)\s*\(", text))
    lib = native.load()
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in vq_mi355x.h"
        assert name in native.EXPORTED_SYMBOLS, f"{name} is not listed in native.EXPORTED_SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ("gumbel_reinmax_stats", "gumbel_reinmax_columns", "gumbel_reinmax_backward_x", "gumbel_reinmax_backward_codes"):
        assert callable(getattr(native, name))


@pytest.mark.parametrize("shape", [(1, 300, 256, 64), (4, 130, 520, 64), (2, 33, 7, 5), (1, 40, 1, 16), (1, 4150, 130, 256),
                                   (4, 2565, 1030, 64), (1, 262144, 1024, 256)], ids=lambda s: "x".join(map(str, s)))
def test_workspace_bytes_follow_the_documented_layout(shape):
    """[x image][g image][ind int32: H x rsM][col partials: splits x H x rsK][e partials: the same][grad_codes partials:
    splits x H x K x D when splits > 1], splits being the row splits of vq_gumbel_backward_codes_f32's plan (read off its
    own workspace: two images + one [H, K, D] partial per split when there are several)."""
    from vector_quantization import native

    lib = native.load()
    h, m, k, d = shape
    img = native.packed_floats(m, d)
    st_floats = int(lib.vq_gumbel_workspace_bytes(h, m, k, d)) // 4 - 2 * h * img
    assert st_floats % (h * k * d) == 0
    splits = max(1, st_floats // (h * k * d))
    rs_m, rs_k = int(lib.vq_gumbel_row_stride(m)), int(lib.vq_gumbel_row_stride(k))
    assert rs_m % 256 == 0 and rs_m >= m and rs_k % 256 == 0 and rs_k >= k
    want = 2 * h * img + h * rs_m + 2 * splits * h * rs_k + (splits * h * k * d if splits > 1 else 0)
    assert int(lib.vq_gumbel_reinmax_workspace_bytes(h, m, k, d)) == 4 * want


def test_workspace_bytes_are_zero_outside_the_range():
    from vector_quantization import native

    lib = native.load()
    assert lib.vq_gumbel_reinmax_workspace_bytes(1, 300, 256, 257) == 0
    assert lib.vq_gumbel_reinmax_workspace_bytes(1, 300, 256, 400) == 0
    for args in ((0, 300, 256, 64), (1, 0, 256, 64), (1, 300, 0, 64), (1, 300, 256, 0), (-1, 300, 256, 64), (1, -5, 256, 64),
                 (1, 2 ** 31, 256, 64)):
        assert lib.vq_gumbel_reinmax_workspace_bytes(*args) == 0, args
    assert lib.vq_gumbel_reinmax_workspace_bytes(1, 300, 256, 256) > 0


@pytest.mark.parametrize("metric", ["euclid", "dot"])
def test_a_backend_without_the_kernels_keeps_the_chunked_path(metric, monkeypatch):
    from vector_quantization import gumbel, search

    assert not hasattr(OracleBackend, "reinmax_backward") and not hasattr(OracleBackend, "gumbel_backward")
    assert callable(getattr(search._NativeBackend, "reinmax_backward"))
    calls = []
    chunked = gumbel._chunked_backward

    def spy(*args, **kwargs):
        calls.append(1)
        return chunked(*args, **kwargs)

    monkeypatch.setattr(gumbel, "_chunked_backward", spy)
    search.set_backend(OracleBackend)
    try:
        h, m, k, d = 2, 420, 24, 12
        gen = torch.Generator().manual_seed(5)
        x = torch.randn((h, m, d), generator=gen) * (0.25 if metric == "dot" else 1.0)
        c = torch.randn((h, k, d), generator=gen)
        g = torch.randn((h, m, d), generator=gen)
        mt = search.DOT if metric == "dot" else search.EUCLID
        ind = OracleBackend.similarities(x, c, metric=mt).argmax(-1)
        xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
        (gumbel.relaxed_gather(xr, cr, ind, mt, 0.5, reinmax=True) * g).sum().backward()
    finally:
        search.set_backend(None)
    assert calls == [1]
    _, gx64, _, gc64 = closed_form64(x, c, g, ind, 2.0, metric == "dot", reinmax=True)
    assert_grad_close(xr.grad, gx64, f"chunked reinmax {metric} gx")
    assert_grad_close(cr.grad, gc64, f"chunked reinmax {metric} gc")
