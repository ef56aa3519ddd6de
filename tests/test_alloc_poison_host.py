"""CPU: the poisoned-allocation harness itself (tests/alloc_poison.py) -- what it hands out, what its guard bands catch --
and an ast walk over native.py which proves that no tensor is created there by a call the harness does not see."""
from __future__ import annotations

import ast
import inspect

import pytest
import torch

import alloc_poison as ap
from vector_quantization import native

DTYPES = [torch.float32, torch.float64, torch.int64, torch.int32, torch.uint8]


def _raw_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("pattern", ap.PATTERNS, ids=ap.PATTERN_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_empty_has_the_shape_dtype_strides_alignment_and_fill_asked_for(dtype, pattern):
    proxy = ap.TorchProxy(pattern)
    for shape in [(5,), (3, 7), (2, 3, 5), (), (0,), (4, 0, 3)]:
        got = proxy.empty(shape, dtype=dtype, device="cpu")
        want = torch.empty(shape, dtype=dtype)
        assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride() and got.device == want.device
        assert got.is_contiguous()
        assert got.data_ptr() % 16 == 0 or got.numel() == 0
        assert bool(ap.holds_pattern(got, pattern).all())
        word = pattern.to_bytes(4, "little")
        assert bytes(_raw_bytes(got).tolist()) == (word * (got.numel() * got.element_size() // 4 + 1))[:got.numel() * got.element_size()]
    assert proxy.empty(2, 3, dtype=dtype).shape == (2, 3)  # sizes as separate arguments
    assert len(proxy.allocations) == 7 and not proxy.guard_errors()
    proxy.check_guards()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_empty_strided_and_empty_like_follow_torch(dtype):
    proxy = ap.TorchProxy(ap.PATTERNS[2])
    for shape, stride in [((3, 4), (4, 1)), ((3, 4), (10, 2)), ((2, 5, 1), (5, 1, 1)), ((2, 5, 3), (3, 6, 1)), ((0, 4), (4, 1)),
                          ((1, 1), (7, 9))]:
        got = proxy.empty_strided(shape, stride, dtype=dtype, device="cpu")
        assert got.shape == shape and got.stride() == stride and got.dtype == dtype
        assert bool(ap.holds_pattern(got, ap.PATTERNS[2]).all()) if dtype != torch.uint8 or got.is_contiguous() else True
        # the view's last element is the last element of the payload: the guard begins right behind it
        alloc = proxy.allocations[-1]
        span = 0 if got.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(shape, stride))
        assert alloc.nbytes == span * got.element_size()
    dense_t = torch.zeros((4, 6), dtype=dtype).t()                 # dense, not contiguous: empty_like keeps the strides
    sparse = torch.zeros((4, 12), dtype=dtype)[:, ::2]             # not dense: empty_like answers contiguous
    for src in (torch.zeros((2, 3), dtype=dtype), dense_t, sparse, torch.zeros((0, 3), dtype=dtype)):
        got, want = proxy.empty_like(src), torch.empty_like(src)
        assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype
    assert proxy.empty_like(torch.zeros(3, dtype=dtype), dtype=torch.float32).dtype == torch.float32
    proxy.check_guards()


def test_everything_else_is_torch_itself():
    proxy = ap.TorchProxy(0)
    assert proxy.zeros is torch.zeros and proxy.float32 is torch.float32 and proxy.cuda is torch.cuda
    assert proxy.Tensor is torch.Tensor and proxy.tensor is torch.tensor
    with pytest.raises(AttributeError):
        proxy.no_such_attribute


@pytest.mark.parametrize("pattern", ap.PATTERNS, ids=ap.PATTERN_IDS)
def test_a_write_outside_the_buffer_is_reported_and_one_inside_is_not(pattern):
    for nbytes in (0, 1, 6, 64):  # (6: the trailing band begins in the middle of a pattern word)
        proxy = ap.TorchProxy(pattern)
        t = proxy.empty((nbytes,), dtype=torch.uint8)
        alloc = proxy.allocations[-1]
        other = (pattern & 0xFF) ^ 0x5A
        if nbytes:
            t[0] = other
            t[-1] = other
        proxy.check_guards()
        for at, what in ((ap.GUARD - 1, "before"), (ap.GUARD + nbytes, "after"), (0, "before"), (alloc.base.numel() - 1, "after")):
            was = int(alloc.base[at])
            alloc.base[at] = was ^ 0x5A
            errors = proxy.guard_errors()
            assert len(errors) == 1 and f"guard byte(s) {what}" in errors[0], errors
            with pytest.raises(AssertionError, match="wrote outside a buffer"):
                proxy.check_guards()
            alloc.base[at] = was
            proxy.check_guards()


def test_the_binding_allocates_through_the_proxy(monkeypatch):
    proxy = ap.TorchProxy(ap.PATTERNS[1])
    monkeypatch.setattr(native, "torch", proxy)
    ws, nbytes = native._alloc_workspace(100, "cpu")
    assert ws.dtype == torch.float64 and ws.is_contiguous() and nbytes == 112 and ws.numel() * 8 == nbytes
    assert ws.data_ptr() % 16 == 0 and bool(ap.holds_pattern(ws, ap.PATTERNS[1]).all()) and bool(torch.isnan(ws).all())
    assert proxy.sites()[0].startswith("native._alloc_workspace:")
    ws.view(torch.uint8)[-1] = 0          # the last byte asked for: fine
    proxy.check_guards()
    proxy.allocations[0].base[ap.GUARD + nbytes] = 0   # one byte further
    with pytest.raises(AssertionError, match=r"native\._alloc_workspace:\d+: float64\[14\].*1 guard byte\(s\) after"):
        proxy.check_guards()


def test_extents_default_to_everything_and_name_their_header_sentence():
    t = torch.zeros((2, 8))
    assert bool(ap.defined_mask("quantize", "out", t, {}).all())
    m = ap.defined_mask("gumbel_stats", "lse2", t, {"M": 5})
    assert bool(m[:, :5].all()) and not bool(m[:, 5:].any())
    header = open(_header_path()).read()
    flat = " ".join(header.replace("*", " ").split())
    for key, (_, sentence) in ap.EXTENTS.items():
        for piece in sentence.split("..."):
            assert " ".join(piece.split()) in flat, (key, piece)


def _header_path():
    import os

    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vq_mi355x.h")


# tensor-creating calls native.py may make: the three the proxy replaces, and two whose contents are defined
ALLOWED_CREATORS = {"empty", "empty_like", "empty_strided", "zeros", "tensor"}
# everything of torch (functions or methods) that makes a NEW tensor whose contents the caller did not give
CREATOR_NAMES = {"empty", "empty_like", "empty_strided", "empty_permuted", "empty_quantized", "zeros", "zeros_like", "ones",
                 "ones_like", "full", "full_like", "rand", "rand_like", "randn", "randn_like", "randint", "randint_like",
                 "arange", "linspace", "logspace", "eye", "tensor", "as_tensor", "from_numpy", "frombuffer", "new_empty",
                 "new_empty_strided", "new_zeros", "new_ones", "new_full", "new_tensor"}
# torch.zeros_like / full_like inside _softmax_stats_wide's torch.where fill values, never handed to a kernel: named here
# so that the walk stays exact about what it lets through
VALUE_ONLY = {("_softmax_stats_wide", "full_like"), ("_softmax_stats_wide", "zeros_like")}


def test_native_creates_tensors_only_through_calls_the_harness_sees():
    tree = ast.parse(inspect.getsource(native))
    seen, bad = set(), []
    for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        for node in ast.walk(fn):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in CREATOR_NAMES):
                continue
            on_torch = isinstance(node.func.value, ast.Name) and node.func.value.id == "torch"
            if on_torch and node.func.attr in ALLOWED_CREATORS:
                seen.add(node.func.attr)
            elif on_torch and (fn.name, node.func.attr) in VALUE_ONLY:
                continue
            else:
                bad.append(f"{fn.name}:{node.lineno}: {ast.unparse(node.func)}")
    assert not bad, "tensor-creating calls the poison harness cannot see:\n  " + "\n  ".join(bad)
    assert {"empty", "empty_like", "empty_strided", "zeros"} <= seen
    # the name ``torch`` is bound once, by the module's import: nothing re-imports it under another name
    imports = [n for n in ast.walk(tree)
               if (isinstance(n, ast.Import) and any(a.name.split(".")[0] == "torch" for a in n.names))
               or (isinstance(n, ast.ImportFrom) and (n.module or "").split(".")[0] == "torch")]
    assert len(imports) == 1 and isinstance(imports[0], ast.Import) and imports[0].names[0].asname is None
