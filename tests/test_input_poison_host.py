"""CPU: the input-placement harness itself (tests/input_poison.py) -- what the three placements hand out, what the poison
around a payload is, and what check_untouched() catches."""
from __future__ import annotations

import pytest
import torch

import alloc_poison as ap
import input_poison as ip

# every dtype a case of tests/native_cases.py places
DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int64, torch.int32, torch.bool, torch.uint8]
IDS = [str(d).replace("torch.", "") for d in DTYPES]
VARIANTS = (0, 1, 2)


def _sample(dtype, shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype in ip.FLOATS:
        return torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
    if dtype == torch.bool:
        return torch.randint(0, 2, shape, generator=g).bool()
    if dtype == torch.uint8:
        return torch.randint(0, 2, shape, generator=g).to(torch.uint8)
    return torch.randint(-1, 70, shape, generator=g).to(dtype)


def _raw(t: torch.Tensor) -> torch.Tensor:
    return t.clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.uint8)


def _same_bits(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_raw(a), _raw(b))


def _outside_bytes(p: ip.Placement) -> torch.Tensor:
    """The bytes of a placement's buffer that are not payload, in storage order."""
    keep = torch.ones(p.base.numel(), dtype=torch.bool)
    isz = p.view.element_size()
    keep.as_strided((*p.view.shape, isz), (*(s * isz for s in p.view.stride()), 1), ip.GUARD).fill_(False)
    return keep


def _poison_bytes(dtype, variant, src, nbytes):
    """What ``nbytes`` of poison around ``src`` must hold, written out independently of Poison.fill."""
    if dtype in ip.FLOATS:
        return torch.tensor(list(ap.PATTERNS[variant].to_bytes(4, "little")) * (nbytes // 4), dtype=torch.uint8)
    if dtype in ip.MASKS:
        return torch.full((nbytes,), 0xFF if variant == 1 else 0, dtype=torch.uint8)
    value = int(src.max() if variant == 1 else src.min())
    return torch.full((nbytes // src.element_size(),), value, dtype=dtype).view(torch.uint8)


def test_pad_vec_and_the_padded_layout():
    assert ip.pad_vec(64, 4) == 4 and ip.pad_vec(100, 4) == 4 and ip.pad_vec(64, 2) == 8 and ip.pad_vec(2, 8) == 2
    assert ip.pad_vec(5, 4) is None and ip.pad_vec(1, 8) is None and ip.pad_vec(70, 4) is None and ip.pad_vec(20, 2) is None
    # [H, M, D]: row stride D + pad, head stride one whole row longer than M rows
    assert ip.padded_layout((2, 5, 8), 1, 4) == ((6 * 12, 12, 1), 2 * 6 * 12)
    # [H, M] with one element per row; [N, C, d] whose C * d values are one row; [Q, G, N, D]
    assert ip.padded_layout((2, 5), 0, 3) == ((6 * 4, 4), 2 * 6 * 4)
    assert ip.padded_layout((7, 2, 3), 2, 3) == ((9, 3, 1), 8 * 9)
    assert ip.padded_layout((3, 2, 5, 8), 1, 3) == ((2 * 6 * 11, 6 * 11, 11, 1), 3 * 2 * 6 * 11)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plain_and_guarded_keep_the_tensor_as_it_is(dtype, variant):
    for shape in [(5,), (3, 7), (2, 3, 5), (), (2, 3, 4, 8)]:
        src = _sample(dtype, shape)
        plain = ip.Placer("plain", variant)(src)
        assert _same_bits(plain, src) and plain.stride() == src.stride()
        placer = ip.Placer("guarded", variant)
        for role in ("dense", "rows"):
            got = placer(src, role)
            assert _same_bits(got, src) and got.stride() == src.stride() and got.is_contiguous()
            assert got.data_ptr() % 16 == 0, "the alignment class of a fresh allocation"
        p = placer.placements[-1]
        assert p.kind == "guarded" and p.base.numel() >= 2 * ip.GUARD + src.numel() * src.element_size()
        outside = _outside_bytes(p)
        assert torch.equal(p.base[outside], _poison_bytes(dtype, variant, src, p.base.numel())[outside])
        assert placer.counts() == (2, 0, 0)
        placer.check_untouched()
    # a dense permutation keeps its strides; a view with gaps is made contiguous; an empty tensor is left alone
    t = _sample(dtype, (4, 6)).t()
    placer = ip.Placer("guarded", variant)
    assert placer(t).stride() == t.stride() and _same_bits(placer(t), t)
    gaps = _sample(dtype, (4, 12))[:, ::2]
    assert placer(gaps).is_contiguous() and _same_bits(placer(gaps), gaps)
    assert placer(_sample(dtype, (0, 3))).shape == (0, 3) and len(placer.placements) == 4
    placer.check_untouched()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("pad", ("vec", "odd"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padded_rows_have_the_strides_and_the_poison_specified(dtype, pad, variant):
    isz = torch.empty(0, dtype=dtype).element_size()
    for shape, row_dims in [((2, 5, 16), 1), ((2, 5, 7), 1), ((3, 9), 0), ((6, 2, 8), 2), ((2, 3, 4, 16), 2), ((1, 1, 32), 1)]:
        src = _sample(dtype, shape, seed=3)
        placer = ip.Placer("padded", variant, pad)
        got = placer(src, "rows", row_dims)
        cols = 1
        for n in shape[len(shape) - row_dims:]:
            cols *= n
        want_pad = ip.PAD_ODD if pad == "odd" else ip.pad_vec(cols, isz)
        assert _same_bits(got, src)
        p = placer.placements[-1]
        if want_pad is None:  # the vector pad does not apply to these rows: the operand is guarded
            assert p.kind == "guarded" and got.stride() == src.stride() and placer.counts() == (1, 0, 0)
        else:
            lead = len(shape) - row_dims
            rs = cols + want_pad
            assert p.kind == "padded" and p.pad == want_pad and placer.counts() == (0, 1, 0)
            assert got.stride(lead - 1) == rs and got.stride()[lead:] == src.stride()[lead:]
            if lead > 1:
                assert got.stride(lead - 2) == (shape[lead - 1] + 1) * rs, "one whole poisoned row between two heads"
            if pad == "vec":
                assert cols * isz % 16 == 0 and all(s * isz % 16 == 0 for s in got.stride()[:lead]) and got.data_ptr() % 16 == 0
                assert all((cols + q) * isz % 16 for q in range(1, want_pad)), "the smallest such pad"
            else:
                assert rs == cols + 3
            assert p.base.numel() >= 2 * ip.GUARD + ip.padded_layout(shape, row_dims, want_pad)[1] * isz
        outside = _outside_bytes(p)
        assert int(outside.sum()) == p.base.numel() - src.numel() * isz
        assert torch.equal(p.base[outside], _poison_bytes(dtype, variant, src, p.base.numel())[outside]), "bands, pads and gap rows"
        placer.check_untouched()
        # operands of any other role are guarded in this mode too
        dense = placer(src, "dense")
        assert dense.stride() == src.stride() and placer.placements[-1].kind == "guarded"


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
def test_integer_poison_is_a_value_of_the_tensor(dtype):
    src = _sample(dtype, (2, 40, 3), seed=5)
    lo, hi = int(src.min()), int(src.max())
    seen = set()
    for variant in VARIANTS:
        for mode, pad in (("guarded", "odd"), ("padded", "odd"), ("padded", "vec")):
            placer = ip.Placer(mode, variant, pad)
            placer(src, "rows")
            p = placer.placements[-1]
            around = p.base.view(dtype)
            assert lo <= int(around.min()) and int(around.max()) <= hi, "no index outside the operand's own range, anywhere"
            value = int(p.base[:8].view(dtype)[0])
            assert value == (hi if variant == 1 else lo) and bool((src == value).any())
            seen.add(value)
    assert seen == {lo, hi}
    # a mask: all zeros / all ones; a float: the three patterns, NaN in every float type for the second
    for variant in VARIANTS:
        placer = ip.Placer("guarded", variant)
        placer(_sample(torch.bool, (9,)))
        assert int(placer.placements[-1].base[0]) == (0xFF if variant == 1 else 0)
    for dtype_f in ip.FLOATS:
        placer = ip.Placer("padded", 1, "odd")
        placer(_sample(dtype_f, (2, 4, 6)), "rows")
        assert bool(torch.isnan(placer.placements[-1].base[:ip.GUARD].view(dtype_f)).all())
        placer = ip.Placer("padded", 2, "odd")
        placer(_sample(dtype_f, (2, 4, 6)), "rows")
        assert bool(torch.isfinite(placer.placements[-1].base[:ip.GUARD].view(dtype_f)).all())


@pytest.mark.parametrize("variant", VARIANTS)
def test_destinations_and_buffers(variant):
    quiet = ip.Placer("padded", variant, "odd")
    assert quiet.dest((2, 5, 8), torch.float32) is None, "no destination unless asked for: the wrapper allocates its own"
    assert ip.Placer("guarded", variant, dests=True).dest((2, 5, 8), torch.float32) is None
    placer = ip.Placer("padded", variant, "odd", dests=True)
    d = placer.dest((2, 5, 8), torch.float32)
    assert d.shape == (2, 5, 8) and d.stride() == (6 * 11, 11, 1) and bool(ap.holds_pattern(d, ap.PATTERNS[variant]).all())
    i = placer.dest((2, 5, 1), torch.int64)
    assert i.dtype == torch.int64 and i.stride() == (6 * 4, 4, 1)
    vec = ip.Placer("padded", variant, "vec", dests=True)
    assert vec.dest((2, 5, 8), torch.float32).stride() == (6 * 12, 12, 1)
    assert vec.dest((2, 5, 7), torch.float32).is_contiguous(), "the vector pad does not apply: a dense guarded buffer"
    b = placer.buffer((3, 10), torch.int64)
    assert b.is_contiguous() and b.data_ptr() % 16 == 0 and bool(ap.holds_pattern(b, ap.PATTERNS[variant]).all())
    assert placer.find(d) is placer.placements[0] and placer.find(d[:, :2]) is None
    assert placer.counts() == (1, 0, 2)
    d.fill_(1.5)  # the payload is the call's to write
    i.fill_(3)
    placer.check_untouched()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_check_untouched_fires_on_a_pad_a_gap_row_and_a_band_and_on_nothing_else(dtype, variant):
    src = _sample(dtype, (2, 5, 8), seed=7)
    placer = ip.Placer("padded", variant, "odd")
    got = placer(src, "rows")
    p = placer.placements[0]
    isz, rs = src.element_size(), 11
    got.copy_(_sample(dtype, (2, 5, 8), seed=8))  # an in/out operand keeps its extent: the payload may change
    placer.check_untouched()
    pad_or_gap, band = "a pad or a gap row", "guard band"
    spots = {"a pad": (ip.GUARD + 8 * isz, pad_or_gap), "the last pad byte of a row": (ip.GUARD + rs * isz - 1, pad_or_gap),
             "a gap row": (ip.GUARD + 5 * rs * isz + 2, pad_or_gap), "the band in front": (ip.GUARD - 1, band),
             "the first byte": (0, band), "the band behind": (ip.GUARD + p.span_bytes, band),
             "the last byte": (p.base.numel() - 1, band),
             # (past the last payload element: reported as behind the storage)
             "the gap row behind the last head": (ip.GUARD + (2 * 6 - 1) * rs * isz + 1, band)}
    for what, (at, kind) in spots.items():
        was = int(p.base[at])
        p.base[at] = was ^ 0x5A
        errors = placer.errors()
        assert len(errors) == 1 and "outside the payload changed" in errors[0] and "input 0 (rows)" in errors[0], (what, errors)
        assert kind in errors[0], (what, errors)
        with pytest.raises(AssertionError, match="wrote outside an operand"):
            placer.check_untouched()
        p.base[at] = was
        placer.check_untouched()
    # the first byte is named
    p.base[ip.GUARD + 8 * isz + 1] ^= 0x5A
    assert f"byte {8 * isz + 1} of its storage" in placer.errors()[0]


def test_adopted_placements_are_checked_too():
    first = ip.Placer("guarded", 1)
    first(_sample(torch.float32, (3, 4)))
    second = ip.Placer("guarded", 1)
    assert first.key == second.key != ip.Placer("padded", 1).key != ip.Placer("padded", 1, "vec").key
    second.adopt(first.placements)
    second.check_untouched()
    first.placements[0].base[0] ^= 1
    with pytest.raises(AssertionError):
        second.check_untouched()
