"""vq_lfq_decode_f32 on the device: indices -> code vectors for LFQ / ResidualLFQ / GroupedResidualLFQ.

Two yardsticks, both exact.  (1) The bit rule restated in float64 (``_rule``): dim j of stage q is +mag[q] where bit d-1-j of
the low 32 bits of the index is set, else -mag[q]; a dropped stage is 0; the sum runs over the stages.  The stage magnitudes
of the residual stacks are powers of two and there are at most 8 stages here, so every partial sum is a multiple of 2^-7 below
2 and exact in fp32 as in fp64: the order of the adds cannot show and ``torch.equal`` needs no tolerance.  (2) The modules'
own tensor-op expressions, selected per call by VQ_NO_FUSED_DECODE=1."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _mags(Q):
    return tuple(2.0**-q for q in range(Q))


def _rand_idx(G, N, Qg, d, *, seed=0, dtype=torch.int64, drop_rate=0.2):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 2**d, (G, N, Qg), generator=g)
    if drop_rate:
        idx[torch.rand((G, N, Qg), generator=g) < drop_rate] = -1
    return idx.to(dtype).to(DEV)


def _rule(idx, mags, d, drop_null=True):
    """(all [Q, G, N, d], sum [G, N, d]) in float64 on the CPU, from idx [G, N, Qg] and Q = len(mags) magnitudes."""
    idx = idx.cpu().to(torch.int64)
    G, N, Qg = idx.shape
    every = torch.zeros((len(mags), G, N, d), dtype=torch.float64)
    shifts = torch.arange(d - 1, -1, -1)
    for q in range(Qg):
        i = idx[..., q]
        bits = (((i & 0xFFFFFFFF)[..., None] >> shifts) & 1).double()
        codes = (bits * 2 - 1) * float(torch.tensor(mags[q], dtype=torch.float32))
        if drop_null:
            codes = torch.where((i == -1)[..., None], torch.zeros((), dtype=torch.float64), codes)
        every[q] = codes
    return every, every.sum(dim=0)


def _no_negative_zero(t):
    return not bool(((t == 0) & torch.signbit(t)).any())


def _check(idx, mags, d, drop_null=True, **kw):
    from vector_quantization import native

    s, a = native.lfq_decode(idx, mags, d, drop_null=drop_null, want_sum=True, want_all=True, **kw)
    torch.cuda.synchronize()
    every, acc = _rule(idx, mags, d, drop_null)
    assert torch.equal(a.cpu().double(), every), "all_codes differ from the bit rule"
    assert torch.equal(s.cpu().double(), acc), "codes_sum differs from the bit rule"
    assert _no_negative_zero(a) and _no_negative_zero(s), "a dropped stage must give +0.0"
    return s, a


# 1. rows x bits per index: one row, partial / full / several waves and workgroups; d = 1 .. the limit; one and several groups
@pytest.mark.parametrize("d", [1, 2, 7, 16, 20])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_rows_and_dims(N, d):
    for G in (1, 3):
        _check(_rand_idx(G, N, 3, d, seed=N * 31 + d + G), _mags(3), d)


# 2. stage counts on both sides of the index-load batch, fewer stages given than the stack has, both index types
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("Q", [1, 3, 8])
def test_stage_counts(Q, G, dtype):
    for Qg in sorted({1, max(Q - 1, 1), Q}):
        _check(_rand_idx(G, 65, Qg, 7, seed=Q * 7 + Qg + G, dtype=dtype), _mags(Q), 7)
    _check(_rand_idx(G, 65, 9, 7, seed=Q + G, dtype=dtype), _mags(9), 7)  # a second batch of one stage


# 3. outputs: sum only, all only, both
def test_each_output_alone():
    from vector_quantization import native

    idx = _rand_idx(3, 65, 3, 7, seed=3)
    every, acc = _rule(idx, _mags(3), 7)
    s, a = native.lfq_decode(idx, _mags(3), 7, want_sum=True, want_all=False)
    assert a is None and torch.equal(s.cpu().double(), acc)
    s, a = native.lfq_decode(idx, _mags(3), 7, want_sum=False, want_all=True)
    assert s is None and torch.equal(a.cpu().double(), every)
    _check(idx, _mags(3), 7)
    s, a = native.lfq_decode(idx[:, :0], _mags(3), 7, want_sum=True, want_all=True)  # no rows: no launch
    assert s.shape == (3, 0, 7) and a.shape == (3, 3, 0, 7)


# 4. index tensors that are views: transposed, sliced on the stage axis (the missing stages are dropped), sliced on the rows
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_index_views(dtype):
    base = _rand_idx(65, 3, 8, 7, seed=4, dtype=dtype)  # [N, G, Q] in memory
    t = base.permute(1, 0, 2)
    assert not t.is_contiguous()
    s, a = _check(t, _mags(8), 7)
    s2, a2 = _check(t.contiguous(), _mags(8), 7)
    assert torch.equal(s, s2) and torch.equal(a, a2)
    view = t[..., :3]
    padded = t.clone()
    padded[..., 3:] = -1
    s, a = _check(view, _mags(8), 7)
    s2, a2 = _check(padded, _mags(8), 7)
    assert torch.equal(s, s2) and torch.equal(a, a2)
    _check(t[:, 1::2, 2:7], _mags(8), 7)
    _check(t.flip(1), _mags(8), 7)  # (a copy in torch, but rows in another order)


# 5. the drop rule and the bits that count
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_dropped_stages_and_odd_indices(dtype):
    from vector_quantization import native

    d, Q = 7, 3
    rows = [[-1, 5, 9], [5, -1, 9], [5, 9, -1], [-1, -1, -1], [-2, -128, -3], [127, 0, 64], [-1, 3, -2]]
    if dtype == torch.int64:
        rows += [[(5 << 32) | 3, (1 << 40) - 1, -(1 << 33) + 6],   # bits above 31 do not count; low 32 bits all set is NOT -1
                 [(1 << 63) - 1, -(1 << 63), (-1 << 32) | 1]]
    idx = torch.tensor(rows, dtype=dtype, device=DEV)[None]
    s, a = _check(idx, _mags(Q), d)
    # the row with every stage dropped: +0.0 everywhere, sign bit clear
    assert torch.equal(s[0, 3].view(torch.int32), torch.zeros(d, dtype=torch.int32, device=DEV))
    assert torch.equal(a[:, 0, 3].contiguous().view(torch.int32), torch.zeros((Q, d), dtype=torch.int32, device=DEV))
    # a negative index other than -1 is an index: -2 = ...1111110 -> every dim positive but the last
    assert a[0, 0, 4].tolist() == [1.0] * (d - 1) + [-1.0]
    if dtype == torch.int64:
        assert a[0, 0, 7].tolist() == [-1.0] * (d - 2) + [1.0, 1.0]  # (5 << 32) | 3 is 3
        assert a[1, 0, 7].tolist() == [0.5] * d  # (1 << 40) - 1: not dropped, all bits set
    # LFQ's rule: nothing is dropped, -1 is the all-positive code
    s, a = _check(idx, _mags(Q), d, drop_null=False)
    assert a[0, 0, 0].tolist() == [1.0] * d and s[0, 3].tolist() == [1.75] * d
    # fewer stages given: the rest are dropped
    s, a = native.lfq_decode(idx[..., :1], _mags(Q), d, want_sum=True, want_all=True)
    assert torch.equal(a[1:], torch.zeros_like(a[1:])) and _no_negative_zero(a) and torch.equal(s, a[0])


# 6. destinations that are strided slices of wider buffers: everything around them stays as it was
@pytest.mark.parametrize("which", ["sum", "all", "both"])
def test_strided_destinations_leave_their_neighbours(which):
    from vector_quantization import native

    G, N, Q, d = 3, 65, 3, 7
    idx = _rand_idx(G, N, Q, d, seed=6)
    every, acc = _rule(idx, _mags(Q), d)
    poison = 12345.0
    kw = {}
    if which in ("sum", "both"):
        # the group-concatenated destination: [N, 2 + G * d + 3] with the result in columns 2 .. 2 + G * d
        wide_s = torch.full((N, 2 + G * d + 3), poison, device=DEV)
        kw["sum_out"] = wide_s[:, 2:2 + G * d].unflatten(1, (G, d)).permute(1, 0, 2)
        assert kw["sum_out"].data_ptr() == wide_s.data_ptr() + 8
    if which in ("all", "both"):
        wide_a = torch.full((Q, N, G, d + 4), poison, device=DEV)  # rows before groups, padded rows
        kw["all_out"] = wide_a[..., 1:1 + d].permute(0, 2, 1, 3)
    s, a = native.lfq_decode(idx, _mags(Q), d, want_sum="sum_out" in kw, want_all="all_out" in kw, **kw)
    torch.cuda.synchronize()
    if "sum_out" in kw:
        assert s is kw["sum_out"] and a is (kw.get("all_out"))
        assert torch.equal(wide_s[:, 2:2 + G * d].cpu().double(), acc.permute(1, 0, 2).reshape(N, G * d))
        assert bool((wide_s[:, :2] == poison).all()) and bool((wide_s[:, 2 + G * d:] == poison).all())
    if "all_out" in kw:
        assert a is kw["all_out"]
        assert torch.equal(wide_a[..., 1:1 + d].cpu().double(), every.permute(0, 2, 1, 3))
        assert bool((wide_a[..., :1] == poison).all()) and bool((wide_a[..., 1 + d:] == poison).all())
    # a sum destination whose last dim is strided as well (any strides)
    wide = torch.full((G, N, 2 * d), poison, device=DEV)
    native.lfq_decode(idx, _mags(Q), d, sum_out=wide[..., ::2])
    assert torch.equal(wide[..., ::2].cpu().double(), acc) and bool((wide[..., 1::2] == poison).all())


# ---- the modules: the fused decode against their own tensor-op expressions (VQ_NO_FUSED_DECODE=1) and the bit rule
def _both_paths(monkeypatch, fn):
    monkeypatch.delenv("VQ_NO_FUSED_DECODE", raising=False)
    with torch.no_grad():
        fused = fn()
        monkeypatch.setenv("VQ_NO_FUSED_DECODE", "1")
        plain = fn()
    monkeypatch.delenv("VQ_NO_FUSED_DECODE", raising=False)
    return fused, plain


@pytest.mark.parametrize("d", [1, 2, 7, 16, 20])
@pytest.mark.parametrize("spherical", [False, True])
@pytest.mark.parametrize("c,keep", [(1, False), (1, True), (3, True)])
def test_lfq_indices_to_codes(monkeypatch, c, keep, spherical, d):
    import vector_quantization as vq

    for scale, dtype in ((1.0, torch.int64), (1.5, torch.int32), (0.7, torch.int64)):
        mod = vq.LFQ(codebook_size=2**d, num_codebooks=c, keep_num_codebooks_dim=keep, codebook_scale=scale,
                     spherical=spherical, has_projections=False).to(DEV).eval()
        g = torch.Generator().manual_seed(d + c)
        idx = torch.randint(0, 2**d, (2, 37, c) if keep else (2, 37), generator=g).to(dtype).to(DEV)
        idx.view(-1)[:2] = torch.tensor([-1, -2], dtype=dtype)
        fused, plain = _both_paths(monkeypatch, lambda: mod.indices_to_codes(idx))
        assert fused.shape == plain.shape == (2, 37, c * d) and fused.dtype == plain.dtype
        assert torch.equal(fused, plain), f"fused decode differs from the tensor ops (scale {scale})"
        i3 = (idx if keep else idx[..., None]).reshape(-1, c).t()[..., None]
        every, _ = _rule(i3, (mod._code_mag,), d, drop_null=False)
        assert torch.equal(fused.reshape(-1, c, d).permute(1, 0, 2).cpu().double(), every[0])


@pytest.mark.parametrize("c", [1, 3])
def test_lfq_channel_first_projections_and_views(monkeypatch, c):
    import vector_quantization as vq

    d = 7
    g = torch.Generator().manual_seed(c)
    base = torch.randint(0, 2**d, (2, c, 5, 6), generator=g).to(DEV)
    idx = base.permute(0, 2, 3, 1)  # [b, h, w, c]: a transposed view
    assert not idx.is_contiguous() or c == 1
    for proj in (False, True):
        torch.manual_seed(1)
        mod = vq.LFQ(dim=10 if proj else c * d, codebook_size=2**d, num_codebooks=c, keep_num_codebooks_dim=True,
                     channel_first=True, codebook_scale=1.5).to(DEV).eval()
        assert mod.has_projections == proj
        fused, plain = _both_paths(monkeypatch, lambda: mod.indices_to_codes(idx))
        assert fused.shape == (2, 10 if proj else c * d, 5, 6) and torch.equal(fused, plain)
        fused, plain = _both_paths(monkeypatch, lambda: mod.indices_to_codes(idx[:, ::2, 1:], project_out=False))
        assert fused.shape == (2, c * d, 3, 5) and torch.equal(fused, plain)
    # the decode of a forward's indices is the forward's quantized output
    mod = vq.LFQ(codebook_size=2**d, num_codebooks=c, keep_num_codebooks_dim=True, spherical=True).to(DEV).eval()
    x = torch.randn(2, 33, c * d, device=DEV)
    with torch.no_grad():
        q, i, _ = mod(x)
        assert torch.equal(mod.indices_to_codes(i), q)


@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("Q", [1, 3, 8])
def test_residual_lfq(monkeypatch, Q, proj):
    import vector_quantization as vq

    d = 7
    torch.manual_seed(Q)
    mod = vq.ResidualLFQ(dim=12 if proj else d, num_quantizers=Q, codebook_size=2**d, quantize_dropout=Q > 1).to(DEV).eval()
    for shape, dtype in (((2, 65, Q), torch.int64), ((2, 3, 5, Q), torch.int32)):
        idx = _rand_idx(shape[0], shape[1] * (shape[2] if len(shape) == 4 else 1), Q, d, seed=Q, dtype=dtype).reshape(shape)
        for Qg in sorted({1, max(Q - 1, 1), Q}):
            given = idx[..., :Qg]
            codes, codes_plain = _both_paths(monkeypatch, lambda: mod.get_codes_from_indices(given))
            out, out_plain = _both_paths(monkeypatch, lambda: mod.get_output_from_indices(given))
            assert codes.shape == (Q, *shape[:-1], d) and torch.equal(codes, codes_plain) and _no_negative_zero(codes)
            assert out.shape == (*shape[:-1], 12 if proj else d) and torch.equal(out, out_plain)
            every, acc = _rule(given.reshape(1, -1, Qg), _mags(Q), d)
            assert torch.equal(codes.reshape(Q, 1, -1, d).cpu().double(), every)
            if not proj:
                assert torch.equal(out.reshape(1, -1, d).cpu().double(), acc) and _no_negative_zero(out)
    # the codes of a forward's indices are what the forward returns with them
    x = torch.randn(2, 65, 12 if proj else d, device=DEV)
    with torch.no_grad():
        q, i, _, all_codes = mod(x, return_all_codes=True)
        assert torch.equal(all_codes, mod.get_codes_from_indices(i))
        assert torch.equal(mod.get_output_from_indices(i), mod.project_out(all_codes.sum(dim=0)))


@pytest.mark.parametrize("proj", [False, True])
def test_grouped_residual_lfq(monkeypatch, proj):
    import vector_quantization as vq

    G, Q, d = 3, 3, 7
    torch.manual_seed(5)
    mod = vq.GroupedResidualLFQ(dim=G * (9 if proj else d), groups=G, num_quantizers=Q, codebook_size=2**d,
                                quantize_dropout=True).to(DEV).eval()
    for dtype in (torch.int64, torch.int32):
        idx = _rand_idx(G, 2 * 65, Q, d, seed=9, dtype=dtype).reshape(G, 2, 65, Q)
        for given in (idx, idx[..., :2], idx.permute(1, 2, 0, 3).contiguous().permute(2, 0, 1, 3)):
            codes, codes_plain = _both_paths(monkeypatch, lambda: mod.get_codes_from_indices(given))
            out, out_plain = _both_paths(monkeypatch, lambda: mod.get_output_from_indices(given))
            assert codes.shape == (G, Q, 2, 65, d) and torch.equal(codes, codes_plain) and _no_negative_zero(codes)
            assert out.shape == (2, 65, G * (9 if proj else d)) and torch.equal(out, out_plain)
            every, acc = _rule(given.reshape(G, -1, given.shape[-1]), _mags(Q), d)
            assert torch.equal(codes.reshape(G, Q, -1, d).cpu().double(), every.permute(1, 0, 2, 3))
            if not proj:
                assert torch.equal(out.reshape(-1, G, d).cpu().double(), acc.permute(1, 0, 2))


# the native call is taken: once per decode, once for ALL the groups of a GroupedResidualLFQ; never with the switch set
def test_one_native_call_per_decode(monkeypatch):
    import vector_quantization as vq
    from vector_quantization import search

    backend = search.get_backend()
    calls = []
    real = backend.lfq_decode

    def counting(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(backend, "lfq_decode", staticmethod(counting))
    monkeypatch.delenv("VQ_NO_FUSED_DECODE", raising=False)
    grouped = vq.GroupedResidualLFQ(dim=21, groups=3, num_quantizers=4, codebook_size=2**7).to(DEV).eval()
    rvq = vq.ResidualLFQ(dim=7, num_quantizers=4, codebook_size=2**7).to(DEV).eval()
    lfq = vq.LFQ(codebook_size=2**7, num_codebooks=3).to(DEV).eval()
    gi = torch.randint(0, 2**7, (3, 2, 67, 4), device=DEV)
    with torch.no_grad():
        grouped.get_output_from_indices(gi)
        assert len(calls) == 1
        grouped.get_codes_from_indices(gi)
        assert len(calls) == 2
        rvq.get_output_from_indices(gi[0])
        assert len(calls) == 3
        rvq.get_codes_from_indices(gi[0])
        assert len(calls) == 4
        lfq.indices_to_codes(gi[0, ..., :3])
        assert len(calls) == 5
        monkeypatch.setenv("VQ_NO_FUSED_DECODE", "1")
        grouped.get_output_from_indices(gi)
        grouped.get_codes_from_indices(gi)
        rvq.get_output_from_indices(gi[0])
        lfq.indices_to_codes(gi[0, ..., :3])
        assert len(calls) == 5


# the registered op: schema and fake implementation, equal to the native call, traceable without a graph break
def test_registered_op_and_compile():
    import torch._dynamo as dynamo

    import vector_quantization as vq
    from vector_quantization import native

    idx = _rand_idx(2, 133, 3, 7, seed=42)
    mag = list(_mags(4))
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.vq_mi355x.lfq_decode.default, (idx, mag, 7, True, True, True), test_utils=utils)
    s, a = torch.ops.vq_mi355x.lfq_decode(idx, mag, 7, True, True, True)
    s2, a2 = native.lfq_decode(idx, mag, 7, want_sum=True, want_all=True)
    assert torch.equal(s, s2) and torch.equal(a, a2)
    s, a = torch.ops.vq_mi355x.lfq_decode(idx, mag, 7, True, True, False)
    assert torch.equal(s, s2) and a.numel() == 0

    def fn(i):
        return torch.ops.vq_mi355x.lfq_decode(i, mag, 7, True, True, True)

    dynamo.reset()
    with torch.no_grad():
        cs, ca = torch.compile(fn, fullgraph=True)(idx)
    assert torch.equal(cs, s2) and torch.equal(ca, a2)

    # the modules' decode methods trace through it as well
    grouped = vq.GroupedResidualLFQ(dim=21, groups=3, num_quantizers=4, codebook_size=2**7).to(DEV).eval()
    lfq = vq.LFQ(codebook_size=2**7, num_codebooks=3).to(DEV).eval()
    gi = torch.randint(0, 2**7, (3, 2, 67, 4), device=DEV)
    with torch.no_grad():
        for method, arg in ((grouped.get_output_from_indices, gi), (grouped.get_codes_from_indices, gi),
                            (grouped.rvqs[0].get_output_from_indices, gi[0]), (lfq.indices_to_codes, gi[0, ..., :3])):
            dynamo.reset()
            assert torch.equal(torch.compile(method, backend="aot_eager", fullgraph=True)(arg), method(arg))
