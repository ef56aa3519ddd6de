"""vq_decode_f32 on the device: indices -> code vectors for VectorQuantize / ResidualVQ / GroupedResidualVQ.

The check is plain torch: ``all_codes`` is a bit copy of ``cb[q][idx]`` with dropped entries +0.0, ``codes_sum`` is the
explicit loop ``acc = acc + t_q`` from zeros -- each step one IEEE fp32 add, so the expected value is unique and every
comparison is ``torch.equal`` (no tolerance).  The modules are compared with themselves under VQ_NO_FUSED_DECODE=1."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rand_case(G, N, Q, K, D, *, seed=0, idx_dtype=torch.int64, drop_rate=0.15, Gc=None, Qc=None):
    g = torch.Generator().manual_seed(seed)
    cb = torch.randn((G if Gc is None else Gc, Q if Qc is None else Qc, K, D), generator=g)
    idx = torch.randint(0, K, (G, N, Q), generator=g)
    if drop_rate:
        idx[torch.rand((G, N, Q), generator=g) < drop_rate] = -1
    return cb.to(DEV), idx.to(idx_dtype).to(DEV)


def _expected(cb, idx, Q, drop_null=True):
    """(all [Q, G, N, D], sum [G, N, D]) by the definition, on the tensors' device."""
    G, N, Qg = idx.shape
    K, D = cb.shape[-2:]
    every = torch.zeros((Q, G, N, D), dtype=torch.float32, device=cb.device)
    for q in range(Qg):
        i = idx[..., q].long()
        if not drop_null:
            i = torch.where(i < 0, i + K, i)
        valid = (i >= 0) & (i < K)
        safe = torch.where(valid, i, torch.zeros_like(i))
        for gi in range(G):
            table = cb[gi if cb.shape[0] > 1 else 0, q if cb.shape[1] > 1 else 0]
            every[q, gi] = torch.where(valid[gi][:, None], table[safe[gi]], torch.zeros((), device=cb.device))
    acc = torch.zeros((G, N, D), dtype=torch.float32, device=cb.device)
    for q in range(Q):
        acc = acc + every[q]
    return every, acc


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(cb, idx, Q, drop_null=True, **kw):
    from vector_quantization import native

    s, a = native.decode_codes(cb, idx, num_stages=Q, drop_null=drop_null, want_sum=True, want_all=True, **kw)
    torch.cuda.synchronize()
    every, acc = _expected(cb, idx, Q, drop_null)
    assert torch.equal(_bits(a), _bits(every)), "all_codes are not bit copies of the codebook rows"
    assert torch.equal(s, acc), "codes_sum is not the left-to-right fp32 sum"
    return s, a


# 1. row widths: scalar path and tails, rows-per-access boundaries, the one-pass limit and the slice loop
@pytest.mark.parametrize("D", [1, 3, 4, 5, 28, 32, 36, 64, 100, 128, 132, 252, 256, 260, 512, 520, 1028])
def test_row_widths(D):
    cb, idx = _rand_case(1, 133, 3, 70, D, seed=D)
    _check(cb, idx, 3)


# 2. row counts: one row, partial and full accesses, several workgroups
@pytest.mark.parametrize("D", [48, 256])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000])
def test_row_counts(N, D):
    cb, idx = _rand_case(1, N, 3, 70, D, seed=N + D)
    _check(cb, idx, 3)


# 3. stage counts on both sides of the gather batch (4 stages); Q = 1 is the single-stage instantiation
@pytest.mark.parametrize("D", [64, 6])
@pytest.mark.parametrize("Q", [1, 2, 4, 5, 8, 9, 17])
def test_stage_counts(Q, D):
    cb, idx = _rand_case(1, 133, Q, 70, D, seed=Q)
    _check(cb, idx, Q)


# 4. codebook sizes, 5. groups
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 1000])
def test_codebook_sizes_and_groups(K, G):
    cb, idx = _rand_case(G, 133, 3, K, 64, seed=K + G)
    _check(cb, idx, 3)
    cb, idx = _rand_case(G, 37, 3, K, 7, seed=K + G)
    _check(cb, idx, 3)


# 6. outputs: sum only, all only, both
@pytest.mark.parametrize("D", [64, 5])
def test_each_output_alone(D):
    from vector_quantization import native

    cb, idx = _rand_case(2, 133, 5, 70, D, seed=11)
    every, acc = _expected(cb, idx, 5)
    s, a = native.decode_codes(cb, idx, want_sum=True, want_all=False)
    assert a is None and torch.equal(s, acc)
    s, a = native.decode_codes(cb, idx, want_sum=False, want_all=True)
    assert s is None and torch.equal(_bits(a), _bits(every))
    _check(cb, idx, 5)


# 7. index forms
@pytest.mark.parametrize("D", [64, 5])
def test_index_forms(D):
    from vector_quantization import native

    cb, idx = _rand_case(2, 133, 4, 70, D, seed=12)
    s64, a64 = _check(cb, idx, 4)
    s32, a32 = _check(cb, idx.to(torch.int32), 4)
    assert torch.equal(s64, s32) and torch.equal(a64, a32)
    # a [.., :2] view of the [G, N, 4] tensor, read in place: the same as -1 in the two missing stages
    view = idx[..., :2]
    assert not view.is_contiguous()
    padded = idx.clone()
    padded[..., 2:] = -1
    sv, av = native.decode_codes(cb, view, num_stages=4, want_sum=True, want_all=True)
    sp, ap = _check(cb, padded, 4)
    assert torch.equal(sv, sp) and torch.equal(_bits(av), _bits(ap))
    assert not av[2:].any()
    # one codebook for all stages (cb_qs = 0), and for all groups (cb_gs = 0)
    _check(cb[:, :1], idx, 4)
    _check(cb[:1, :1], idx, 4)


# 8. memory layouts
def test_memory_layouts():
    from vector_quantization import native

    G, N, Q, K, D = 2, 133, 3, 70, 64
    cb, idx = _rand_case(G, N, Q, K, D, seed=13)
    every, acc = _expected(cb, idx, Q)
    # codebooks that start 4 bytes into their buffer: no 16-byte accesses
    buf = torch.zeros(cb.numel() + 1, device=DEV)
    off = buf[1:].view(G, Q, K, D)
    off.copy_(cb)
    assert off.data_ptr() % 16 == 4
    _check(off, idx, Q)
    # an output whose row stride exceeds D: the gaps stay untouched
    wide = torch.full((G, N, D + 4), 7.0, device=DEV)
    native.decode_codes(cb, idx, sum_out=wide[..., :D])
    assert torch.equal(wide[..., :D], acc) and bool((wide[..., D:] == 7.0).all())
    wide_all = torch.full((Q, G, N, D + 8), 7.0, device=DEV)
    native.decode_codes(cb, idx, want_sum=False, want_all=True, all_out=wide_all[..., :D])
    assert torch.equal(wide_all[..., :D], every) and bool((wide_all[..., D:] == 7.0).all())
    # a channel-first output [G, D, N]
    cf = torch.empty((G, D, N), device=DEV)
    native.decode_codes(cb, idx, sum_out=cf.transpose(1, 2))
    assert torch.equal(cf, acc.transpose(1, 2))
    # the groups side by side on the feature axis [N, G * D] (multi-head concatenation: sum_gs = D)
    cat = torch.empty((N, G, D), device=DEV)
    native.decode_codes(cb, idx, sum_out=cat.transpose(0, 1))
    assert torch.equal(cat.reshape(N, G * D), torch.cat([acc[0], acc[1]], dim=-1))


# 9. index rule
@pytest.mark.parametrize("D", [64, 5])
def test_index_rule(D):
    from vector_quantization import native

    G, N, Q, K = 1, 133, 3, 70
    cb, idx = _rand_case(G, N, Q, K, D, seed=14)
    idx[0, 5] = -1           # every stage dropped
    idx[0, 6] = -7           # any negative index is a dropped stage
    idx[0, 9, 1] = 0         # code 0 really selected
    cb[:, 0, 0] = float("nan")
    cb[:, 1, 0] = float("inf")
    cb[:, 2, 0] = float("nan")
    s, a = native.decode_codes(cb, idx, want_sum=True, want_all=True)
    assert torch.equal(_bits(s[0, 5]), torch.zeros(D, dtype=torch.int32, device=DEV))  # exactly +0.0
    assert torch.equal(_bits(s[0, 6]), torch.zeros(D, dtype=torch.int32, device=DEV))
    assert torch.equal(_bits(a[:, 0, 5]), torch.zeros((Q, D), dtype=torch.int32, device=DEV))
    every, acc = _expected(cb, idx, Q)
    assert torch.equal(_bits(a), _bits(every))
    chose0 = idx == 0                                                        # [G, N, Q]
    assert torch.equal(a.isnan().any(dim=-1), (chose0 & torch.tensor([True, False, True], device=DEV)).permute(2, 0, 1))
    assert torch.equal(s.isnan(), acc.isnan())
    assert torch.equal(s.isnan().any(dim=-1), (chose0[..., 0] | chose0[..., 2]))
    assert torch.equal(torch.nan_to_num(s, nan=1.0), torch.nan_to_num(acc, nan=1.0))
    # drop_null = 0: ATen's indexing, -1 and -K wrap
    cb, idx = _rand_case(G, N, 1, K, D, seed=15, drop_rate=0)
    idx[0, 3, 0] = -1
    idx[0, 4, 0] = -K
    idx[0, 7, 0] = -K + 1
    s, _ = native.decode_codes(cb, idx, drop_null=False)
    assert torch.equal(s[0], cb[0, 0][idx[0, :, 0]])
    assert torch.equal(s[0, 3], cb[0, 0, K - 1]) and torch.equal(s[0, 4], cb[0, 0, 0])
    _check(cb, idx, 1, drop_null=False)


# 10. out-of-range indices: never an address, a zero code; every other row exact (an input check, run once per path)
@pytest.mark.parametrize("D", [64, 5])
def test_out_of_range_indices_give_zero_codes(D):
    G, N, Q, K = 1, 133, 3, 70
    cb, idx = _rand_case(G, N, Q, K, D, seed=16)
    idx[0, 2, 0] = K
    idx[0, 40, 1] = K + 5
    idx[0, 132, 2] = K
    s, a = _check(cb, idx, Q, drop_null=True)
    assert not a[0, 0, 2].any() and not a[1, 0, 40].any() and not a[2, 0, 132].any()
    cb1, idx1 = _rand_case(G, N, 1, K, D, seed=17, drop_rate=0)
    idx1[0, 2, 0] = K
    idx1[0, 40, 0] = K + 5
    idx1[0, 132, 0] = -K - 1
    s, _ = _check(cb1, idx1, 1, drop_null=False)
    assert not s[0, 2].any() and not s[0, 40].any() and not s[0, 132].any()


# ---- 11. the modules, against themselves under VQ_NO_FUSED_DECODE=1
def _params(K, **kw):
    from vector_quantization.codebooks import CodebookParams

    return CodebookParams(dim=1, codebook_size=K, **kw)


def _randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    from vector_quantization.codebook import Codebook

    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, Codebook):
                m.embeddings.copy_(torch.randn(m.embeddings.shape, generator=g))
    return mod.to(DEV).eval()


def _both_paths(monkeypatch, fn):
    native_out = fn()
    monkeypatch.setenv("VQ_NO_FUSED_DECODE", "1")
    plain_out = fn()
    monkeypatch.delenv("VQ_NO_FUSED_DECODE")
    return native_out, plain_out


def _left_to_right(codes):
    acc = torch.zeros_like(codes[0])
    for q in range(codes.shape[0]):
        acc = acc + codes[q]
    return acc


@pytest.mark.parametrize("variant", ["plain", "shared", "image", "projections", "coarse"])
def test_residual_vq_module(monkeypatch, variant):
    import vector_quantization as vq

    Q, K, d = 5, 70, 48
    mod = _randomise(vq.ResidualVQ(dim=40 if variant == "projections" else d, codebook_dim=d, num_quantizers=Q,
                                   shared_codebook=variant == "shared", quantize_dropout=variant == "coarse",
                                   codebook_params=_params(K)), 21)
    g = torch.Generator().manual_seed(22)
    idx = torch.randint(0, K, (2, 6, 11, Q) if variant == "image" else (2, 67, Q), generator=g)
    idx[torch.rand(idx.shape, generator=g) < 0.1] = -1
    idx = idx.to(DEV)
    if variant == "coarse":
        idx = idx[..., :2]
    with torch.no_grad():
        codes, codes_plain = _both_paths(monkeypatch, lambda: mod.get_codes_from_indices(idx))
        out, out_plain = _both_paths(monkeypatch, lambda: mod.get_output_from_indices(idx))
        assert codes.shape == codes_plain.shape == (Q, *idx.shape[:-1], d) and codes.dtype == codes_plain.dtype
        assert torch.equal(codes, codes_plain)
        assert out.shape == out_plain.shape
        torch.testing.assert_close(out, out_plain, rtol=1e-5, atol=1e-5)
        assert torch.equal(out, mod.project_out(_left_to_right(codes_plain)))


def test_residual_vq_output_equals_the_forward(monkeypatch):
    import vector_quantization as vq

    for shared in (False, True):
        mod = _randomise(vq.ResidualVQ(dim=48, num_quantizers=5, shared_codebook=shared, codebook_params=_params(70)), 23)
        x = torch.randn((2, 300, 48), generator=torch.Generator().manual_seed(24)).to(DEV)
        with torch.no_grad():
            quantized, idx, _ = mod(x)
            assert torch.equal(mod.get_output_from_indices(idx), quantized)
            q2, idx2, _, codes = mod(x, return_all_codes=True)  # picks the native path up through get_codes_from_indices
            assert torch.equal(_left_to_right(codes), q2)


@pytest.mark.parametrize("projections", [False, True])
def test_grouped_residual_vq_module(monkeypatch, projections):
    import vector_quantization as vq

    G, Q, K, d = 3, 4, 70, 16
    kw = dict(codebook_dim=8) if projections else {}
    mod = _randomise(vq.GroupedResidualVQ(dim=G * d, groups=G, num_quantizers=Q, codebook_params=_params(K), **kw), 25)
    g = torch.Generator().manual_seed(26)
    idx = torch.randint(0, K, (G, 2, 67, Q), generator=g)
    idx[torch.rand(idx.shape, generator=g) < 0.1] = -1
    idx = idx.to(DEV)
    with torch.no_grad():
        codes, codes_plain = _both_paths(monkeypatch, lambda: mod.get_codes_from_indices(idx))
        out, out_plain = _both_paths(monkeypatch, lambda: mod.get_output_from_indices(idx))
        assert codes.shape == codes_plain.shape and torch.equal(codes, codes_plain)
        assert out.shape == out_plain.shape == (2, 67, G * d)
        torch.testing.assert_close(out, out_plain, rtol=1e-5, atol=1e-5)
        want = torch.cat([rvq.project_out(_left_to_right(codes_plain[gi])) for gi, rvq in enumerate(mod.rvqs)], dim=-1)
        assert torch.equal(out, want)
        if not projections:
            x = torch.randn((2, 300, G * d), generator=g).to(DEV)
            quantized, fidx, _ = mod(x)
            assert torch.equal(mod.get_output_from_indices(fidx), quantized)


@pytest.mark.parametrize("heads,separate", [(1, False), (4, False), (4, True)])
@pytest.mark.parametrize("channel_last", [True, False])
@pytest.mark.parametrize("projections", [False, True])
def test_vector_quantize_module(monkeypatch, heads, separate, channel_last, projections):
    import vector_quantization as vq

    K, hd = 70, 12
    mod = _randomise(vq.VectorQuantize(dim=20 if projections else hd * heads, codebook_dim=hd, heads=heads,
                                       separate_codebook_per_head=separate, channel_last=channel_last,
                                       codebook_params=_params(K)), 27)
    g = torch.Generator().manual_seed(28)
    idx = torch.randint(0, K, (2, 67, heads) if heads > 1 else (2, 67), generator=g)
    idx[0, 0] = -1
    idx[1, 1] = -K
    idx = idx.to(DEV)
    with torch.no_grad():
        codes, codes_plain = _both_paths(monkeypatch, lambda: mod.get_codes_from_indices(idx))
        assert codes.shape == codes_plain.shape and torch.equal(codes, codes_plain)
        if heads > 1 and not separate and projections:
            return  # [b, n, h, d] codes do not fit project_out, with either path
        out, out_plain = _both_paths(monkeypatch, lambda: mod.get_output_from_indices(idx))
        assert out.shape == out_plain.shape and out.dtype == out_plain.dtype
        assert torch.equal(out, out_plain)  # one stage: no sum, so no order


def test_vector_quantize_image_indices_channel_first(monkeypatch):
    import vector_quantization as vq

    mod = _randomise(vq.VectorQuantize(dim=12, channel_last=False, codebook_params=_params(70)), 29)
    idx = torch.randint(0, 70, (2, 5, 9), generator=torch.Generator().manual_seed(30)).to(DEV)
    with torch.no_grad():
        out, out_plain = _both_paths(monkeypatch, lambda: mod.get_output_from_indices(idx))
        codes, codes_plain = _both_paths(monkeypatch, lambda: mod.get_codes_from_indices(idx))
    assert out.shape == out_plain.shape == (2, 12, 5, 9) and torch.equal(out, out_plain)
    assert torch.equal(codes, codes_plain)


# 12. the native call is taken: once per decode, also for all the groups of a uniform GroupedResidualVQ
def test_one_native_call_per_decode(monkeypatch):
    import vector_quantization as vq
    from vector_quantization import search

    backend = search.get_backend()
    calls = []
    real = backend.decode

    def counting(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(backend, "decode", staticmethod(counting))
    grouped = _randomise(vq.GroupedResidualVQ(dim=48, groups=3, num_quantizers=4, codebook_params=_params(70)), 31)
    rvq = _randomise(vq.ResidualVQ(dim=48, num_quantizers=4, codebook_params=_params(70)), 32)
    gi = torch.randint(0, 70, (3, 2, 67, 4), device=DEV)
    with torch.no_grad():
        grouped.get_output_from_indices(gi)
        assert len(calls) == 1
        grouped.get_codes_from_indices(gi)
        assert len(calls) == 2
        rvq.get_output_from_indices(gi[0])
        assert len(calls) == 3
        rvq.get_codes_from_indices(gi[0])
        assert len(calls) == 4
        # VectorQuantize: a codebook per head is one call for all heads; one shared codebook stays one gather (not dispatched)
        per_head = _randomise(vq.VectorQuantize(dim=48, codebook_dim=12, heads=4, separate_codebook_per_head=True,
                                                codebook_params=_params(70)), 46)
        shared = _randomise(vq.VectorQuantize(dim=48, codebook_params=_params(70)), 47)
        per_head.get_output_from_indices(gi[0])
        assert len(calls) == 5
        shared.get_output_from_indices(gi[0, ..., 0])
        assert len(calls) == 5
        monkeypatch.setenv("VQ_NO_FUSED_DECODE", "1")
        rvq.get_output_from_indices(gi[0])
        per_head.get_output_from_indices(gi[0])
        assert len(calls) == 5


# 13. nothing of [Q, N, D]
def test_output_from_indices_allocates_nothing_of_q_n_d(monkeypatch):
    import vector_quantization as vq

    N, Q, K, D = 65536, 8, 1024, 64
    mod = _randomise(vq.ResidualVQ(dim=D, num_quantizers=Q, codebook_params=_params(K)), 33)
    idx = torch.randint(0, K, (1, N, Q), device=DEV)
    mib = 1 << 20

    def rise():
        with torch.no_grad():
            mod.get_output_from_indices(idx[:, :64])  # (the stacked codebooks are built once, outside the measurement)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = mod.get_output_from_indices(idx)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
        assert out.shape == (1, N, D)
        return peak

    fused = rise()
    monkeypatch.setenv("VQ_NO_FUSED_DECODE", "1")
    plain = rise()
    print(f"peak rise: fused {fused / mib:.1f} MiB, tensor ops {plain / mib:.1f} MiB")
    assert fused < 64 * mib, fused
    assert plain > 128 * mib, plain


# 14. gradient to a learnable codebook: a scatter-add by index, exact on integer-valued gradients
@pytest.mark.parametrize("shared", [False, True])
def test_gradient_reaches_a_learnable_codebook(monkeypatch, shared):
    import vector_quantization as vq

    Q, K, D, N = 3, 7, 5, 200
    mod = vq.ResidualVQ(dim=D, num_quantizers=Q, shared_codebook=shared,
                        codebook_params=_params(K, learnable_codebook=True, ema_update=False))
    mod = _randomise(mod, 34)
    g = torch.Generator().manual_seed(35)
    idx = torch.randint(0, K, (1, N, Q), generator=g)
    idx[torch.rand(idx.shape, generator=g) < 0.2] = -1
    idx = idx.to(DEV)
    w_out = torch.randint(-3, 4, (1, N, D), generator=g).float().to(DEV)
    w_all = torch.randint(-3, 4, (Q, 1, N, D), generator=g).float().to(DEV)
    params = [p for p in mod.parameters() if p.requires_grad]
    assert params

    def grads():
        out = mod.get_output_from_indices(idx)
        codes = mod.get_codes_from_indices(idx)
        assert out.requires_grad and codes.requires_grad
        g_out = torch.autograd.grad((out * w_out).sum(), params)
        g_codes = torch.autograd.grad((codes * w_all).sum(), params)
        return g_out, g_codes

    (fo, fc), (po, pc) = _both_paths(monkeypatch, grads)
    for a, b in zip(fo + fc, po + pc):
        assert a.shape == b.shape and torch.equal(a, b)
        assert bool(a.any())


def test_gradient_vector_quantize_heads(monkeypatch):
    import vector_quantization as vq

    for separate in (False, True):
        mod = _randomise(vq.VectorQuantize(dim=20, codebook_dim=5, heads=4, separate_codebook_per_head=separate,
                                           codebook_params=_params(7, learnable_codebook=True, ema_update=False)), 36)
        g = torch.Generator().manual_seed(37)
        idx = torch.randint(-7, 7, (2, 50, 4), generator=g).to(DEV)
        params = [mod._codebook.embeddings]

        def grads():
            codes = mod.get_codes_from_indices(idx)
            w = torch.randint(-3, 4, codes.shape, generator=torch.Generator().manual_seed(38)).float().to(DEV)
            return torch.autograd.grad((codes * w).sum(), params)

        (fg,), (pg,) = _both_paths(monkeypatch, grads)
        assert torch.equal(fg, pg) and bool(fg.any())


# 15. one decode call captured in a graph, replayed on fresh indices written into the captured buffer
def test_decode_is_capturable():
    from vector_quantization import native

    G, N, Q, K, D = 1, 300, 4, 70, 64
    cb, idx = _rand_case(G, N, Q, K, D, seed=39)
    static_idx = idx.clone()
    s = torch.empty((G, N, D), device=DEV)
    a = torch.empty((Q, G, N, D), device=DEV)
    native.decode_codes(cb, static_idx, want_sum=True, want_all=True, sum_out=s, all_out=a)  # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        native.decode_codes(cb, static_idx, want_sum=True, want_all=True, sum_out=s, all_out=a)
    for seed in (40, 41):
        _, fresh = _rand_case(G, N, Q, K, D, seed=seed)
        static_idx.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        every, acc = _expected(cb, fresh, Q)
        assert torch.equal(s, acc) and torch.equal(_bits(a), _bits(every))


# the registered op: schema, fake implementation, the real call, its autograd registration, and a traced module
def test_registered_op(monkeypatch):
    import torch._dynamo as dynamo

    import vector_quantization as vq
    from vector_quantization import native

    cb, idx = _rand_case(2, 133, 3, 7, 8, seed=42)
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.vq_mi355x.decode_codes.default, (cb, idx, 3, True, True, True), test_utils=utils)
    s, a = torch.ops.vq_mi355x.decode_codes(cb, idx, 3, True, True, True)
    s2, a2 = native.decode_codes(cb, idx, want_sum=True, want_all=True)
    assert torch.equal(s, s2) and torch.equal(a, a2)
    s, a = torch.ops.vq_mi355x.decode_codes(cb, idx, 3, True, True, False)
    assert torch.equal(s, s2) and a.numel() == 0
    # gradient: integer-valued upstream gradients, against the definition differentiated by autograd
    w_s = torch.randint(-3, 4, s2.shape, generator=torch.Generator().manual_seed(43)).float().to(DEV)
    w_a = torch.randint(-3, 4, a2.shape, generator=torch.Generator().manual_seed(44)).float().to(DEV)
    leaf = cb.clone().requires_grad_()
    s, a = torch.ops.vq_mi355x.decode_codes(leaf, idx, 3, True, True, True)
    (got,) = torch.autograd.grad((s * w_s).sum() + (a * w_a).sum(), leaf)
    ref = cb.clone().requires_grad_()
    dropped = idx < 0
    terms = [torch.stack([ref[gi, q][idx[gi, :, q].clamp(min=0)] for gi in range(2)]).masked_fill(dropped[..., q, None], 0.0)
             for q in range(3)]
    (want,) = torch.autograd.grad(sum((t * (w_s + w_a[q])).sum() for q, t in enumerate(terms)), ref)
    assert torch.equal(got, want) and bool(got.any())
    # a module decode traced without a graph break goes through the op
    mod = _randomise(vq.ResidualVQ(dim=48, num_quantizers=4, codebook_params=_params(70)), 45)
    midx = torch.randint(0, 70, (2, 67, 4), device=DEV)
    dynamo.reset()
    with torch.no_grad():
        eager = mod.get_output_from_indices(midx)
        gm, _guards = dynamo.export(mod.get_output_from_indices)(midx)  # export = fullgraph: any graph break raises
        targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
        assert any("vq_mi355x.decode_codes" in t for t in targets), targets
        assert torch.equal(gm(midx), eager)
    dynamo.reset()
