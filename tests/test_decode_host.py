"""CPU suite for the fused decode (vq_decode_f32): the symbol and its argument checks without a device, the registered op's
fake implementation, and the three modules on CPU tensors / with the CPU checker backend, which keep the tensor-op
expressions -- compared here against those expressions written out."""
from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from helpers import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_symbol():
    from vector_quantization import native

    with open(os.path.join(ROOT, "include", "vq_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"^int vq_decode_f32\(const float \*cb, int64_t cb_gs, int64_t cb_qs, int G, int Q, int K, int D,", header, re.M)
    assert "vq_decode_f32" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load(), "vq_decode_f32")
    assert callable(native.decode_codes)


def test_cabi_argument_validation_without_a_device():
    from vector_quantization import native

    lib = native.load()
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its checks first

    def call(cb=p, G=1, Q=3, K=8, D=4, idx=p, N=10, Qg=3, s=p, a=p):
        return lib.vq_decode_f32(cb, 0, K * D, G, Q, K, D, idx, 1, 0, Q, 1, N, Qg, 1, s, 0, D, 1, a, N * D, 0, D, None)

    def err():
        return lib.vq_last_error().decode()

    assert call(cb=None) == -1 and "null" in err()
    assert call(idx=None) == -1 and "null" in err()
    assert call(s=None, a=None) == -1 and "both outputs" in err()
    assert call(Qg=4) == -1 and "Q_given" in err()
    assert call(Qg=0) == -1 and "Q_given" in err()
    for kw in (dict(K=0), dict(K=-1), dict(D=0), dict(Q=0, Qg=0), dict(G=0), dict(N=-1)):
        assert call(**kw) == -1 and "non-positive" in err(), kw
    assert call(N=2**62) == -1 and "too many" in err()
    assert call(N=0) == 0  # nothing to do, nothing launched


def test_op_has_a_fake_implementation():
    import vector_quantization  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        cb = torch.empty((2, 5, 70, 12))
        i = torch.empty((2, 100, 3), dtype=torch.int32)
        s, a = torch.ops.vq_mi355x.decode_codes(cb, i, 5, True, True, True)
        assert s.shape == (2, 100, 12) and a.shape == (5, 2, 100, 12) and s.dtype == a.dtype == torch.float32
        s, a = torch.ops.vq_mi355x.decode_codes(cb, i, 5, True, True, False)
        assert s.shape == (2, 100, 12) and a.numel() == 0
        s, a = torch.ops.vq_mi355x.decode_codes(cb[:1, :1], i.long(), 5, False, False, True)
        assert s.numel() == 0 and a.shape == (5, 2, 100, 12)


def test_native_call_refuses_cpu_tensors():
    from vector_quantization import native

    with pytest.raises(native.NativeUnavailable):
        native.decode_codes(torch.zeros(1, 2, 8, 4), torch.zeros(1, 5, 2, dtype=torch.int64))


# ---- the modules on the CPU: today's expressions, with the native backend (CPU tensors) and with the CPU checker backend
def _params(K, **kw):
    from vector_quantization.codebooks import CodebookParams

    return CodebookParams(dim=1, codebook_size=K, **kw)


def _rvq_expected(books, indices, Q):
    """[Q, b, ..., D]: gather per stage, dropped stages (index < 0, or not given) zero."""
    if indices.shape[-1] < Q:
        indices = torch.cat([indices, indices.new_full((*indices.shape[:-1], Q - indices.shape[-1]), -1)], dim=-1)
    per_stage = []
    for q in range(Q):
        i = indices[..., q]
        per_stage.append(torch.where((i < 0)[..., None], torch.zeros(()), books[q][i.clamp(min=0)]))
    return torch.stack(per_stage, dim=0)


@pytest.fixture(params=["native-backend", "checker-backend"])
def backend(request, oracle):
    from vector_quantization import search

    if request.param == "checker-backend":
        search.set_backend(OracleBackend)
    yield request.param
    search.set_backend(None)


def test_residual_vq_on_cpu_keeps_the_expressions(backend):
    import vector_quantization as vq

    torch.manual_seed(0)
    for shared, dropout in ((False, False), (True, False), (False, True)):
        mod = vq.ResidualVQ(dim=12, num_quantizers=4, codebook_dim=8, shared_codebook=shared, quantize_dropout=dropout,
                            codebook_params=_params(19)).eval()
        idx = torch.randint(0, 19, (2, 7, 4))
        idx[0, 3, 2:] = -1
        books = mod.codebooks
        want = _rvq_expected(books, idx, 4)
        assert torch.equal(mod.get_codes_from_indices(idx), want)
        assert torch.equal(mod.get_output_from_indices(idx), mod.project_out(want.sum(dim=0)))
        if dropout:
            want2 = _rvq_expected(books, idx[..., :2], 4)
            assert torch.equal(mod.get_codes_from_indices(idx[..., :2]), want2)
        else:
            with pytest.raises(AssertionError, match="quantize dropout must be greater than 0"):
                mod.get_codes_from_indices(idx[..., :2])
            with pytest.raises(AssertionError, match="quantize dropout must be greater than 0"):
                mod.get_output_from_indices(idx[..., :2])


def test_grouped_residual_vq_on_cpu_keeps_the_expressions(backend):
    import vector_quantization as vq

    torch.manual_seed(1)
    mod = vq.GroupedResidualVQ(dim=24, groups=3, num_quantizers=2, codebook_params=_params(11)).eval()
    idx = torch.randint(0, 11, (3, 2, 5, 2))
    idx[1, 0, 0, 1] = -1
    books = mod.codebooks  # [G, Q, K, d]
    per_group = [_rvq_expected(books[g], idx[g], 2) for g in range(3)]
    assert torch.equal(mod.get_codes_from_indices(idx), torch.stack(per_group))
    assert torch.equal(mod.get_output_from_indices(idx), torch.cat([c.sum(dim=0) for c in per_group], dim=-1))


@pytest.mark.parametrize("heads,separate", [(1, False), (4, False), (4, True)])
@pytest.mark.parametrize("channel_last", [True, False])
@pytest.mark.parametrize("projections", [False, True])
def test_vector_quantize_on_cpu_keeps_the_expressions(backend, heads, separate, channel_last, projections):
    import vector_quantization as vq

    torch.manual_seed(2)
    hd = 6
    dim = 10 if projections else hd * heads
    mod = vq.VectorQuantize(dim=dim, codebook_dim=hd, heads=heads, separate_codebook_per_head=separate,
                            channel_last=channel_last, codebook_params=_params(13)).eval()
    idx = torch.randint(0, 13, (2, 9, heads) if heads > 1 else (2, 9))
    idx[0, 0] = -1  # ATen's rule: the last code
    codes = mod.codebook
    if codes.ndim == 2:
        want = codes[idx]
    else:
        want = torch.cat([codes[h][idx[..., h]] for h in range(heads)], dim=-1)
    got = mod.get_codes_from_indices(idx)
    assert torch.equal(got, want if channel_last else want.movedim(-1, 1))
    if heads > 1 and not separate:
        if projections:
            return  # [b, n, h, d] does not fit project_out: an error today as well
    out = mod.get_output_from_indices(idx)
    assert torch.equal(out, mod.project_out(want) if channel_last else mod.project_out(want).movedim(-1, 1))
