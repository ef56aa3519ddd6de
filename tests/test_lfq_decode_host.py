"""CPU suite for the fused decode of the lookup-free family (vq_lfq_decode_f32): the symbol and its argument checks without a
device, the registered op's fake implementation, and the three modules on CPU tensors / with the CPU checker backend, which
keep the tensor-op expressions -- compared here against the bit rule written out in float64."""
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
    assert re.search(r"^int vq_lfq_decode_f32\(const void \*idx, int idx_64, int64_t idx_gs, int64_t idx_rs, int64_t idx_qs,", header,
                     re.M)
    assert "vq_lfq_decode_f32" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load(), "vq_lfq_decode_f32")
    assert callable(native.lfq_decode)


def test_cabi_argument_validation_without_a_device():
    from vector_quantization import native

    lib = native.load()
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its checks first
    mags = (ctypes.c_float * 3)(1.0, 0.5, 0.25)

    def call(idx=p, G=1, N=10, Qg=3, Q=3, d=4, mag=mags, s=p, a=p):
        return lib.vq_lfq_decode_f32(idx, 1, 0, Q, 1, G, N, Qg, Q, d, mag, 1, s, 0, d, 1, a, N * d, 0, d, None)

    def err():
        return lib.vq_last_error().decode()

    assert call(idx=None) == -1 and "vq_lfq_decode: " in err() and "null" in err()
    assert call(mag=None) == -1 and "null" in err()
    assert call(s=None, a=None) == -1 and "both outputs" in err()
    assert call(d=0) == -1 and "d must be" in err()
    assert call(d=native.LFQ_MAX_DIM + 1) == -1 and "d must be" in err()
    assert call(d=native.LFQ_MAX_DIM, N=0) == 0
    assert call(Qg=4) == -1 and "Q_given" in err()
    assert call(Qg=0) == -1 and "Q_given" in err()
    assert call(Q=0, Qg=0) == -1 and "Q must be" in err()
    assert call(Q=native.RLFQ_MAX_STAGES + 1, Qg=1) == -1 and "Q must be" in err()
    assert call(G=0) == -1 and call(G=65536) == -1 and call(N=-1) == -1
    assert call(N=2**40) == -1 and "too many" in err()
    assert call(N=0) == 0  # nothing to do, nothing launched
    assert call(N=0, s=None) == 0 and call(N=0, a=None) == 0


def test_op_has_a_fake_implementation():
    import vector_quantization  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        i = torch.empty((2, 100, 3), dtype=torch.int32)
        mag = [1.0, 0.5, 0.25, 0.125, 0.0625]
        s, a = torch.ops.vq_mi355x.lfq_decode(i, mag, 12, True, True, True)
        assert s.shape == (2, 100, 12) and a.shape == (5, 2, 100, 12) and s.dtype == a.dtype == torch.float32
        s, a = torch.ops.vq_mi355x.lfq_decode(i, mag, 12, True, True, False)
        assert s.shape == (2, 100, 12) and a.numel() == 0
        s, a = torch.ops.vq_mi355x.lfq_decode(i.long(), mag, 7, False, False, True)
        assert s.numel() == 0 and a.shape == (5, 2, 100, 7)


def test_native_call_refuses_cpu_tensors():
    from vector_quantization import native

    with pytest.raises(native.NativeUnavailable):
        native.lfq_decode(torch.zeros(1, 5, 2, dtype=torch.int64), (1.0, 0.5), 4)


def test_dispatch_rule_on_the_host(oracle):
    """CPU indices, the switch and a backend without the method all keep the tensor ops."""
    from vector_quantization import search

    i = torch.zeros((1, 4, 2), dtype=torch.int64)
    assert search.lfq_decode_backend(i) is None
    assert search.lfq_decode_backend([1, 2]) is None
    assert callable(getattr(search.get_backend(), "lfq_decode"))
    search.set_backend(OracleBackend)
    try:
        assert search.lfq_decode_backend(i) is None
    finally:
        search.set_backend(None)


# ---- the modules on the CPU: today's expressions, with the native backend (CPU tensors) and with the CPU checker backend
def _codes64(idx, d, mag, drop_null):
    """The bit rule in float64: idx [...] -> [..., d]; bit d-1-j of the low 32 bits picks the sign of dim j."""
    low = idx.to(torch.int64) & 0xFFFFFFFF
    shifts = torch.arange(d - 1, -1, -1)
    bits = (low[..., None] >> shifts) & 1
    codes = (bits.double() * 2 - 1) * mag
    if drop_null:
        codes = torch.where((idx == -1)[..., None], torch.zeros((), dtype=torch.float64), codes)
    return codes


@pytest.fixture(params=["native-backend", "checker-backend"])
def backend(request, oracle):
    from vector_quantization import search

    if request.param == "checker-backend":
        search.set_backend(OracleBackend)
    yield request.param
    search.set_backend(None)


@pytest.mark.parametrize("c,keep", [(1, False), (1, True), (3, True)])
@pytest.mark.parametrize("spherical", [False, True])
@pytest.mark.parametrize("channel_first", [False, True])
def test_lfq_on_cpu_keeps_the_expressions(backend, c, keep, spherical, channel_first):
    import vector_quantization as vq

    torch.manual_seed(0)
    d = 5
    mod = vq.LFQ(codebook_size=2**d, num_codebooks=c, keep_num_codebooks_dim=keep, codebook_scale=1.5, spherical=spherical,
                 channel_first=channel_first, has_projections=False).eval()
    idx = torch.randint(0, 2**d, (2, 7, c) if keep else (2, 7))
    idx.view(-1)[0] = -1  # no drop rule in LFQ: all bits set
    got = mod.indices_to_codes(idx)
    want = _codes64(idx if keep else idx[..., None], d, 1.5, False).float()  # [2, 7, c, d], +-1.5 exactly
    if spherical:  # the module's own fp32 arithmetic: l2norm per codebook, times the scale
        want = torch.nn.functional.normalize(want, p=2, dim=-1) * 1.5
    want = want.reshape(2, 7, c * d)
    if channel_first:
        want = want.movedim(-1, 1)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(got.abs(), torch.full_like(got, float(got.abs().flatten()[0])))


def test_residual_lfq_on_cpu_keeps_the_expressions(backend):
    import vector_quantization as vq

    torch.manual_seed(1)
    d, Q = 6, 4
    for dropout, dim in ((False, d), (True, d), (True, 10)):
        mod = vq.ResidualLFQ(dim=dim, num_quantizers=Q, codebook_size=2**d, quantize_dropout=dropout).eval()
        idx = torch.randint(0, 2**d, (2, 7, Q))
        idx[0, 3, 2:] = -1
        idx[1, 1, 0] = -1
        want = torch.stack([_codes64(idx[..., q], d, 2.0**-q, True) for q in range(Q)])
        got = mod.get_codes_from_indices(idx)
        assert got.dtype == torch.float32 and torch.equal(got.double(), want)
        assert torch.equal(mod.get_output_from_indices(idx), mod.project_out(want.sum(dim=0).float()))
        if dropout:
            want2 = want.clone()
            want2[2:] = 0.0
            assert torch.equal(mod.get_codes_from_indices(idx[..., :2]).double(), want2)
        else:
            with pytest.raises(AssertionError, match="quantize dropout must be greater than 0"):
                mod.get_codes_from_indices(idx[..., :2])
            with pytest.raises(AssertionError, match="quantize dropout must be greater than 0"):
                mod.get_output_from_indices(idx[..., :2])


@pytest.mark.parametrize("dim", [18, 24])
def test_grouped_residual_lfq_on_cpu_keeps_the_expressions(backend, dim):
    import vector_quantization as vq

    torch.manual_seed(2)
    d, Q, G = 6, 3, 3
    mod = vq.GroupedResidualLFQ(dim=dim, groups=G, num_quantizers=Q, codebook_size=2**d).eval()
    idx = torch.randint(0, 2**d, (G, 2, 5, Q))
    idx[1, 0, 0, 1] = -1
    per_group = [torch.stack([_codes64(idx[g, ..., q], d, 2.0**-q, True) for q in range(Q)]) for g in range(G)]
    got = mod.get_codes_from_indices(idx)
    assert got.shape == (G, Q, 2, 5, d) and torch.equal(got.double(), torch.stack(per_group))
    want_out = torch.cat([rvq.project_out(c.sum(dim=0).float()) for rvq, c in zip(mod.rvqs, per_group)], dim=-1)
    assert torch.equal(mod.get_output_from_indices(idx), want_out)
    assert torch.equal(mod.get_output_from_indices(tuple(idx)), want_out)  # a tuple of per-group indices, as zip() takes it
