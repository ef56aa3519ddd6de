"""LFQ without a GPU: import surface, constructor checks, indices_to_codes against the reference fixtures, the dense
fp64 restatement (tests/lfq_dense.py) against the same fixtures, and the no-CPU-fallback rule."""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
FIXTURES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(DATA, "lfq_*.npz")))


def load_fixture(name):
    f = np.load(os.path.join(DATA, f"lfq_{name}.npz"))
    return f, json.loads(str(f["config"]))


def build_module(f, c):
    from vector_quantization import LFQ

    mod = LFQ(**c["kwargs"])
    sd = {k[2:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("w_")}
    missing, unexpected = mod.load_state_dict(sd, strict=False)
    assert not unexpected and all(not k.startswith("project_") for k in missing)
    return mod.train(c.get("train", True))


def test_fixtures_present():
    assert len(FIXTURES) >= 15


def test_import_surface():
    import vector_quantization
    from vector_quantization import LFQ
    from vector_quantization.lookup_free_quantization import LFQ as LFQ2, CosineSimLinear, LossBreakdown, Return

    assert LFQ is LFQ2 and "LFQ" in vector_quantization.__all__
    assert Return._fields == ("quantized", "indices", "entropy_aux_loss")
    assert LossBreakdown._fields == ("per_sample_entropy", "batch_entropy", "commitment")
    assert isinstance(LFQ(dim=8, codebook_size=16, cosine_sim_project_in=True).project_in, CosineSimLinear)


def test_constructor_checks():
    from vector_quantization import LFQ

    with pytest.raises(AssertionError):
        LFQ()
    with pytest.raises(AssertionError, match="power of 2"):
        LFQ(codebook_size=100)
    with pytest.raises(AssertionError):
        LFQ(codebook_size=16, soft_clamp_input_value=0.5, codebook_scale=1.0)
    for frac in (0.0, -0.1, 1.5):
        with pytest.raises(AssertionError):
            LFQ(codebook_size=16, frac_per_sample_entropy=frac)
    with pytest.raises(AssertionError):
        LFQ(codebook_size=16, num_codebooks=2, keep_num_codebooks_dim=False)
    with pytest.raises(ValueError, match="20"):
        LFQ(codebook_size=2**21)
    m = LFQ(codebook_size=2**20)
    assert m.codebook_dim == 20 and m.dim == 20 and not m.has_projections
    m = LFQ(dim=32, codebook_size=2**12, num_codebooks=2)
    assert m.keep_num_codebooks_dim and m.has_projections and m.project_in.out_features == 24
    assert m.mask.tolist() == [2**i for i in range(11, -1, -1)]


@pytest.mark.parametrize("name", FIXTURES)
def test_indices_to_codes_against_fixture(name):
    f, c = load_fixture(name)
    mod = build_module(f, c)
    idx = torch.from_numpy(f["idx"])
    with torch.no_grad():
        codes = mod.indices_to_codes(idx)
    want = torch.from_numpy(f["out"])
    assert codes.shape == want.shape
    if not mod.has_projections and not mod.training:
        assert torch.equal(codes, want)
    else:
        # training output is x + (q - x), within an ulp of q (and of project_out(q) up to the matmul's rounding)
        torch.testing.assert_close(codes, want, rtol=1e-5, atol=1e-6)


def test_indices_to_codes_bits_msb_first():
    from vector_quantization import LFQ

    m = LFQ(codebook_size=16, codebook_scale=2.0)
    codes = m.indices_to_codes(torch.tensor([0, 1, 8, 15]))
    assert codes.tolist() == [[-2.0, -2.0, -2.0, -2.0], [-2.0, -2.0, -2.0, 2.0], [2.0, -2.0, -2.0, -2.0], [2.0] * 4]
    sph = LFQ(codebook_size=16, spherical=True)
    assert torch.allclose(sph.indices_to_codes(torch.tensor([5])).abs(), torch.full((1, 4), 0.5))


# plain configurations (no projection, clamp, l2norm or mask): v is x itself
_PLAIN = [n for n in ("d1", "d4", "d9_c2", "d12", "d16", "d16_t100", "d16_c2_nocommit") if n in FIXTURES]


@pytest.mark.parametrize("name", _PLAIN)
def test_dense_restatement_against_fixture(name):
    from lfq_dense import dense_entropy

    f, c = load_fixture(name)
    kw = c["kwargs"]
    C = kw.get("num_codebooks", 1)
    x = torch.from_numpy(f["x"]).double()
    d = x.shape[-1] // C
    v = x.reshape(-1, C, d)
    gamma = kw.get("diversity_gamma", 1.0)
    res = dense_entropy(v, None, kw.get("codebook_scale", 1.0), c.get("tau", 100.0), g_ps=1.0, g_cb=-gamma)
    np.testing.assert_allclose(float(res["per_sample"]), float(f["ps"]), rtol=1e-5)
    np.testing.assert_allclose(float(res["codebook"]), float(f["cb"]), rtol=1e-5)
    # dL/dx of aux.sum() + (out * r).sum(): entropy weight * the restatement's gradient + commitment + r (straight-through)
    q = torch.where(v > 0, 1.0, -1.0).double() * kw.get("codebook_scale", 1.0)
    cw = kw.get("commitment_loss_weight", 0.25)
    grad = 0.1 * res["grad"] + cw * 2.0 * (v - q) / v.numel() + torch.from_numpy(f["r"]).double().reshape(v.shape)
    np.testing.assert_allclose(grad.reshape(f["grad"].shape).numpy(), f["grad"], rtol=1e-4, atol=1e-6)


def test_cpu_tensors_raise_native_unavailable():
    from vector_quantization import LFQ, native

    m = LFQ(codebook_size=16)
    for training in (True, False):
        with pytest.raises(native.NativeUnavailable):
            m.train(training)(torch.randn(2, 5, 4))
    v = torch.randn(8, 1, 4)
    with pytest.raises(native.NativeUnavailable):
        native.lfq_quantize(v, 1.0)
    with pytest.raises(native.NativeUnavailable):
        native.lfq_entropy_forward(v, None, 1.0, 1.0)
    with pytest.raises(native.NativeUnavailable):
        native.lfq_entropy_backward(v, None, 1.0, 1.0, torch.ones(()), torch.ones(1, 16))


def test_workspace_bytes_bound():
    """The library's workspace stays within O(R * C * 2^ceil(d/2) + C * 2^d) (no [R, 2^d] buffer)."""
    from vector_quantization import native

    lib = native.load()
    for d in (1, 4, 9, 16, 20):
        for R in (1, 4096, 32768):
            for C in (1, 2):
                nbytes = lib.vq_lfq_workspace_bytes(R, R, C, d)
                bound = 8 * (R * C * (2 * 2 ** ((d + 1) // 2) + 1) + C * (2**d + 2**18) + R * C) + 5 * 256
                assert 0 < nbytes <= bound, (d, R, C, nbytes, bound)
    assert lib.vq_lfq_workspace_bytes(16, 16, 1, 21) == 0
    assert lib.vq_lfq_workspace_bytes(16, 16, 0, 4) == 0
