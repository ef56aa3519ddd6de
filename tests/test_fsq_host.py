"""FSQ / ResidualFSQ / GroupedResidualFSQ without a GPU: import surface, constructor checks, attributes, buffers and
state_dict against the reference fixtures (tests/golden/data/fsq_*.npz, rfsq_*.npz), the index helpers on CPU, the numpy
restatement of the kernel's index expression (tests/fsq_dense.py) against every fixture and against torch's CPU sum, the
fp64 restatement against the fixtures, the no-CPU-fallback rule, the C-ABI argument checks and the fake implementations."""
from __future__ import annotations

import ctypes
import glob
import json
import os
import random

import numpy as np
import pytest
import torch

from fsq_dense import indices_np, restate, torch_sum_order_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DATA, "fsq_*.npz")) + glob.glob(os.path.join(DATA, "rfsq_*.npz")))


def load_fixture(name):
    f = np.load(os.path.join(DATA, f"{name}.npz"))
    return f, json.loads(str(f["config"]))


def build_module(f, c):
    from vector_quantization import FSQ, GroupedResidualFSQ, ResidualFSQ

    cls = dict(fsq=FSQ, rfsq=ResidualFSQ, grfsq=GroupedResidualFSQ)[c["kind"]]
    mod = cls(**c["kwargs"])
    sd = {k[3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd_") and k != "sd_keys"}
    mod.load_state_dict(sd, strict=True)
    return mod.train(c.get("train", True))


def fixture_input(f, c):
    x = torch.from_numpy(f["x"])
    return x.to(getattr(torch, c.get("dtype", "float32")))


def test_fixtures_present():
    assert len([n for n in FIXTURES if n.startswith("fsq_")]) >= 13
    assert len([n for n in FIXTURES if n.startswith("rfsq_")]) >= 15


def test_import_surface():
    import vector_quantization
    from vector_quantization import FSQ, GroupedResidualFSQ, ResidualFSQ
    from vector_quantization.finite_scalar_quantization import FSQ as F2, round_ste
    from vector_quantization.residual_fsq import GroupedResidualFSQ as G2, ResidualFSQ as R2

    assert FSQ is F2 and ResidualFSQ is R2 and GroupedResidualFSQ is G2
    for name in ("FSQ", "ResidualFSQ", "GroupedResidualFSQ"):
        assert name in vector_quantization.__all__
    x = torch.tensor([0.4, 0.6, -1.5], requires_grad=True)
    y = round_ste(x)
    y.sum().backward()
    assert y.tolist() == [0.0, 1.0, -2.0] and x.grad.tolist() == [1.0, 1.0, 1.0]
    m = ResidualFSQ(dim=4, levels=[8, 5, 5, 5], num_quantizers=2)
    assert all(isinstance(layer, FSQ) for layer in m.layers)


def test_constructor_checks_and_attributes():
    from torch import nn

    from vector_quantization import FSQ, GroupedResidualFSQ, ResidualFSQ

    for bad in ([8, 1, 5], [0], [8, -3]):
        with pytest.raises(ValueError):
            FSQ(bad)
        with pytest.raises(ValueError):
            ResidualFSQ(dim=len(bad), levels=bad, num_quantizers=2)
    assert FSQ([8, 5], num_codebooks=2, keep_num_codebooks_dim=False).keep_num_codebooks_dim  # as the reference
    m = FSQ([8, 5, 5, 5])
    assert (m.codebook_dim, m.num_codebooks, m.effective_codebook_dim, m.dim) == (4, 1, 4, 4)
    assert m.codebook_size == 1000 and not m.has_projections and not m.keep_num_codebooks_dim
    assert isinstance(m.project_in, nn.Identity) and m.return_indices and not m.channel_first
    assert m.allowed_dtypes == (torch.float32, torch.float64)
    assert m._levels.dtype == torch.int32 and m._basis.tolist() == [1, 8, 40, 200]
    assert m.implicit_codebook.shape == (1000, 4) and m.implicit_codebook.dtype == torch.float32
    assert sorted(k for k, _ in m.named_buffers()) == ["_basis", "_levels", "implicit_codebook"]
    assert m.state_dict() == {}
    m2 = FSQ([8, 5, 5, 5], dim=16, num_codebooks=2, projection_has_bias=False)
    assert m2.keep_num_codebooks_dim and m2.has_projections and m2.project_in.bias is None
    assert sorted(m2.state_dict()) == ["project_in.weight", "project_out.weight"]
    m3 = FSQ([8, 5, 5, 5], return_indices=False)
    assert not hasattr(m3, "implicit_codebook") and not hasattr(m3, "codebook_size")
    r = ResidualFSQ(dim=4, levels=[8, 5, 5, 5], num_quantizers=3, quantize_dropout=True)
    assert r.scales.shape == (3, 4) and r.scales.dtype == torch.float32 and r.codebook_size == 1000
    assert torch.equal(r.scales[2], (torch.tensor([8.0, 5, 5, 5]) - 1) ** -2)
    assert r.quantize_dropout and r.levels == [8, 5, 5, 5] and r.state_dict() == {}
    assert r.codebooks.shape == (3, 1000, 4)
    g = GroupedResidualFSQ(dim=32, groups=2, levels=[8, 5, 5, 5], num_quantizers=2)
    assert g.codebook_size == 1000 and g.split_dim == -1 and g.codebooks.shape == (2, 2, 1000, 4)
    assert sorted(g.state_dict()) == sorted(f"rvqs.{i}.{p}.{w}" for i in range(2) for p in ("project_in", "project_out")
                                            for w in ("weight", "bias"))


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_matches_reference(name):
    f, c = load_fixture(name)
    mod = build_module(f, c)
    keys = json.loads(str(f["sd_keys"]))
    assert [[k, list(t.shape), str(t.dtype)] for k, t in mod.state_dict().items()] == keys


@pytest.mark.parametrize("name", FIXTURES)
def test_index_helpers_against_fixture(name):
    f, c = load_fixture(name)
    mod = build_module(f, c)
    if c["kind"] == "fsq":
        if "idx_valid" not in f.files:
            return
        idx = torch.from_numpy(f["idx_valid"])
        assert torch.equal(mod.indices_to_level_indices(idx), torch.from_numpy(f["level_idx"]))
        with torch.no_grad():
            got = mod.indices_to_codes(idx)
        np.testing.assert_array_equal(got.float().numpy(), f["codes_from_idx"]) if not mod.has_projections else \
            np.testing.assert_allclose(got.numpy(), f["codes_from_idx"], rtol=1e-6, atol=1e-7)
        return
    idx = torch.from_numpy(f["idx"])
    with torch.no_grad():
        np.testing.assert_allclose(mod.get_output_from_indices(idx).numpy(), f["from_idx"], rtol=1e-6, atol=1e-7)
        if "all_codes" in f.files:
            codes = mod.get_codes_from_indices(idx)
            assert torch.equal(codes, torch.from_numpy(f["all_codes"]))
        if "from_idx_pad" in f.files:
            np.testing.assert_allclose(mod.get_output_from_indices(idx[..., :2]).numpy(), f["from_idx_pad"], rtol=1e-6,
                                       atol=1e-7)


@pytest.mark.parametrize("name", [n for n in FIXTURES if n.startswith("fsq_")])
def test_index_restatement_reproduces_fixture(name):
    """The kernel's index expression (numpy fp32, torch's summation order) gives the reference's indices, collisions
    included: the codes are recovered exactly from the reference's own level indices where the index is valid."""
    f, c = load_fixture(name)
    if "idx" not in f.files:
        return
    mod = build_module(f, c)
    levels = c["kwargs"]["levels"]
    x = fixture_input(f, c)
    if c["kwargs"].get("channel_first"):
        x = x.movedim(1, -1)
    with torch.no_grad():
        feats = mod.project_in(x.reshape(x.shape[0], -1, x.shape[-1]))
        feats = feats.reshape(*feats.shape[:2], mod.num_codebooks, mod.codebook_dim)
        if feats.dtype not in mod.allowed_dtypes:
            feats = feats.float()
        codes = mod.quantize(feats).float()
    got = indices_np(codes.numpy(), levels)
    want = f["idx"].reshape(got.shape)
    assert np.array_equal(got, want)
    if c.get("collide"):
        # the collision: some valid code maps below its integer index sum_i k_i * basis_i
        k = np.rint(codes.double().numpy() * (np.array(levels) // 2) + np.array(levels) // 2).astype(np.int64)
        exact = (k * np.cumprod([1] + levels[:-1])).sum(-1)
        assert (got < exact).any() and not (got > exact).any()


def test_collision_levels():
    """FSQ([26]) maps code 6 to index 5 (25 distinct indices); [27, 5] and [1000] have one collision each."""
    from vector_quantization import FSQ

    for levels, n_distinct in (([26], 25), ([27, 5], 134), ([1000], 999), ([8, 5, 5, 5], 1000)):
        m = FSQ(levels)
        idx = m.codes_to_indices(m.implicit_codebook)
        assert len(torch.unique(idx)) == n_distinct, levels
        assert np.array_equal(indices_np(m.implicit_codebook.numpy(), levels), idx.numpy())
    m = FSQ([26])
    assert int(m.codes_to_indices(m.implicit_codebook[6:7])) == 5


@pytest.mark.parametrize("d", range(1, 8))
def test_sum_order_reproduces_torch_cpu_sum(d):
    rng = np.random.default_rng(d)
    t = (rng.standard_normal((200_000, d)) * rng.choice([1.0, 100.0, 1e4], size=(200_000, 1))).astype(np.float32)
    want = torch.from_numpy(t).sum(-1).numpy()
    assert np.array_equal(torch_sum_order_np(t).view(np.uint32), want.view(np.uint32))


def test_nan_index_is_int32_min():
    f, c = load_fixture("fsq_nonfinite")
    idx = f["idx"].reshape(-1)
    assert idx[0] == np.iinfo(np.int32).min and idx[1] >= 0 and idx[2] >= 0
    out = f["out"][0]
    assert np.isnan(out[0, 1]) and np.isfinite(out[0, [0, 2, 3]]).all() and np.isfinite(out[1:]).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_dense_restatement_against_fixture(name):
    f, c = load_fixture(name)
    sd = {k[3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd_") and k != "sd_keys"}
    x = fixture_input(f, c)
    stages = None
    if c["kind"] != "fsq":
        idx = f["idx"]
        stages = int((idx.reshape(-1, idx.shape[-1]) != -1).any(0).sum())
    st = restate(c["kind"], c["kwargs"], sd, x, torch.from_numpy(f["r"]), stages)
    np.testing.assert_array_equal(st["grad"].numpy(), f["grad64"])
    fin = np.isfinite(f["grad64"]) & np.isfinite(f["x"]).all(axis=-1 if not c["kwargs"].get("channel_first") else 1,
                                                             keepdims=True)
    np.testing.assert_allclose(f["grad"][fin], f["grad64"][fin], rtol=0, atol=float(f["grad_ref_dev"]) * 1.0000001)
    assert float(f["margin"]) >= 1e-4
    np.testing.assert_allclose(f["out"], st["out"].numpy(), rtol=1e-2 if c.get("dtype") == "bfloat16" else 1e-5, atol=1e-5,
                               equal_nan=True)


def test_cpu_forward_raises_native_unavailable():
    from vector_quantization import FSQ, GroupedResidualFSQ, ResidualFSQ, native

    for mod in (FSQ([8, 5, 5, 5]), ResidualFSQ(dim=4, levels=[8, 5, 5, 5], num_quantizers=3),
                GroupedResidualFSQ(dim=8, groups=2, levels=[8, 5, 5, 5], num_quantizers=2)):
        for training in (True, False):
            with pytest.raises(native.NativeUnavailable):
                mod.train(training)(torch.randn(2, 5, mod.dim if hasattr(mod, "dim") and isinstance(mod.dim, int) else 4))
    with pytest.raises(native.NativeUnavailable):
        FSQ([8, 5, 5, 5])(torch.randn(2, 5, 4, dtype=torch.float64))
    x = torch.randn(1, 8, 4)
    k = torch.zeros(4, 4)
    with pytest.raises(native.NativeUnavailable):
        native.fsq_quantize(x, [8, 5, 5, 5], k)
    with pytest.raises(native.NativeUnavailable):
        native.fsq_backward(x, [8, 5, 5, 5], k, x)
    with pytest.raises(native.NativeUnavailable):
        native.fsq_decode(torch.zeros(8, 1, dtype=torch.int32), [8, 5, 5, 5], torch.ones(1, 4))


def test_cabi_argument_validation():
    from vector_quantization import native

    lib = native.load()
    lv = (ctypes.c_int32 * 17)(*([8] * 17))
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its checks first

    def err():
        return lib.vq_last_error().decode()

    q = lib.vq_fsq_quantize_f32
    assert q(None, 0, 4, 1, 10, 4, lv, 1, p, 0, p, 0, 4, None, None) == -1 and "null" in err()
    assert q(p, 0, 4, 1, 10, 4, lv, 1, p, 0, None, 0, 4, None, None) == -1 and "null" in err()
    assert q(p, 0, 4, 1, 10, 4, None, 1, p, 0, p, 0, 4, None, None) == -1 and "null" in err()
    assert q(p, 0, 4, 1, 10, 4, lv, 1, None, 0, p, 0, 4, None, None) == -1 and "null" in err()
    assert q(p, 0, 17, 1, 10, 17, lv, 1, p, 0, p, 0, 17, None, None) == -1 and "[1, 16]" in err()
    assert q(p, 0, 0, 1, 10, 0, lv, 1, p, 0, p, 0, 0, None, None) == -1 and "[1, 16]" in err()
    for G, N, S in ((0, 10, 1), (1, 0, 1), (1, -5, 1), (1, 10, 0), (70000, 10, 1)):
        assert q(p, 0, 4, G, N, 4, lv, S, p, 0, p, 0, 4, None, None) == -1 and "positive" in err()
    bad = (ctypes.c_int32 * 4)(8, 5, 1, 5)
    assert q(p, 0, 4, 1, 10, 4, bad, 1, p, 0, p, 0, 4, None, None) == -1 and ">= 2" in err()
    big = (ctypes.c_int32 * 4)(65536, 65536, 2, 2)
    assert q(p, 0, 4, 1, 10, 4, big, 1, p, 0, p, 0, 4, None, None) == -1 and "int32" in err()
    b = lib.vq_fsq_backward_f32
    assert b(p, 0, 4, 1, 10, 4, lv, 1, p, 1, None, 0, 4, p, 0, 4, None) == -1 and "null" in err()
    assert b(p, 0, 4, 1, 10, 4, lv, 1, p, 1, p, 0, 4, None, 0, 4, None) == -1 and "null" in err()
    assert b(p, 0, 4, 1, 10, 4, bad, 1, p, 1, p, 0, 4, p, 0, 4, None) == -1 and ">= 2" in err()
    assert b(p, 0, 4, 1, 10, 20, lv, 1, p, 1, p, 0, 4, p, 0, 4, None) == -1 and "[1, 16]" in err()
    dcd = lib.vq_fsq_decode_f32
    assert dcd(p, 0, 10, 2, 4, lv, p, 1, None, None, None) == -1 and "null" in err()
    assert dcd(None, 0, 10, 2, 4, lv, p, 1, p, None, None) == -1 and "null" in err()
    assert dcd(p, 0, 10, 2, 4, lv, None, 1, p, None, None) == -1 and "null" in err()
    assert dcd(p, 0, 10, 0, 4, lv, p, 1, p, None, None) == -1 and "positive" in err()
    assert dcd(p, 0, 0, 2, 4, lv, p, 1, p, None, None) == -1 and "positive" in err()
    assert dcd(p, 0, 10, 2, 4, bad, p, 1, p, None, None) == -1 and ">= 2" in err()
    assert dcd(p, 0, 10, 2, 17, lv, p, 1, p, None, None) == -1 and "[1, 16]" in err()


def test_ops_have_fake_implementations():
    import vector_quantization  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty((2, 100, 4))
        k = torch.empty((3 + 5, 4))
        out, idx = torch.ops.vq_mi355x.fsq_quantize(x, [8, 5, 5, 5], k, True, True)
        assert out.shape == x.shape and idx.shape == (2, 100, 5) and idx.dtype == torch.int32
        _, idx = torch.ops.vq_mi355x.fsq_quantize(x, [8, 5, 5, 5], k, True, False)
        assert idx.numel() == 0
        gx = torch.ops.vq_mi355x.fsq_backward(x, [8, 5, 5, 5], k, True, x)
        assert gx.shape == x.shape
        i = torch.empty((100, 5), dtype=torch.int64)
        s, a = torch.ops.vq_mi355x.fsq_decode(i, [8, 5, 5, 5], torch.empty((5, 4)), True, True, True)
        assert s.shape == (100, 4) and a.shape == (5, 100, 4)


def test_inference_forward_traces_without_graph_break():
    import torch._dynamo as dynamo

    from vector_quantization import ResidualFSQ

    torch.manual_seed(0)
    mod = ResidualFSQ(dim=16, levels=[8, 5, 5, 5], num_quantizers=4).eval()
    x = torch.randn(2, 30, 16)
    dynamo.reset()
    with torch.no_grad():
        gm, _guards = dynamo.export(mod)(x)  # export = fullgraph: any graph break raises
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert any("vq_mi355x.fsq_quantize" in t for t in targets), targets


def test_dropout_cut_sequence():
    from vector_quantization import ResidualFSQ

    m = ResidualFSQ(dim=4, levels=[8, 5, 5, 5], num_quantizers=8, quantize_dropout=True, quantize_dropout_cutoff_index=1,
                    quantize_dropout_multiple_of=2).train()
    for seed in range(20):
        rand = random.Random(seed)
        cut = rand.randrange(1, 8)
        cut = -(-(cut + 1) // 2) * 2 - 1
        assert m._dropout_cut(seed) == cut
    assert m.eval()._dropout_cut(3) is None


@pytest.mark.parametrize("d", range(1, 17))
def test_sweep_recipe_against_the_cpu_helpers(d):
    """The oracle of tests/test_gpu_fsq_dims.py checked on the CPU: with levels_for(d) and the sweep's inputs every index
    term of the CPU module's codes is a whole number (so the sum is exact in any order), the numpy index model and the
    int64 index both equal the module's codes_to_indices, and fewer than 1 % of the rows lie within 1e-5 of a rounding
    boundary at any stage of Q = 1 and of Q = 3."""
    from fsq_dense import chain64, exact_indices, levels_for, sweep_input, whole_terms

    from vector_quantization import FSQ

    levels = levels_for(d)
    assert max(levels) <= 25 and int(np.prod(np.array(levels, dtype=np.int64))) <= 2**24
    x = torch.from_numpy(sweep_input(20011, d, d))
    mod = FSQ(levels)
    codes = mod.quantize(x)
    want = mod.codes_to_indices(codes).numpy()
    keep = whole_terms(codes.numpy(), levels)
    assert keep.all()
    assert np.array_equal(indices_np(codes.numpy(), levels), want)
    k = np.rint(codes.numpy().astype(np.float64) * np.array([v // 2 for v in levels]))
    assert np.array_equal(exact_indices(k, levels), want.astype(np.int64))
    lv = torch.tensor(levels, dtype=torch.float32)
    for Q, prebound in ((1, False), (3, True)):
        scales = torch.stack([(lv - 1) ** -q for q in range(Q)]).double()
        _, margin = chain64(x.double(), levels, scales, prebound)
        left_out = float((margin < 1e-5).double().mean())
        print(f"d={d} Q={Q}: {left_out:.4%} of rows within 1e-5 of a rounding boundary")
        assert left_out < 0.01
