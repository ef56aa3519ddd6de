"""ResidualLFQ / GroupedResidualLFQ without a GPU: import surface, constructor attributes, state_dict against the reference
fixtures (tests/golden/data/rlfq_*.npz), the index helpers on CPU, the quantize-dropout cut sequence, the fp64 restatement
(tests/rlfq_dense.py) against the fixtures, the no-CPU-fallback rule, and a fullgraph trace under fake tensors."""
from __future__ import annotations

import glob
import json
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(DATA, "rlfq_*.npz")))


def load_fixture(name):
    f = np.load(os.path.join(DATA, f"rlfq_{name}.npz"))
    return f, json.loads(str(f["config"]))


def build_module(f, c):
    from vector_quantization import GroupedResidualLFQ, ResidualLFQ

    mod = (GroupedResidualLFQ if c["kind"] == "grlfq" else ResidualLFQ)(**c["kwargs"])
    sd = {k[3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd_") and k != "sd_keys"}
    mod.load_state_dict(sd, strict=True)
    return mod.train(c.get("train", True))


def test_fixtures_present():
    assert len(FIXTURES) >= 25


def test_import_surface():
    import vector_quantization
    from vector_quantization import GroupedResidualLFQ, LFQ, ResidualLFQ
    from vector_quantization.residual_lfq import GroupedResidualLFQ as G2, ResidualLFQ as R2

    assert ResidualLFQ is R2 and GroupedResidualLFQ is G2
    assert "ResidualLFQ" in vector_quantization.__all__ and "GroupedResidualLFQ" in vector_quantization.__all__
    m = ResidualLFQ(dim=12, num_quantizers=2, codebook_size=4096)
    assert all(isinstance(layer, LFQ) for layer in m.layers)


def test_constructor_attributes():
    from torch import nn

    from vector_quantization import GroupedResidualLFQ, ResidualLFQ

    m = ResidualLFQ(dim=12, num_quantizers=4, codebook_size=4096, soft_clamp_input_value=3.0, spherical=True)
    assert m.num_quantizers == 4 and not m.has_projections and not m.quantize_dropout
    assert isinstance(m.project_in, nn.Identity) and isinstance(m.project_out, nn.Identity)
    assert [layer.codebook_scale for layer in m.layers] == [1.0, 0.5, 0.25, 0.125]
    assert [layer.soft_clamp_input_value for layer in m.layers] == [3.0, 1.5, 0.75, 0.375]
    assert all(layer.spherical and layer.dim == 12 and layer.codebook_dim == 12 for layer in m.layers)
    p = ResidualLFQ(dim=32, num_quantizers=2, codebook_size=256, quantize_dropout=True, quantize_dropout_cutoff_index=1,
                    quantize_dropout_multiple_of=2)
    assert p.has_projections and p.project_in.in_features == 32 and p.project_in.out_features == 8
    assert p.project_out.in_features == 8 and p.project_out.out_features == 32
    assert p.quantize_dropout and p.quantize_dropout_cutoff_index == 1 and p.quantize_dropout_multiple_of == 2
    assert not ResidualLFQ(dim=4, num_quantizers=1, codebook_size=16, quantize_dropout=True).quantize_dropout
    g = GroupedResidualLFQ(dim=24, groups=3, num_quantizers=2, codebook_size=256)
    assert len(g.rvqs) == 3 and g.split_dim == -1 and all(not r.has_projections for r in g.rvqs)
    assert GroupedResidualLFQ(dim=8, groups=2, accept_image_fmap=True, num_quantizers=1, codebook_size=16).split_dim == 1
    with pytest.raises(AssertionError):
        GroupedResidualLFQ(dim=10, groups=3, num_quantizers=1, codebook_size=16)
    with pytest.raises(ValueError, match="20"):
        ResidualLFQ(dim=21, num_quantizers=2, codebook_size=2**21)


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_matches_reference(name):
    f, c = load_fixture(name)
    mod = build_module(f, c)
    want = json.loads(str(f["sd_keys"]))
    got = [[k, list(t.shape), str(t.dtype)] for k, t in mod.state_dict().items()]
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("name", FIXTURES)
def test_index_helpers_against_fixture(name):
    f, c = load_fixture(name)
    mod = build_module(f, c)
    idx = torch.from_numpy(f["idx"])
    with torch.no_grad():
        got = mod.get_output_from_indices(idx)
        np.testing.assert_array_equal(got.numpy(), f["from_idx"])
        if "from_idx_pad" in f.files:
            np.testing.assert_array_equal(mod.get_output_from_indices(idx[..., :2]).numpy(), f["from_idx_pad"])
        if "all_codes" in f.files:
            np.testing.assert_array_equal(mod.get_codes_from_indices(idx).numpy(), f["all_codes"])
        if not c.get("train", True) and "rvqs" not in dict(mod.named_children()) and not mod.has_projections:
            # eval output is the sum of the stages' codes
            np.testing.assert_array_equal(got.numpy(), f["out"])


def test_codebooks_property():
    from vector_quantization import GroupedResidualLFQ, ResidualLFQ

    m = ResidualLFQ(dim=4, num_quantizers=3, codebook_size=16, spherical=True)
    cbs = m.codebooks
    assert cbs.shape == (3, 16, 4)
    assert torch.equal(cbs[2, 5], torch.tensor([-0.25, 0.25, -0.25, 0.25]))  # unnormalised bits_to_codes, even when spherical
    codes = m.get_codes_from_indices(torch.tensor([[[5, 0, 15]]]))
    assert torch.equal(codes[:, 0, 0], torch.stack([cbs[0, 5], cbs[1, 0], cbs[2, 15]]))
    g = GroupedResidualLFQ(dim=8, groups=2, num_quantizers=2, codebook_size=16)
    assert g.codebooks.shape == (2, 2, 16, 4)


def test_padding_needs_dropout():
    from vector_quantization import ResidualLFQ

    m = ResidualLFQ(dim=4, num_quantizers=3, codebook_size=16)
    with pytest.raises(AssertionError, match="quantize dropout"):
        m.get_codes_from_indices(torch.zeros(1, 2, 2, dtype=torch.long))


def _ref_cut(Q, cutoff, mult, seed):
    """residual_lfq.py:141-156 of the reference, restated."""
    rand = random.Random(seed) if seed is not None else random
    i = rand.randrange(cutoff, Q)
    if mult != 1:
        i = int(np.ceil((i + 1) / mult) * mult) - 1
    return i


def test_dropout_cut_sequence():
    from vector_quantization import ResidualLFQ

    for Q, cutoff, mult in ((4, 0, 1), (6, 0, 2), (5, 2, 1), (8, 1, 4)):
        m = ResidualLFQ(dim=4, num_quantizers=Q, codebook_size=16, quantize_dropout=True,
                        quantize_dropout_cutoff_index=cutoff, quantize_dropout_multiple_of=mult)
        for seed in range(20):
            assert m._dropout_cut(seed) == _ref_cut(Q, cutoff, mult, seed)
        # no fixed seed: the global `random` is consumed exactly as the reference does
        random.seed(123)
        got = [m._dropout_cut(None) for _ in range(10)]
        random.seed(123)
        assert got == [_ref_cut(Q, cutoff, mult, None) for _ in range(10)]
        assert m.eval()._dropout_cut(0) is None  # eval: no dropout, no `random` use


def test_grouped_forward_draws_its_seed_in_eval():
    from vector_quantization import GroupedResidualLFQ, native

    g = GroupedResidualLFQ(dim=8, groups=2, num_quantizers=2, codebook_size=16).eval()
    random.seed(7)
    with pytest.raises(native.NativeUnavailable):
        g(torch.randn(1, 3, 8))
    after = random.random()
    random.seed(7)
    random.randint(0, int(1e7))
    assert after == random.random()


_TRAIN = [n for n in FIXTURES if "eval" not in n]


@pytest.mark.parametrize("name", [n for n in _TRAIN if n.startswith(("d4", "d12_q3", "d12_clamp", "d12_sph", "g2_proj",
                                                                       "d12_frac_mask"))])
def test_dense_restatement_against_fixture(name):
    """tests/rlfq_dense.py reproduces the fixture's stored restatement, which sits within the reference's own fp32 error."""
    from rlfq_dense import restate, stage_rows

    f, c = load_fixture(name)
    mod = build_module(f, c)
    kw = dict(c["kwargs"])
    G = kw.pop("groups", 1)
    kw.pop("dim")
    x = torch.from_numpy(f["x"])
    r = torch.from_numpy(f["r"])
    mask = torch.from_numpy(f["mask"]) if "mask" in f.files else None
    idx = torch.from_numpy(f["idx"])
    idx_g = idx if c["kind"] == "grlfq" else idx[None]
    rvqs = list(mod.rvqs) if c["kind"] == "grlfq" else [mod]
    torch.manual_seed(c.get("draw_seed", 5))
    grads = []
    for gi, rvq in enumerate(rvqs):
        xs, rs = x.chunk(G, dim=-1)[gi], r.chunk(G, dim=-1)[gi]
        stages = int((idx_g[gi].reshape(-1, idx.shape[-1]) != -1).any(0).sum())
        rows = stage_rows(xs.numel() // xs.shape[-1], mask, kw.get("frac_per_sample_entropy", 1.0), stages)
        sd = {k: t for k, t in rvq.state_dict().items()}
        grads.append(restate(kw, sd, xs, mask, rs, stages, rows)["grad"])
    grad = torch.cat(grads, dim=-1)
    np.testing.assert_allclose(grad.numpy(), f["grad64"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(f["grad"], f["grad64"], rtol=0, atol=float(f["grad_ref_dev"]) * 1.0000001)
    assert float(f["grad_ref_dev"]) < 2e-5


def test_cpu_forward_raises_native_unavailable():
    from vector_quantization import GroupedResidualLFQ, ResidualLFQ, native

    m = ResidualLFQ(dim=12, num_quantizers=3, codebook_size=4096)
    for training in (True, False):
        with pytest.raises(native.NativeUnavailable):
            m.train(training)(torch.randn(2, 5, 12))
    g = GroupedResidualLFQ(dim=16, groups=2, num_quantizers=2, codebook_size=256)
    with pytest.raises(native.NativeUnavailable):
        g(torch.randn(2, 5, 16))
    v = torch.randn(1, 8, 4)
    with pytest.raises(native.NativeUnavailable):
        native.rlfq_quantize(v, [1.0], [None], [1.0])
    with pytest.raises(native.NativeUnavailable):
        native.rlfq_backward(v, [1.0], [None], [1.0])
    with pytest.raises(native.NativeUnavailable):
        native.lfq_entropy_staged_forward(v, None, [1.0], 1.0)
    with pytest.raises(native.NativeUnavailable):
        native.lfq_entropy_staged_backward(v, None, [1.0], 1.0, torch.ones(1), torch.ones(1, 16))


def test_library_limits():
    from vector_quantization import native

    lib = native.load()
    assert lib.vq_rlfq_workspace_bytes(1, 1000, 32) > 0
    assert lib.vq_rlfq_workspace_bytes(1, 1000, 33) == 0
    assert lib.vq_rlfq_workspace_bytes(0, 1000, 4) == 0
    one = lib.vq_lfq_staged_workspace_bytes(4096, 1, 16)
    assert one == lib.vq_lfq_workspace_bytes(4096, 4096, 1, 16)
    assert lib.vq_lfq_staged_workspace_bytes(4096, 8, 16) <= 8 * one
    assert lib.vq_lfq_staged_workspace_bytes(4096, 1, 21) == 0
    assert native.RLFQ_MAX_STAGES == 32
    with pytest.raises(AssertionError):
        native.rlfq_stages([1.0] * 33, [0.0] * 33, [1.0] * 33, "cpu")
    st = native.rlfq_stages([1.0, 0.5], [None, 2.0], [1.0, 0.5], "cpu")
    assert st.tolist() == [[1.0, 0.5], [0.0, 2.0], [1.0, 0.5]]


def test_ops_have_fake_implementations():
    import vector_quantization  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty((2, 100, 12))
        out, idx, v_all, commit = torch.ops.vq_mi355x.rlfq_quantize(x, [1.0, 0.5, 0.25], [0.0] * 3, [1.0, 0.5, 0.25], False,
                                                                    True, None, True, True)
        assert out.shape == x.shape and idx.shape == (2, 100, 3) and idx.dtype == torch.int64
        assert v_all.shape == (2, 3, 100, 12) and commit.shape == (2, 3) and commit.dtype == torch.float64
        gx = torch.ops.vq_mi355x.rlfq_backward(x, [1.0], [0.0], [1.0], False, None, x, None, None)
        assert gx.shape == x.shape
        v = torch.empty((6, 100, 12))
        ps, avg = torch.ops.vq_mi355x.lfq_entropy_staged_fwd(v, None, [1.0, 0.5, 0.25], 100.0)
        assert ps.shape == (6,) and ps.dtype == torch.float64 and avg.shape == (6, 4096)
        gv = torch.ops.vq_mi355x.lfq_entropy_staged_bwd(v, None, [1.0], 100.0, ps.float(), avg)
        assert gv.shape == v.shape


@pytest.mark.parametrize("dim", [10, 20])
def test_inference_forward_traces_without_graph_break(dim):
    """(GroupedResidualLFQ draws a Python random seed per forward, which an export cannot hold as a constant.)"""
    import torch._dynamo as dynamo

    from vector_quantization import ResidualLFQ

    torch.manual_seed(0)
    mod = ResidualLFQ(dim=dim, num_quantizers=4, codebook_size=1024).eval()
    x = torch.randn(2, 30, dim)
    dynamo.reset()
    with torch.no_grad():
        gm, _guards = dynamo.export(mod)(x)  # export = fullgraph: any graph break raises
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert any("vq_mi355x.rlfq_quantize" in t for t in targets), targets
