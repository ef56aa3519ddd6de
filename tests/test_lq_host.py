"""LatentQuantize without a GPU: import surface, constructor parity against every reference fixture
(tests/golden/data/lq_*.npz: attributes, buffers, state_dict), the constructor's errors, the index helpers on CPU, the
numpy fp32 model of the kernel (tests/lq_dense.py) against every fixture's out and indices, the share of rows a
comparison may leave out, the fp64 restatement against the fixtures, the no-CPU-fallback rule, the op registration and
the C ABI's declarations and argument checks."""
from __future__ import annotations

import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

from lq_cases import LQ_CASES
from lq_dense import indices_np, levels_of, order_free, quantize_np, restate64, smallest_gap, terms_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DATA, "lq_*.npz")))
MARGIN = 1e-4
MAX_SKIPPED_SHARE = 0.25


def load_fixture(name):
    f = np.load(os.path.join(DATA, f"{name}.npz"))
    return f, json.loads(str(f["config"]))


def fixture_tables(f, c):
    return [f[f"tab_{i}"] for i in range(len(levels_of(c["kwargs"])))]


def build_module(f, c):
    from vector_quantization import LatentQuantize

    torch.manual_seed(0)
    mod = LatentQuantize(**c["kwargs"])
    sd = {k[3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd_") and k != "sd_keys"}
    mod.load_state_dict(sd, strict=True)
    return mod.train(c.get("train", True))


def projected(f):
    return any(k.startswith("sd_project") for k in f.files)


def quantizer_input(f, c):
    """The fp32 values the quantizer sees, [b, n, C, d] (through project_in on the CPU when there is one)."""
    x = torch.from_numpy(f["x"])
    z = x.movedim(1, -1).reshape(x.shape[0], -1, x.shape[1])
    if projected(f):
        z = torch.nn.functional.linear(z, torch.from_numpy(f["sd_project_in.weight"]), torch.from_numpy(f["sd_project_in.bias"]))
    d = len(levels_of(c["kwargs"]))
    return z.reshape(z.shape[0], z.shape[1], -1, d).numpy()


def comparable_rows(f, c):
    """Rows (flat, one per sub-row) whose index a test compares: all of them for d <= 7; the order-free ones for d >= 8
    (torch's sum order over 8 and more terms is not pinned)."""
    levels = levels_of(c["kwargs"])
    z = quantizer_input(f, c)
    codes, _ = quantize_np(z, fixture_tables(f, c))
    keep = np.ones(codes.shape[:-1], dtype=bool) if len(levels) <= 7 else order_free(codes, levels)
    return keep.reshape(-1)


def test_fixtures_cover_the_cases():
    assert FIXTURES == sorted(f"lq_{n}" for n in LQ_CASES)
    assert len(FIXTURES) >= 24


def test_import_surface():
    import vector_quantization
    from vector_quantization import LatentQuantize
    from vector_quantization.latent_quantization import LatentQuantize as L2

    assert LatentQuantize is L2 and "LatentQuantize" in vector_quantization.__all__
    assert "LatentQuantize" in vector_quantization.__doc__ and "not part of this build" not in vector_quantization.__doc__


@pytest.mark.parametrize("name", FIXTURES)
def test_constructor_matches_reference(name):
    f, c = load_fixture(name)
    mod = build_module(f, c)
    want = json.loads(str(f["attrs"]))
    got = dict(dim=mod.dim, codebook_dim=mod.codebook_dim, num_codebooks=mod.num_codebooks,
               effective_codebook_dim=mod.effective_codebook_dim, keep_num_codebooks_dim=mod.keep_num_codebooks_dim,
               has_projections=mod.has_projections, codebook_size=mod.codebook_size, levels=mod._levels.tolist(),
               basis=mod._basis.tolist(), implicit_codebook_shape=list(mod.implicit_codebook.shape),
               values_type=type(mod.values_per_latent).__name__)
    assert got == want
    assert sorted(k for k, _ in mod.named_buffers()) == json.loads(str(f["buffers"]))
    assert not any(k in mod.state_dict() for k, _ in mod.named_buffers())  # every buffer is non-persistent
    assert [[k, list(t.shape), str(t.dtype)] for k, t in mod.state_dict().items()] == json.loads(str(f["sd_keys"]))
    assert mod.in_place_codebook_optimizer is None
    assert mod.commitment_loss_weight.dtype == torch.float32 and mod.commitment_loss_weight.dim() == 0
    for t, want_t in zip(mod.values_per_latent, fixture_tables(f, c)):
        assert t.device.type == "cpu" and np.array_equal(t.detach().numpy(), want_t, equal_nan=True)


def test_constructor_errors_and_divergences():
    from torch import nn

    from vector_quantization import LatentQuantize

    with pytest.raises(RuntimeError):
        LatentQuantize(levels=5, dim=4)  # an int without codebook_dim (the reference's own test expects it)
    for bad in ([5, 1, 8], [0], [5, -3]):
        with pytest.raises(ValueError):
            LatentQuantize(levels=bad, dim=len(bad))
    m = LatentQuantize(levels=[5, 5, 8], dim=6, num_codebooks=2)  # the reference's constructor raises here
    assert m.keep_num_codebooks_dim and not m.has_projections and m.effective_codebook_dim == 6
    assert m.implicit_codebook.shape == (200, 3) and isinstance(m.project_in, nn.Identity)
    m1 = LatentQuantize(levels=[5, 5, 8], dim=3)
    assert torch.equal(m.implicit_codebook, m1.implicit_codebook)
    k = LatentQuantize(levels=[5, 5, 8], dim=3, keep_num_codebooks_dim=True)
    assert k.keep_num_codebooks_dim and k.implicit_codebook.shape == (200, 3)
    idx = torch.tensor([[[3, 7], [11, 199]]])  # [b, n, c]
    codes = m.indices_to_codes(idx)
    assert codes.shape == (1, 6, 2)
    assert torch.equal(codes[0, :3, 1], m1.implicit_codebook[11]) and torch.equal(codes[0, 3:, 1], m1.implicit_codebook[199])
    lst = LatentQuantize(levels=[5, 5, 8], dim=3, optimize_values=False)
    assert isinstance(lst.values_per_latent, list) and lst.state_dict() == {}
    opt = LatentQuantize(levels=[5, 5, 8], dim=3, in_place_codebook_optimizer=lambda p: torch.optim.SGD(p, lr=0.1))
    assert isinstance(opt.in_place_codebook_optimizer, torch.optim.SGD)


@pytest.mark.parametrize("name", FIXTURES)
def test_index_helpers_against_fixture(name):
    f, c = load_fixture(name)
    mod = build_module(f, c)
    with torch.no_grad():
        got = mod.indices_to_codes(torch.from_numpy(f["idx_valid"]))
    if projected(f):
        np.testing.assert_allclose(got.numpy(), f["codes_from_idx"], rtol=1e-6, atol=1e-7)
    else:
        np.testing.assert_array_equal(got.numpy(), f["codes_from_idx"])
    if not projected(f):
        # the CPU helper is the reference's arithmetic and order: out (channel-first) -> indices
        out = torch.from_numpy(f["out"])
        codes = out.movedim(1, -1).reshape(out.shape[0], -1, mod.num_codebooks, mod.codebook_dim)
        idx = mod.codes_to_indices(codes)
        assert idx.dtype == torch.int32
        assert np.array_equal(idx.numpy().reshape(f["idx"].shape), f["idx"])


def test_codes_to_indices_maps_nan_to_int32_min():
    from vector_quantization import LatentQuantize

    m = LatentQuantize(levels=[5, 5, 8], dim=3)
    idx = m.codes_to_indices(torch.tensor([[0.0, float("nan"), 0.0], [0.0, 0.0, 0.0]]))
    assert idx.tolist() == [-(2**31), 2 + 2 * 5 + 4 * 25]


@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_model_reproduces_fixture(name):
    """tests/lq_dense.py's operation-by-operation model gives the reference's out and indices: bitwise on every row for
    no-projection cases with d <= 7, on the order-free rows for d >= 8, and through the CPU project_in otherwise."""
    f, c = load_fixture(name)
    levels = levels_of(c["kwargs"])
    z = quantizer_input(f, c)
    codes, _ = quantize_np(z, fixture_tables(f, c))
    keep = comparable_rows(f, c)
    got = indices_np(codes, levels).reshape(-1)
    want = f["idx"].reshape(-1)
    assert f["idx"].dtype == np.int32
    assert np.array_equal(got[keep], want[keep])
    if not projected(f):
        b = z.shape[0]
        out = np.moveaxis(codes.reshape(b, -1, codes.shape[2] * codes.shape[3]), -1, 1).reshape(f["out"].shape)
        assert np.array_equal(out.view(np.uint32), f["out"].view(np.uint32))


@pytest.mark.parametrize("name", FIXTURES)
def test_share_of_rows_left_out(name):
    f, c = load_fixture(name)
    keep = comparable_rows(f, c)
    skipped = 1.0 - keep.mean()
    if len(levels_of(c["kwargs"])) <= 7:
        assert skipped == 0.0
    assert skipped <= MAX_SKIPPED_SHARE, skipped
    if projected(f):
        gap = smallest_gap(quantizer_input(f, c), fixture_tables(f, c))
        assert float(np.nanmin(gap)) >= MARGIN and float(f["margin"]) >= MARGIN  # no row inside the margin: none left out


def test_truncation_cases_are_in_the_fixtures():
    """The index comes from c_i, not from the digits: the fixtures hold rows whose index differs from sum j_i * basis_i."""
    hit = {}
    for name in ("lq_l6_7_10_11", "lq_l15_22_24", "lq_l15", "lq_l26", "lq_d8"):
        f, c = load_fixture(name)
        levels = levels_of(c["kwargs"])
        codes, sel = quantize_np(quantizer_input(f, c), fixture_tables(f, c))
        digits = (sel * np.cumprod([1] + levels[:-1])).sum(-1).reshape(-1)
        hit[name] = int((digits != f["idx"].reshape(-1)).sum())
        t = terms_np(codes, levels)
        assert (t != np.trunc(t)).any(), name
    assert hit["lq_l15"] > 0 and hit["lq_l26"] > 0 and hit["lq_l15_22_24"] > 0, hit
    # L = 15 maps level 7 (an input exactly on the table's middle value) to index 6
    f, c = load_fixture("lq_l15")
    tab = f["tab_0"]
    pos = int(np.where(f["x"][0, 0] == tab[7])[0][0])
    assert f["idx"][0, pos] == 6


def test_ties_go_to_the_first_and_nan_rules():
    f, c = load_fixture("lq_dup")
    tab = f["tab_0"]
    assert tab[0] == tab[1]
    _, sel = quantize_np(quantizer_input(f, c), fixture_tables(f, c))
    assert (sel[..., 0] != 1).all() and (sel[..., 0] == 0).any()
    f, c = load_fixture("lq_nonfinite")
    assert np.isnan(f["out"][0, 1, 0]) and f["idx"][0, 0] == np.iinfo(np.int32).min
    assert np.isnan(f["loss"])
    f, c = load_fixture("lq_table_nan")
    assert np.isnan(f["out"][0, 1]).all() and np.isfinite(f["out"][0, [0, 2]]).all()  # a NaN distance is the minimum
    assert (f["idx"] == np.iinfo(np.int32).min).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_fp64_restatement_against_fixture(name):
    f, c = load_fixture(name)
    sd = {k[3:]: f[k] for k in f.files if k.startswith("sd_") and k != "sd_keys"}
    st = restate64(c["kwargs"], sd, f["x"], f["r"], c.get("train", True), fixture_tables(f, c))
    np.testing.assert_array_equal(st["grad"].numpy(), f["grad64"])
    np.testing.assert_array_equal(float(st["loss"]), float(f["loss64"]))
    fin = np.isfinite(f["grad64"]) & np.isfinite(f["grad"])
    np.testing.assert_allclose(f["grad"][fin], f["grad64"][fin], rtol=0, atol=float(f["grad_ref_dev"]) * 1.0000001 + 1e-30)
    if np.isfinite(f["loss64"]):
        assert abs(float(f["loss"]) - float(f["loss64"])) <= float(f["loss_ref_dev"]) * 1.0000001
        assert float(f["loss_ref_dev"]) <= 1e-6 * max(1.0, abs(float(f["loss64"])))
    if not c.get("train", True):
        assert float(f["loss"]) == 0.0
    assert not bool(f["table_grad_set"])  # values_per_latent never receives a gradient in the reference
    np.testing.assert_allclose(f["out"], st["out"].numpy(), rtol=1e-5, atol=1e-5, equal_nan=True)


def test_cpu_forward_raises_native_unavailable():
    from vector_quantization import LatentQuantize, native

    for mod in (LatentQuantize([5, 5, 8], dim=3), LatentQuantize([5, 5, 8], dim=4),
                LatentQuantize([5, 5, 8], dim=3, optimize_values=False)):
        for training in (True, False):
            with pytest.raises(native.NativeUnavailable):
                mod.train(training)(torch.randn(2, mod.dim, 5))
    with pytest.raises(native.NativeUnavailable):
        LatentQuantize([5, 5, 8], dim=3)(torch.randn(2, 3, 5, dtype=torch.float64))
    z = torch.randn(1, 8, 3)
    with pytest.raises(native.NativeUnavailable):
        native.lq_quantize(z, [5, 5, 8], torch.zeros(18))
    with pytest.raises(native.NativeUnavailable):
        native.lq_backward(z, z, z, torch.ones(()), 0.1)
    assert native.LQ_MAX_DIM == 16


def test_in_place_optimizer_training_forward_is_not_implemented():
    from vector_quantization import LatentQuantize

    m = LatentQuantize([5, 5, 8], dim=3, in_place_codebook_optimizer=lambda p: torch.optim.SGD(p, lr=0.1)).train()
    with pytest.raises(NotImplementedError, match="in-place"):
        m(torch.randn(2, 3, 5))
    from vector_quantization import native

    with pytest.raises(native.NativeUnavailable):  # the eval forward is supported (on the GPU)
        m.eval()(torch.randn(2, 3, 5))


def test_ops_are_registered_with_fake_implementations():
    import vector_quantization  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert hasattr(torch.ops.vq_mi355x, "lq_quantize") and hasattr(torch.ops.vq_mi355x, "lq_backward")
    with FakeTensorMode():
        z = torch.empty((2, 3, 100)).transpose(1, 2)
        tab = torch.empty((18,))
        out, idx, loss = torch.ops.vq_mi355x.lq_quantize(z, [5, 5, 8], tab, 1, True, True, 0.25, 0.1)
        assert out.shape == z.shape and out.stride() == z.stride()
        assert idx.shape == (2, 100, 1) and idx.dtype == torch.int32 and loss.shape == (2,)
        _, idx, loss = torch.ops.vq_mi355x.lq_quantize(z, [5, 5, 8], tab, 1, False, False, 0.0, 0.0)
        assert idx.numel() == 0 and loss.numel() == 0
        gx = torch.ops.vq_mi355x.lq_backward(z, out, z, torch.empty(()), 0.1)
        assert gx.shape == z.shape and gx.stride() == z.stride()


def test_eval_forward_traces_without_graph_break():
    import torch._dynamo as dynamo

    from vector_quantization import LatentQuantize

    mod = LatentQuantize([5, 5, 8], dim=3).eval()
    dynamo.reset()
    with torch.no_grad():
        gm, _guards = dynamo.export(mod)(torch.randn(2, 3, 30))  # export = fullgraph: any graph break raises
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert any("vq_mi355x.lq_quantize" in t for t in targets), targets


def test_cabi_declared_and_exported():
    from vector_quantization import native

    header = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    for sym in ("vq_lq_workspace_bytes", "vq_lq_quantize_f32", "vq_lq_backward_f32"):
        assert f" {sym}(" in header and sym in native.EXPORTED_SYMBOLS
        assert hasattr(native.load(), sym)


def test_cabi_argument_validation():
    from vector_quantization import native

    lib = native.load()
    lv = (ctypes.c_int32 * 17)(*([8] * 17))
    p = ctypes.c_void_p(16)  # never dereferenced: every call below fails its checks first

    def err():
        return lib.vq_last_error().decode()

    def q(z=p, B=2, P=10, C=1, d=4, levels=lv, tables=p, codes=p, idx=None, loss=None, ws=None, ws_bytes=0):
        return lib.vq_lq_quantize_f32(z, 40, 1, 10, B, P, C, d, levels, tables, codes, 40, 1, 10, idx, loss, 0.1, 0.1, ws,
                                      ws_bytes, None)

    assert q(z=None) == -1 and "null" in err()
    assert q(codes=None) == -1 and "null" in err()
    assert q(levels=None) == -1 and "null" in err()
    assert q(tables=None) == -1 and "null" in err()
    assert q(d=17) == -1 and "[1, 16]" in err()
    assert q(d=0) == -1 and "[1, 16]" in err()
    for B, P, C in ((0, 10, 1), (2, 0, 1), (2, 10, 0), (-1, 10, 1)):
        assert q(B=B, P=P, C=C) == -1 and "positive" in err()
    assert q(levels=(ctypes.c_int32 * 4)(8, 5, 1, 5)) == -1 and ">= 2" in err()
    assert q(levels=(ctypes.c_int32 * 4)(65536, 65536, 2, 2)) == -1 and "int32" in err()
    assert q(levels=(ctypes.c_int32 * 4)(46341, 46341, 2, 2)) == -1 and "int32" in err()
    assert q(levels=(ctypes.c_int32 * 2)(4000, 200), d=2) == -1 and "4096" in err()
    assert q(B=2**40, P=2**30) == -1 and "too many" in err()
    assert q(loss=p) == -1 and "workspace" in err()
    assert q(loss=p, ws=p, ws_bytes=3) == -1 and "workspace" in err()
    assert lib.vq_lq_workspace_bytes(2, 10, 1) == 4 and lib.vq_lq_workspace_bytes(1, 257, 2) == 12
    assert lib.vq_lq_workspace_bytes(0, 10, 1) == 0

    def bw(x=p, out=p, g=p, gl=p, gx=p, B=2, P=10, W=4):
        return lib.vq_lq_backward_f32(x, 40, 1, 10, out, 40, 1, 10, g, 40, 1, 10, gl, 0.1, B, P, W, gx, 40, 1, 10, None)

    for kw in (dict(x=None), dict(out=None), dict(g=None), dict(gl=None), dict(gx=None)):
        assert bw(**kw) == -1 and "null" in err()
    for kw in (dict(B=0), dict(P=0), dict(W=0)):
        assert bw(**kw) == -1 and "positive" in err()


SWEEP_ROWS = 20011


@pytest.mark.parametrize("tables", ["default", "learned"])
@pytest.mark.parametrize("d", range(1, 17))
def test_sweep_recipe_against_the_cpu_helpers(d, tables):
    """The oracle of tests/test_gpu_lq_dims.py checked on the CPU: with levels_for(d) and the sweep's inputs the numpy fp32
    model equals the module's CPU helpers (quantize and codes_to_indices, the reference's arithmetic) bitwise, on every row
    for d <= 7 and on the order-free rows for d >= 8, and the shares of rows the GPU tests leave out stay under their caps
    (1 % within 1e-6 of a tie; with default tables at d >= 8 at least 99 % order-free)."""
    from lq_dense import default_tables, learned_tables, levels_for, sweep_input

    from vector_quantization import LatentQuantize

    levels = levels_for(d)
    size = int(np.prod(np.array(levels, dtype=np.int64)))
    assert size <= 2**24 and (d <= 7 or set(levels) <= {2, 3, 4, 5, 8}) and (d < 4 or d > 7 or 6 in levels)
    tabs = default_tables(levels) if tables == "default" else learned_tables(levels, 100 + d)
    z = sweep_input(SWEEP_ROWS, d, d)
    mod = LatentQuantize(levels=levels, dim=d)
    with torch.no_grad():
        for p, t in zip(mod.values_per_latent, tabs):
            p.copy_(torch.from_numpy(t))
        want = mod.quantize(torch.from_numpy(z))
        want_idx = mod.codes_to_indices(want).numpy()
    codes, _ = quantize_np(z, tabs)
    assert np.array_equal(codes.view(np.uint32), want.numpy().view(np.uint32))
    keep = np.ones(SWEEP_ROWS, dtype=bool) if d <= 7 else order_free(codes, levels)
    got_idx = indices_np(codes, levels)
    assert got_idx.dtype == want_idx.dtype == np.int32
    assert np.array_equal(got_idx[keep], want_idx[keep])
    near_tie = float((smallest_gap(z, [np.unique(t) for t in tabs]) < 1e-6).mean())
    print(f"d={d} {tables}: {1 - keep.mean():.4%} of rows not order-free, {near_tie:.4%} within 1e-6 of a tie")
    assert near_tie <= 0.01
    if tables == "default" and d >= 8:
        assert keep.mean() >= 0.99
