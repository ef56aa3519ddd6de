"""FSQ / ResidualFSQ / GroupedResidualFSQ on the GPU: every reference fixture (tests/golden/data/fsq_*.npz, rfsq_*.npz)
through the fused path and the torch fallback, fused against fallback at 65 536 rows and on strided / transposed inputs,
the decode kernel against the implicit-codebook gather, determinism, the launch count of a forward, and opcheck."""
from __future__ import annotations

import contextlib
import random

import numpy as np
import pytest
import torch

from fsq_dense import chain64, restate
from test_fsq_host import FIXTURES, build_module, fixture_input, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@contextlib.contextmanager
def fallback():
    """Route every forward to the torch fallback (the reference's forward, on the GPU)."""
    from vector_quantization import finite_scalar_quantization as fsq

    orig = fsq._fused_ok
    fsq._fused_ok = lambda *a: False
    try:
        yield
    finally:
        fsq._fused_ok = orig


def _forward(mod, x, c):
    random.seed(c.get("py_seed", 0))
    if c["kind"] == "fsq":
        return mod(x)
    codes = c.get("codes", False)
    if c["kind"] == "rfsq":
        return mod(x, return_all_codes=codes, rand_quantize_dropout_fixed_seed=c.get("seed"))
    return mod(x, return_all_codes=codes)


def _run(name, fused):
    f, c = load_fixture(name)
    mod = build_module(f, c).to(DEV)
    x = fixture_input(f, c).to(DEV).requires_grad_(True)
    with contextlib.nullcontext() if fused else fallback():
        res = _forward(mod, x, c)
        (res[0].float() * torch.from_numpy(f["r"]).to(DEV)).sum().backward()
    return f, c, mod, res, x.grad


def _stages(f, c):
    if c["kind"] == "fsq":
        return 1
    idx = f["idx"]
    return int((idx.reshape(-1, idx.shape[-1]) != -1).any(0).sum())


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "fallback"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(name, fused):
    f, c, mod, res, grad = _run(name, fused)
    out, idx = res[:2]
    if "idx" in f.files:
        want = torch.from_numpy(f["idx"])
        assert idx.dtype == want.dtype and idx.shape == want.shape
        if fused or not c.get("collide"):  # torch's GPU sum may add the terms in another order
            assert torch.equal(idx.cpu(), want), "indices differ from the reference"
    else:
        assert idx is None
    projected = any(k.startswith("sd_") and "project" in k for k in f.files)
    got = out.detach().float().cpu().numpy()
    if projected:
        np.testing.assert_allclose(got, f["out"], rtol=1e-5, atol=1e-6)
    else:
        np.testing.assert_array_equal(got, f["out"])
    if "all_codes" in f.files:
        all_codes = res[2]
        all_codes = torch.stack(all_codes) if isinstance(all_codes, tuple) else all_codes
        assert torch.equal(all_codes.cpu(), torch.from_numpy(f["all_codes"]))
    # gradients: against the fixture's own fp32 dL/dx (2x its distance from the fp64 restatement), and the fused path
    # against the fp64 restatement itself
    g = grad.float().cpu().numpy()
    fin = np.isfinite(f["grad64"])
    bf16 = c.get("dtype") == "bfloat16"
    dev = float(f["grad_ref_dev"])
    np.testing.assert_allclose(g[fin], f["grad"][fin], rtol=0, atol=2 * dev + 1e-6)
    if fused and not bf16:
        # stage t divides the residual by scale_t, so one ulp of r_t moves z_t by ulp / scale_t: the fixture's own
        # distance is the floor at deep stages
        Q = _stages(f, c)
        np.testing.assert_allclose(g[fin], f["grad64"][fin], rtol=1e-4, atol=1e-6 * Q + 2 * dev)
    if c["kind"] != "fsq":
        with torch.no_grad():
            idx_dev = torch.from_numpy(f["idx"]).to(DEV)
            np.testing.assert_allclose(mod.get_output_from_indices(idx_dev).cpu().numpy(), f["from_idx"], rtol=1e-6,
                                       atol=1e-7)
            if "from_idx_pad" in f.files:
                np.testing.assert_allclose(mod.get_output_from_indices(idx_dev[..., :2]).cpu().numpy(), f["from_idx_pad"],
                                           rtol=1e-6, atol=1e-7)
    elif "idx_valid" in f.files:
        with torch.no_grad():
            codes = mod.indices_to_codes(torch.from_numpy(f["idx_valid"]).to(DEV)).float().cpu().numpy()
        if projected:
            np.testing.assert_allclose(codes, f["codes_from_idx"], rtol=1e-5, atol=1e-6)
        else:
            np.testing.assert_array_equal(codes, f["codes_from_idx"])


def _clearing_rows(levels, scales, xs, prebound):
    """Rows (of xs [G, N, d] as the fallback sees them) whose stage values all clear a boundary by 1e-5."""
    _, margin = chain64(xs.double(), levels, scales.double(), prebound)
    return margin >= 1e-5


@pytest.mark.parametrize("case", ["rfsq", "grfsq", "grfsq_strided", "fsq_transposed", "rfsq_transposed"])
def test_fused_equals_fallback_65536_rows(case):
    from vector_quantization import FSQ, GroupedResidualFSQ, ResidualFSQ

    torch.manual_seed(1)
    levels = [8, 5, 5, 5]
    g = torch.Generator(device=DEV).manual_seed(9)
    if case == "rfsq":
        mod = ResidualFSQ(dim=4, levels=levels, num_quantizers=8).to(DEV)
        x = torch.randn(4, 16384, 4, device=DEV, generator=g) * 2
    elif case.startswith("grfsq"):
        mod = GroupedResidualFSQ(dim=16, groups=4, levels=levels, num_quantizers=8).to(DEV)
        x = torch.randn(4, 16384, 16 if case == "grfsq" else 40, device=DEV, generator=g) * 2
        if case == "grfsq_strided":
            x = x[..., 3:35:2]  # rows not contiguous: copied once, then the group axis
    elif case == "fsq_transposed":
        mod = FSQ([7, 5, 5, 5, 5, 6]).to(DEV)
        x = torch.randn(1, 6, 65536, device=DEV, generator=g).transpose(1, 2) * 2
    else:
        mod = ResidualFSQ(dim=4, levels=levels, num_quantizers=8).to(DEV)
        x = torch.randn(1, 4, 65536, device=DEV, generator=g).transpose(1, 2) * 2
    mod.train()
    outs = []
    for fused in (True, False):
        xi = x.detach().clone().requires_grad_(True) if fused else x.detach().requires_grad_(True)
        with contextlib.nullcontext() if fused else fallback():
            out, idx = _forward(mod, xi, dict(kind="grfsq" if case.startswith("grfsq") else "rfsq" if "rfsq" in case
                                              else "fsq"))
            out.sum().backward()
        outs.append((out.detach(), idx, xi.grad))
    (o1, i1, g1), (o2, i2, g2) = outs
    assert i1.dtype == i2.dtype and i1.shape == i2.shape and o1.shape == o2.shape
    # rows whose fallback stage values clear every boundary by 1e-5 (computed in fp64 on the same inputs)
    d = len(mod.layers[0]._level_values) if case.startswith("rfsq") else len(levels) if case.startswith("grfsq") else 6
    if case.startswith("grfsq"):
        scales = mod.rvqs[0].scales
        xs = x.reshape(-1, 4, d).transpose(0, 1)
        ok = _clearing_rows(levels, scales, xs, True).all(dim=0).reshape(x.shape[:-1])
        o1r, o2r = o1.reshape(*x.shape[:-1], 4, d), o2.reshape(*x.shape[:-1], 4, d)
        i1r, i2r = i1.permute(1, 2, 0, 3), i2.permute(1, 2, 0, 3)
    elif case.startswith("rfsq"):
        ok = _clearing_rows(levels, mod.scales, x, True)
        o1r, o2r, i1r, i2r = o1, o2, i1, i2
    else:
        ok = _clearing_rows(mod._level_values, torch.ones(1, d, device=DEV), x, False)
        o1r, o2r, i1r, i2r = o1, o2, i1[..., None], i2[..., None]
    n_bad = int((~ok).sum())
    n_diff = int(((o1r != o2r).flatten(ok.dim()).any(-1) | (i1r != i2r).flatten(ok.dim()).any(-1))[ok].sum())
    print(f"{case}: {n_bad} of {ok.numel()} rows within 1e-5 of a rounding boundary; {n_diff} clearing rows differ")
    assert n_bad < ok.numel() // 100
    assert torch.equal(o1r[ok], o2r[ok]) and torch.equal(i1r[ok], i2r[ok])
    # the fallback's fp32 1 - tanh^2 cancels where tanh saturates (the fused kernel's does not): a loose check here, the
    # fp64 restatement is the tight one
    np.testing.assert_allclose(g1[ok].cpu().numpy(), g2[ok].cpu().numpy(), rtol=1e-3, atol=1e-2)


def test_collision_levels_fused():
    """[26], [27, 5], [1000]: the fused kernel reproduces the reference's truncated fp32 index on every code."""
    from vector_quantization import FSQ

    for levels in ([26], [27, 5], [1000], [8, 5, 5, 5], [8, 6, 5], [7, 5, 5, 5, 5]):
        m = FSQ(levels)
        want = m.codes_to_indices(m.implicit_codebook)  # CPU: the reference's own arithmetic and order
        md = m.to(DEV)
        # inputs whose bound lands on every code exactly
        L = torch.tensor(levels, dtype=torch.float64)
        half_l = (L - 1) * 1.001 / 2
        offset = torch.tensor([0.5 if v % 2 == 0 else 0.0 for v in levels], dtype=torch.float64)
        b = m.implicit_codebook.double().cpu() * torch.tensor([v // 2 for v in levels], dtype=torch.float64)
        x = torch.atanh((b + offset) / half_l) - torch.atanh(offset / half_l)
        with torch.no_grad():
            out, idx = md(x.float()[None].to(DEV))
        assert torch.equal(out[0].cpu(), m.implicit_codebook.cpu()), levels
        assert torch.equal(idx[0].cpu(), want), levels


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_decode_bitwise_equals_gather(dtype):
    from vector_quantization import GroupedResidualFSQ, ResidualFSQ, native

    mod = ResidualFSQ(dim=5, levels=[7, 5, 5, 5, 5], num_quantizers=5, quantize_dropout=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(4)
    idx = torch.randint(0, mod.codebook_size, (3, 700, 5), device=DEV, generator=g).to(dtype)
    idx[0, :50, 3:] = -1
    all_codes = mod.get_codes_from_indices(idx)
    cb = mod.codebooks
    want = torch.stack([cb[q][idx[..., q].clamp(min=0).long()] for q in range(5)]) * mod.scales[:, None, None, :]
    want = want.masked_fill((idx == -1).permute(2, 0, 1)[..., None], 0.0)
    assert torch.equal(all_codes, want)
    out = mod.get_output_from_indices(idx)
    acc = torch.zeros_like(want[0])
    for q in range(5):
        acc = acc + want[q]
    assert torch.equal(out, acc)
    # coarse indices pad with -1
    assert torch.equal(mod.get_codes_from_indices(idx[..., :2])[2:], torch.zeros_like(want[2:]))
    # FSQ.indices_to_codes on the GPU (Python floor / modulo semantics, negative indices included)
    from vector_quantization import FSQ

    m = FSQ([8, 5, 5, 5]).to(DEV)
    i = torch.arange(-1000, 2000, device=DEV, dtype=dtype)
    assert torch.equal(m.indices_to_codes(i), m._scale_and_shift_inverse(m.indices_to_level_indices(i)))
    gm = GroupedResidualFSQ(dim=8, groups=2, levels=[8, 5, 5, 5], num_quantizers=3).to(DEV)
    gi = torch.randint(0, 1000, (2, 2, 10, 3), device=DEV, generator=g).to(dtype)
    assert gm.get_output_from_indices(gi).shape == (2, 10, 8)
    with pytest.raises(RuntimeError):
        native.fsq_decode(idx.reshape(-1, 5), [7, 5, 5, 5, 1], mod.scales.contiguous())


def test_two_training_steps_bitwise_equal():
    from vector_quantization import GroupedResidualFSQ

    torch.manual_seed(3)
    mod = GroupedResidualFSQ(dim=64, groups=4, levels=[8, 5, 5, 5], num_quantizers=6).to(DEV).train()
    x0 = torch.randn(4, 3000, 64, device=DEV)
    res = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        random.seed(5)
        out, idx = mod(x)
        (out * out).sum().backward()
        res.append((out.detach(), idx, x.grad, mod.rvqs[0].project_in.weight.grad.clone()))
        mod.zero_grad()
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("Q,G", [(1, 1), (8, 1), (8, 4)])
def test_one_native_quantize_launch_per_forward(monkeypatch, Q, G):
    from vector_quantization import FSQ, GroupedResidualFSQ, ResidualFSQ, native

    calls = {}
    for name in ("fsq_quantize", "fsq_backward", "fsq_decode"):
        fn = getattr(native, name)

        def wrap(*a, _fn=fn, _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **k)

        monkeypatch.setattr(native, name, wrap)
    if G > 1:
        mod = GroupedResidualFSQ(dim=4 * G, groups=G, levels=[8, 5, 5, 5], num_quantizers=Q)
    elif Q > 1:
        mod = ResidualFSQ(dim=4, levels=[8, 5, 5, 5], num_quantizers=Q)
    else:
        mod = FSQ([8, 5, 5, 5])
    mod = mod.to(DEV).train()
    x = torch.randn(2, 512, 4 * G, device=DEV, requires_grad=True)
    out, idx = mod(x)
    assert calls == {"fsq_quantize": 1}, calls
    out.sum().backward()
    assert calls == {"fsq_quantize": 1, "fsq_backward": 1}, calls


def test_torch_library_opcheck():
    from vector_quantization.finite_scalar_quantization import kernel_consts

    levels = [8, 5, 5, 5]
    lv = torch.tensor(levels, dtype=torch.int32, device=DEV)
    scales = torch.stack([(torch.tensor(levels, dtype=torch.float32) - 1) ** -q for q in range(3)]).to(DEV)
    k = kernel_consts(lv, scales)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(2, 300, 4, device=DEV, generator=g)
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.vq_mi355x.fsq_quantize.default, (x, levels, k, True, True), test_utils=utils)
    torch.library.opcheck(torch.ops.vq_mi355x.fsq_backward.default, (x, levels, k, True, torch.ones_like(x)), test_utils=utils)
    idx = torch.randint(0, 1000, (300, 3), device=DEV, generator=g)
    torch.library.opcheck(torch.ops.vq_mi355x.fsq_decode.default, (idx, levels, scales.contiguous(), True, True, True),
                          test_utils=utils)
    out, i = torch.ops.vq_mi355x.fsq_quantize(x, levels, k, True, True)
    s, a = torch.ops.vq_mi355x.fsq_decode(i.reshape(-1, 3), levels, scales.contiguous(), True, True, True)
    assert torch.equal(s.reshape(out.shape), out)


def test_fp64_restatement_gradient_at_scale():
    """The fused dL/dx against the fp64 restatement on 65 536 rows, Q = 3, saturated inputs included (there the fp32
    1 - tanh^2 of autograd has no correct digit left)."""
    from vector_quantization import ResidualFSQ

    torch.manual_seed(2)
    mod = ResidualFSQ(dim=4, levels=[8, 5, 5, 5], num_quantizers=3).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(12)
    x = (torch.randn(1, 65536, 4, device=DEV, generator=g) * 3).requires_grad_(True)
    r = torch.randn(1, 65536, 4, device=DEV, generator=g)
    out, _ = mod(x)
    (out * r).sum().backward()
    st = restate("rfsq", dict(levels=[8, 5, 5, 5], num_quantizers=3), {}, x.detach(), r)
    _, margin = chain64(x.detach().double(), [8, 5, 5, 5], mod.scales.double(), True)
    ok = (margin >= 1e-5)[..., None].expand_as(x)
    np.testing.assert_allclose(x.grad[ok].cpu().numpy(), st["grad"][ok].cpu().numpy(), rtol=1e-4, atol=2e-5)
