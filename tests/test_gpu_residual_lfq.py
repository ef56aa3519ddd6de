"""ResidualLFQ / GroupedResidualLFQ on the GPU: the reference fixtures (tests/golden/data/rlfq_*.npz) through the fused and
the stage-by-stage path, fused against stage-by-stage at 65 536 rows, the staged entropy kernels against single-stage
calls (bitwise), the launch plan of a training step, determinism, groups batched in one launch, and torch.compile."""
from __future__ import annotations

import contextlib
import random

import numpy as np
import pytest
import torch

from test_rlfq_host import FIXTURES, build_module, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@contextlib.contextmanager
def stagewise():
    """Route every forward to the stage-by-stage fallback."""
    from vector_quantization import residual_lfq

    orig = residual_lfq._fused_ok
    residual_lfq._fused_ok = lambda *a: False
    try:
        yield
    finally:
        residual_lfq._fused_ok = orig


def _run(name, fused):
    f, c = load_fixture(name)
    mod = build_module(f, c).to(DEV)
    x = torch.from_numpy(f["x"]).to(DEV).requires_grad_(True)
    mask = torch.from_numpy(f["mask"]).to(DEV) if "mask" in f.files else None
    codes = c.get("codes", False)
    random.seed(c.get("py_seed", 0))
    torch.manual_seed(c.get("draw_seed", 5))
    kw = dict(mask=mask, return_all_codes=codes)
    if c["kind"] == "rlfq":
        kw["rand_quantize_dropout_fixed_seed"] = c.get("seed")
    with contextlib.nullcontext() if fused else stagewise():
        res = mod(x, **kw)
        out, idx, losses = res[:3]
        if mod.training:
            (losses.sum() + (out * torch.from_numpy(f["r"]).to(DEV)).sum()).backward()
    return f, c, mod, res, x.grad


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stagewise"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(name, fused):
    f, c, mod, res, grad = _run(name, fused)
    out, idx, losses = res[:3]
    assert torch.equal(idx.cpu(), torch.from_numpy(f["idx"])), "indices differ from the reference"
    kw = c["kwargs"]
    plain = not (kw.get("soft_clamp_input_value") or kw.get("spherical"))
    rvq = mod.rvqs[0] if c["kind"] == "grlfq" else mod
    if plain and not rvq.has_projections:
        torch.testing.assert_close(out.detach().cpu(), torch.from_numpy(f["out"]), rtol=2e-6, atol=1e-7)
    else:
        torch.testing.assert_close(out.detach().cpu(), torch.from_numpy(f["out"]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(losses.detach().cpu().numpy(), f["losses"], rtol=1e-5, atol=1e-6)
    if "all_codes" in f.files:
        codes = res[3]
        codes = torch.stack(codes) if isinstance(codes, tuple) else codes
        assert torch.equal(codes.cpu(), torch.from_numpy(f["all_codes"]))
    if grad is not None:
        g = grad.double().cpu().numpy()
        np.testing.assert_allclose(g, f["grad64"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(g, f["grad"], rtol=0, atol=2 * float(f["grad_ref_dev"]) + 1e-6)


_LARGE = {
    "d16_plain": dict(d=16, kw={}),
    "d16_clamp": dict(d=16, kw=dict(soft_clamp_input_value=2.0)),
    "d16_mask_frac": dict(d=16, kw=dict(frac_per_sample_entropy=0.5), mask=True),
    "d20_plain": dict(d=20, kw={}),
    "d20_clamp_mask_frac": dict(d=20, kw=dict(soft_clamp_input_value=2.0, frac_per_sample_entropy=0.5), mask=True),
}


def _train_step(mod, x0, mask, fused, seed=9):
    x = x0.clone().requires_grad_(True)
    torch.manual_seed(seed)
    with contextlib.nullcontext() if fused else stagewise():
        out, idx, losses = mod(x, mask=mask)
        w = torch.linspace(0.5, 1.5, losses.numel(), device=DEV).reshape(losses.shape)
        ((losses * w).sum() + (out * 0.01).sum()).backward()
    return out.detach(), idx, losses.detach(), x.grad


@pytest.mark.parametrize("name", list(_LARGE))
def test_fused_equals_stagewise_65536_rows(name):
    from vector_quantization import ResidualLFQ

    cfg = _LARGE[name]
    d = cfg["d"]
    torch.manual_seed(1)
    mod = ResidualLFQ(dim=d, num_quantizers=8, codebook_size=2**d, **cfg["kw"]).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(2)
    x0 = torch.randn(16, 4096, d, device=DEV, generator=g)
    mask = (torch.rand(16, 4096, device=DEV, generator=g) > 0.3) if cfg.get("mask") else None
    a = _train_step(mod, x0, mask, True)
    b = _train_step(mod, x0, mask, False)
    assert torch.equal(a[1], b[1]), "indices differ between the fused and the stage-by-stage path"
    if "clamp" in cfg["kw"]:
        torch.testing.assert_close(a[0], b[0], rtol=1e-6, atol=1e-7)
    else:
        assert torch.equal(a[0], b[0]), "out differs between the fused and the stage-by-stage path"
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-6)
    scale = float(b[3].abs().max())
    torch.testing.assert_close(a[3], b[3], rtol=1e-4, atol=1e-6 * max(1.0, scale))


def test_commitment_sums_bitwise_equal_to_chained_lfq_calls():
    from vector_quantization import native

    g = torch.Generator(device=DEV).manual_seed(5)
    N, d, S = 65536 + 77, 16, 6
    x = torch.randn(N, d, device=DEV, generator=g)
    mask = torch.rand(N, device=DEV, generator=g) > 0.25
    qmag = [2.0**-s for s in range(S)]
    out, idx, v_all, commit = native.rlfq_quantize(x[None], qmag, [None] * S, qmag, mask=mask, want_v=True,
                                                   want_commit=True)
    r, acc = x, 0.0
    for s in range(S):
        v = r.reshape(N, 1, d)
        _, o, i, c = native.lfq_quantize(v, qmag[s], xa=v, mask=mask, want_commit=True)
        assert torch.equal(v_all[0, s], r)
        assert torch.equal(idx[0, :, s], i[:, 0])
        assert torch.equal(commit[0, s], c), s
        o = o.reshape(N, d)
        r = r - o
        acc = acc + o
    assert torch.equal(out[0], acc)


@pytest.mark.parametrize("d", [13, 16, 20])
def test_staged_entropy_bitwise_equals_single_stage_calls(d):
    from vector_quantization import native

    g = torch.Generator(device=DEV).manual_seed(d)
    T, N = 5, 3001 if d < 20 else 411
    R = N - 17 - d  # ragged
    v = torch.randn(T, N, d, device=DEV, generator=g) * 0.4
    rows = torch.stack([torch.randperm(N, device=DEV, generator=g)[:R].sort().values for _ in range(T)])
    scales = [1.0, 0.5, 0.25, 0.125, 0.0625]
    for rr in (rows, rows[0], None):
        ps, avg = native.lfq_entropy_staged_forward(v, rr, scales, 100.0 if d < 20 else 1.0)
        RR = N if rr is None else rr.shape[-1]
        w_ps = torch.rand(T, device=DEV, generator=g)
        w_cb = torch.randn(T, 1 << d, device=DEV, generator=g) / RR
        gv = native.lfq_entropy_staged_backward(v, rr, scales, 100.0 if d < 20 else 1.0, w_ps, w_cb)
        for t in range(T):
            rt = None if rr is None else (rr[t] if rr.dim() == 2 else rr)
            p1, a1 = native.lfq_entropy_forward(v[t].unsqueeze(1), rt, scales[t], 100.0 if d < 20 else 1.0)
            assert torch.equal(ps[t], p1) and torch.equal(avg[t], a1[0]), t
            g1 = native.lfq_entropy_backward(v[t].unsqueeze(1), rt, scales[t], 100.0 if d < 20 else 1.0, w_ps[t], w_cb[t:t + 1])
            assert torch.equal(gv[t], g1[:, 0]), t


def test_training_step_takes_the_fused_path(monkeypatch):
    from vector_quantization import ResidualLFQ, native

    calls = {}
    for name in ("rlfq_quantize", "rlfq_backward", "lfq_entropy_staged_forward", "lfq_entropy_staged_backward",
                 "lfq_quantize", "lfq_entropy_forward", "lfq_entropy_backward"):
        fn = getattr(native, name)

        def wrap(*a, _fn=fn, _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **k)

        monkeypatch.setattr(native, name, wrap)
    mod = ResidualLFQ(dim=16, num_quantizers=8, codebook_size=2**16, frac_per_sample_entropy=0.5).to(DEV).train()
    x = torch.randn(4, 1024, 16, device=DEV, requires_grad=True)
    mask = torch.ones(4, 1024, dtype=torch.bool, device=DEV)
    out, idx, losses = mod(x, mask=mask)
    assert calls == {"rlfq_quantize": 1, "lfq_entropy_staged_forward": 1}, calls
    (losses.sum() + out.sum()).backward()
    assert calls == {"rlfq_quantize": 1, "lfq_entropy_staged_forward": 1, "lfq_entropy_staged_backward": 1,
                     "rlfq_backward": 1}, calls


def test_deterministic_training_steps():
    from vector_quantization import GroupedResidualLFQ

    torch.manual_seed(3)
    mod = GroupedResidualLFQ(dim=32, groups=2, num_quantizers=6, codebook_size=2**14, frac_per_sample_entropy=0.75,
                             soft_clamp_input_value=4.0).to(DEV).train()
    x0 = torch.randn(4, 3000, 32, device=DEV)
    res = [_train_step(mod, x0, None, True, seed=4) for _ in range(2)]
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("train", [True, False])
def test_grouped_batched_equals_separate_groups(train):
    from vector_quantization import GroupedResidualLFQ

    torch.manual_seed(4)
    G, d = 4, 12
    grp = GroupedResidualLFQ(dim=G * d, groups=G, num_quantizers=5, codebook_size=2**d, frac_per_sample_entropy=0.5,
                             spherical=True).to(DEV).train(train)
    x0 = torch.randn(3, 2000, G * d, device=DEV)
    mask = torch.rand(3, 2000, device=DEV) > 0.2
    x = x0.clone().requires_grad_(True)
    torch.manual_seed(6)
    out, idx, losses = grp(x, mask=mask)
    xs = [c.clone().requires_grad_(True) for c in x0.chunk(G, dim=-1)]
    torch.manual_seed(6)  # the separate calls draw in the same order: group-major, then stage
    sep = [rvq(xc, mask=mask) for rvq, xc in zip(grp.rvqs, xs)]
    assert torch.equal(out, torch.cat([s[0] for s in sep], dim=-1))
    assert torch.equal(idx, torch.stack([s[1] for s in sep]))
    torch.testing.assert_close(losses, torch.stack([s[2] for s in sep]), rtol=1e-6, atol=1e-7)
    if train:
        (losses.sum() + out.sum()).backward()
        sum(s[2].sum() + s[0].sum() for s in sep).backward()
        torch.testing.assert_close(x.grad, torch.cat([xc.grad for xc in xs], dim=-1), rtol=1e-5, atol=1e-7)


def test_compiled_eval_equals_eager():
    import torch._dynamo as dynamo

    from vector_quantization import ResidualLFQ

    torch.manual_seed(0)
    mod = ResidualLFQ(dim=24, num_quantizers=4, codebook_size=2**12, soft_clamp_input_value=3.0).to(DEV).eval()
    x = torch.randn(2, 300, 24, device=DEV)
    dynamo.reset()
    compiled = torch.compile(mod, backend="aot_eager", fullgraph=True)
    with torch.no_grad():
        for xi in (x, x * 0.5 + 0.1):
            want = mod(xi)
            got = compiled(xi)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_torch_library_ops_on_device():
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn(2, 500, 10, device=DEV, generator=g)
    out, idx, v_all, commit = torch.ops.vq_mi355x.rlfq_quantize(x, [1.0, 0.5], [0.0, 0.0], [1.0, 0.5], False, True, None,
                                                                True, True)
    assert out.shape == x.shape and idx.shape == (2, 500, 2) and v_all.shape == (2, 2, 500, 10) and commit.shape == (2, 2)
    assert torch.equal(v_all[:, 0], x)
    ps, avg = torch.ops.vq_mi355x.lfq_entropy_staged_fwd(v_all.reshape(4, 500, 10), None, [1.0, 0.5], 1.0)
    np.testing.assert_allclose(avg.sum(-1).cpu().numpy(), np.ones(4), rtol=1e-5)
    gv = torch.ops.vq_mi355x.lfq_entropy_staged_bwd(v_all.reshape(4, 500, 10), None, [1.0, 0.5], 1.0, torch.ones(4, device=DEV),
                                                    torch.zeros_like(avg))
    gx = torch.ops.vq_mi355x.rlfq_backward(x, [1.0, 0.5], [0.0, 0.0], [1.0, 0.5], False, None, out, None,
                                           gv.reshape(2, 2, 500, 10))
    assert gx.shape == x.shape and bool(torch.isfinite(gx).all())


@pytest.mark.parametrize("train", [True, False])
def test_non_contiguous_batch1_input(train):
    """A batch-1 [b, d, t] feature map passed as .transpose(1, 2): reshape keeps a view whose rows are strided, which the
    fused path copies (as LFQ does) and then matches the stage-by-stage path."""
    from vector_quantization import GroupedResidualLFQ, ResidualLFQ

    torch.manual_seed(7)
    mods = [ResidualLFQ(dim=16, num_quantizers=4, codebook_size=2**16, frac_per_sample_entropy=0.5),
            GroupedResidualLFQ(dim=24, groups=2, num_quantizers=3, codebook_size=2**12)]
    for mod in mods:
        mod = mod.to(DEV).train(train)
        feats = torch.randn(1, mod.dim if isinstance(mod, GroupedResidualLFQ) else 16, 301, device=DEV)
        res = []
        for fused in (True, False):
            x = feats.clone().requires_grad_(True)
            inp = x.transpose(1, 2)
            assert not inp.is_contiguous()
            random.seed(2)
            torch.manual_seed(3)
            with contextlib.nullcontext() if fused else stagewise():
                out, idx, losses = mod(inp)
                if train:
                    (losses.sum() + (out * 0.3).sum()).backward()
            res.append((out.detach(), idx, losses.detach(), x.grad))
        (a_out, a_idx, a_l, a_g), (b_out, b_idx, b_l, b_g) = res
        assert a_out.shape == (1, 301, feats.shape[1]) and torch.equal(a_idx, b_idx) and torch.equal(a_out, b_out)
        torch.testing.assert_close(a_l, b_l, rtol=1e-5, atol=1e-6)
        if train:
            torch.testing.assert_close(a_g, b_g, rtol=1e-4, atol=1e-6 * max(1.0, float(b_g.abs().max())))
