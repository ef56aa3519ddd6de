"""CPU checks of the rotation trick: tests/rotation_dense.py's closed form is the fp64 autograd of the literal composition,
its bound bites, the modules run the same formulas in torch through helpers.OracleBackend (a backend without the native
entry) and change nothing but x.grad, and the constructor refuses the combinations where another rule defines the gradient."""
from __future__ import annotations

import copy
import os

import numpy as np
import pytest
import torch

import rotation_dense as rd
import train_dense as td
from helpers import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "vq_rotate_backward_f32"


# ------------------------------------------------------------------------------------------------
# the closed form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("D", [1, 3, 64, 260])
def test_closed_form_equals_fp64_autograd_of_the_literal_composition(D, Q):
    per_head = D == 64
    x, cb, idx, go, ge, rows = rd.degenerate_inputs(2, 9, D, Q, 5, 40 + D + Q, per_head=per_head)
    want, value_err = rd.literal_autograd(x, cb, idx, go, ge, share=False, per_head=per_head)
    got, _ = rd.rotate_backward_model(x, cb, idx, go, ge, share=False, per_head=per_head, chain_dtype=np.float64)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.1
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert value_err <= 1e-12  # rot(r) is c
    # every term matters on these inputs: without the loss term, or without the rotation, the result is another one
    no_loss, _ = rd.rotate_backward_model(x, cb, idx, go, None, share=False, per_head=per_head, chain_dtype=np.float64)
    no_rot, _ = rd.rotate_backward_model(x, cb, idx, None, ge, share=False, per_head=per_head, chain_dtype=np.float64)
    assert np.abs(no_loss - want).max() > 1e-3 and np.abs(no_rot - want).max() > 1e-3
    assert np.abs(no_loss + no_rot - want).max() <= 1e-12 * np.abs(want).max()


def test_shared_codebook_closed_form_equals_autograd():
    x, cb, idx, go, ge, _ = rd.degenerate_inputs(2, 9, 7, 3, 5, 77, share=True)
    want, _ = rd.literal_autograd(x, cb, idx, go, ge, share=True, per_head=False)
    got, _ = rd.rotate_backward_model(x, cb, idx, go, ge, share=True, per_head=False, chain_dtype=np.float64)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_degenerate_rows_follow_the_formula():
    x, cb, idx, go, _ge, (anti, same, zero_x, zero_c) = rd.degenerate_inputs(1, 9, 16, 2, 5, 5)
    g, tol = rd.rotate_backward_model(x, cb, idx[..., :1], go, None, share=False, per_head=False)
    assert np.isfinite(g).all() and np.isfinite(tol).all()
    god, xd, c0 = go.double().numpy()[0], x.double().numpy()[0], cb.double().numpy()[0, 0]
    # c = -r: w = 0 and lam = 1, u = r / |r|, qh = -u  ->  g - 2 (g.u) u
    u = xd[anti] / np.linalg.norm(xd[anti])
    assert np.allclose(g[0, anti], god[anti] - 2 * (god[anti] @ u) * u, rtol=0, atol=1e-6)
    # c = r: the rotation is the identity
    assert np.allclose(g[0, same], god[same], rtol=0, atol=1e-6)
    # x = 0: u = 0, s = qh, lam = |c| / eps  ->  lam (g - 2 (g.qh) qh)
    c = c0[idx[0, zero_x, 0]]
    qh = c / np.linalg.norm(c)
    assert np.allclose(g[0, zero_x], np.linalg.norm(c) / rd.EPS * (god[zero_x] - 2 * (god[zero_x] @ qh) * qh), rtol=1e-9)
    # a zero code: no gradient through the output
    assert not g[0, zero_c].any()


# ------------------------------------------------------------------------------------------------
# the bound bites
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", td.backward_cases()[::5], ids=str)
def test_wrong_models_fall_outside_the_bound(case):
    D, Q, H, _ste, per_head = case
    x, cb, idx, go, ge = td.backward_case_inputs(*case)
    kw = dict(share=False, per_head=per_head)
    g, tol = rd.rotate_backward_model(x, cb, idx, go, ge, **kw)
    assert np.isfinite(tol).all() and (tol > 0).all()
    if D > 1:  # a rounding-error bound, not a loose one (D = 1: every other row is antipodal, s = 0, and takes the cap)
        assert np.median(tol / np.maximum(np.abs(g), 1e-30)) < 1e-3
    no_u, _ = rd.rotate_backward_model(x, cb, idx, go, ge, drop_u_term=True, **kw)
    assert td.error_ratio(no_u, g, tol) > 1e2
    lam1, _ = rd.rotate_backward_model(x, cb, idx, go, ge, unit_lam=True, **kw)
    assert td.error_ratio(lam1, g, tol) > 1e2


def test_fp32_torch_formulas_are_within_the_bound():
    """search.rotate_backward_rows without a native entry (OracleBackend): the stage-by-stage torch formulas."""
    from vector_quantization import search

    search.set_backend(OracleBackend)
    try:
        for D, Q, per_head in ((1, 1, False), (3, 2, True), (64, 3, False), (260, 2, True)):
            x, cb, idx, go, ge, _ = rd.degenerate_inputs(2, 9, D, Q, 5, 90 + D, per_head=per_head)
            got = search.rotate_backward_rows(x, cb, idx, go, ge, sq_err_per_head=per_head)
            g, tol = rd.rotate_backward_model(x, cb, idx, go, ge, share=False, per_head=per_head)
            ratio = td.error_ratio(got.numpy(), g, tol)
            print(f"rotate torch formulas D={D} Q={Q}: error / bound = {ratio:.3f}")
            assert ratio <= 1.0
    finally:
        search.set_backend(None)


# ------------------------------------------------------------------------------------------------
# modules on the CPU through OracleBackend
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def oracle_backend():
    from vector_quantization import search

    search.set_backend(OracleBackend)
    try:
        yield
    finally:
        search.set_backend(None)


def _params(dim, **kw):
    from vector_quantization.codebooks import CodebookParams

    return CodebookParams(dim=dim, codebook_size=16, threshold_ema_dead_code=0, **kw)


def _build(kind, rotation_trick=True):
    import vector_quantization as vq

    torch.manual_seed(3)
    if kind == "vq":
        return vq.VectorQuantize(dim=32, codebook_params=_params(32), rotation_trick=rotation_trick)
    if kind == "rvq":
        return vq.ResidualVQ(dim=32, num_quantizers=3, codebook_params=_params(32), rotation_trick=rotation_trick)
    return vq.GroupedResidualVQ(dim=32, groups=2, num_quantizers=2, codebook_params=_params(16), rotation_trick=rotation_trick)


def _codes_and_rows(kind, module, x, indices):
    """-> (flat x [H, M, D], stage codebooks [H, Q, K, D], idx [H, M, Q], commitment weight / elements per stage sum)."""
    b, n, dim = x.shape
    if kind == "vq":
        return x.reshape(1, b * n, dim), module._codebook.embeddings.detach()[:, None].clone(), indices.reshape(1, b * n, 1)
    if kind == "rvq":
        cb = torch.stack([layer._codebook.embeddings.detach()[0] for layer in module.layers])[None].clone()
        return x.reshape(1, b * n, dim), cb, indices.reshape(1, b * n, -1)
    G = module.groups
    cb = torch.stack([torch.stack([layer._codebook.embeddings.detach()[0] for layer in rvq.layers]) for rvq in module.rvqs]).clone()
    return x.reshape(b * n, G, dim // G).permute(1, 0, 2), cb, indices.reshape(G, b * n, -1)


def _step(module, x, go):
    xs = x.clone().requires_grad_(True)
    out, indices, loss = module(xs)
    ((out * go).sum() + loss.sum()).backward()
    return out.detach(), indices, loss.detach(), xs.grad


@pytest.mark.parametrize("kind", ["vq", "rvq", "grvq"])
def test_modules_change_nothing_but_the_gradient(kind, oracle_backend):
    module = _build(kind).train()
    twin = copy.deepcopy(module)
    for m in twin.modules():
        if hasattr(m, "rotation_trick"):
            m.rotation_trick = False
    codes_before = copy.deepcopy(module)
    g = torch.Generator().manual_seed(8)
    x, go = torch.randn((2, 19, 32), generator=g), torch.randn((2, 19, 32), generator=g)
    out, indices, loss, grad = _step(module, x, go)
    out_t, indices_t, loss_t, grad_t = _step(twin, x, go)
    assert torch.equal(out, out_t) and torch.equal(indices, indices_t) and torch.equal(loss, loss_t)
    for (name, buf), (_, buf_t) in zip(module.named_buffers(), twin.named_buffers()):
        assert torch.equal(buf, buf_t), name
    assert not torch.equal(grad, grad_t)
    flat, cb, idx = _codes_and_rows(kind, codes_before, x, indices)
    H, M, D = flat.shape
    Q = idx.shape[-1]
    ge = torch.full((H, Q), 1.0 / (M * D), dtype=torch.float64)  # commitment_weight 1, mean over the rows of a head
    flat_go = _codes_and_rows(kind, codes_before, go, indices)[0]
    g64, tol = rd.rotate_backward_model(flat, cb, idx, flat_go, ge, share=False, per_head=True)
    got = _codes_and_rows(kind, codes_before, grad, indices)[0]
    ratio = td.error_ratio(got.numpy(), g64, tol)
    print(f"{kind} on the CPU: error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # and the twin's gradient is the straight-through one, far outside the bound
    twin_got = _codes_and_rows(kind, codes_before, grad_t, indices)[0]
    assert td.error_ratio(twin_got.numpy(), g64, tol) > 1e2


def test_eval_mode_ignores_the_flag(oracle_backend):
    module = _build("vq").eval()
    twin = _build("vq", rotation_trick=False).eval()
    x = torch.randn(2, 19, 32, generator=torch.Generator().manual_seed(9))
    xs, xt = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out, indices, loss = module(xs)
    out_t, indices_t, loss_t = twin(xt)
    assert torch.equal(out, out_t) and torch.equal(indices, indices_t) and torch.equal(loss, loss_t)
    assert not out.requires_grad and not out_t.requires_grad  # an eval-mode gather: nothing to differentiate, flag or not


def test_masked_residual_stacks_take_the_layer_loop():
    from vector_quantization import residual

    module = _build("rvq").train()
    x = torch.zeros(2, 19, 32)
    mask = torch.ones(2, 19, dtype=torch.bool)
    assert not residual._mask_fusable(module.layers, x, mask)
    assert not module._fusable(x, mask, False)


# ------------------------------------------------------------------------------------------------
# constructor and ABI
# ------------------------------------------------------------------------------------------------
def test_constructor_refuses_other_gradient_rules():
    import vector_quantization as vq
    from vector_quantization.codebooks import AffineParameters, GumbelParams

    def build(params=None, **kw):
        return vq.VectorQuantize(dim=8, codebook_params=params or _params(8), rotation_trick=True, **kw)

    with pytest.raises(ValueError):
        build(_params(8, gumbel_params=GumbelParams(straight_through=True)))
    with pytest.raises(ValueError):
        build(_params(8, gumbel_params=GumbelParams(straight_through=True, reinmax=True)))
    with pytest.raises(ValueError):
        build(_params(8, learnable_codebook=True, ema_update=False), sync_update_v=0.5)
    with pytest.raises(NotImplementedError):
        build(_params(8, learnable_codebook=True, ema_update=False), in_place_codebook_optimizer=lambda p: torch.optim.SGD(p, lr=0.1))
    with pytest.raises(NotImplementedError):
        build(_params(8, use_affine=True, affine_params=AffineParameters(sync=False)))
    with pytest.raises(ValueError):
        vq.ResidualVQ(dim=8, num_quantizers=2, codebook_params=_params(8, gumbel_params=GumbelParams(straight_through=True)),
                      rotation_trick=True)
    build()  # the plain module, plain stochastic sampling and a learnable codebook are fine
    build(_params(8, gumbel_params=GumbelParams(stochastic=True)))
    build(_params(8, learnable_codebook=True, ema_update=False))


def test_sharded_codebook_is_refused():
    import vector_quantization as vq

    # (the check runs before the process group is looked at)
    with pytest.raises(NotImplementedError):
        vq.VectorQuantize(dim=8, codebook_params=_params(8), rotation_trick=True, codebook_shard_group=True)


def test_symbol_is_declared_bound_and_exported():
    from vector_quantization import native

    header = open(os.path.join(ROOT, "include", "vq_mi355x.h")).read()
    assert f"int {ENTRY}(const vq_args *a, const float *grad_out" in header
    assert ENTRY in native._SIGNATURES and ENTRY in native.EXPORTED_SYMBOLS
    assert native._SIGNATURES[ENTRY] == native._SIGNATURES["vq_quantize_backward_f32"]
    assert native.ROTATE_MAX_DIM == 1024 and callable(native.rotate_backward)
    assert hasattr(native.load(), ENTRY)
