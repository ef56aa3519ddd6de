"""The rotation trick through the modules on the GPU: one train step of a ``rotation_trick=True`` module against its
``rotation_trick=False`` twin (a deepcopy with the flag turned off).  Output, indices, losses, the EMA buffers after the step
and a learnable codebook's gradient are bit-identical; x.grad is within tests/rotation_dense.py's bound of the fp64 model for
the indices the forward chose, and the fused kernel agrees with the torch formulas (VQ_ROTATE_NO_FUSED=1).  Small shapes:
[2, 19, 32] rows, 16 codes."""
from __future__ import annotations

import copy
import random

import numpy as np
import pytest
import torch

import rotation_dense as rd
import train_dense as td

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, N, DIM, K = 2, 19, 32, 16


@pytest.fixture(autouse=True)
def reproducible_ema():
    """The EMA statistics are accumulated with float atomics unless torch asks for deterministic algorithms: two runs of ONE
    module would already differ in the last bits of embed_avg.  The comparisons with the twin are bit for bit, so they ask."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


def _params(dim, **kw):
    from vector_quantization.codebooks import CodebookParams

    kw.setdefault("threshold_ema_dead_code", 0)
    return CodebookParams(dim=dim, codebook_size=K, **kw)


def _build(kind, dim=DIM):
    import vector_quantization as vq
    from vector_quantization.codebooks import GumbelParams

    torch.manual_seed(3)
    if kind == "vq":
        m = vq.VectorQuantize(dim=dim, codebook_params=_params(dim), rotation_trick=True)
    elif kind == "vq_expiry":
        m = vq.VectorQuantize(dim=dim, codebook_params=_params(dim, threshold_ema_dead_code=2), rotation_trick=True)
    elif kind == "vq_heads":
        m = vq.VectorQuantize(dim=dim, codebook_dim=dim // 2, heads=2, separate_codebook_per_head=True,
                              codebook_params=_params(dim // 2), rotation_trick=True)
    elif kind == "vq_cosine":
        m = vq.VectorQuantize(dim=dim, codebook_params=_params(dim, use_cosine_sim=True), rotation_trick=True)
    elif kind == "vq_learnable":
        m = vq.VectorQuantize(dim=dim, codebook_params=_params(dim, learnable_codebook=True, ema_update=False), rotation_trick=True)
    elif kind == "vq_stochastic":
        m = vq.VectorQuantize(dim=dim, codebook_params=_params(dim, gumbel_params=GumbelParams(stochastic=True)),
                              rotation_trick=True)
    elif kind == "rvq":
        m = vq.ResidualVQ(dim=dim, num_quantizers=3, codebook_params=_params(dim), rotation_trick=True)
    elif kind == "rvq_shared":
        m = vq.ResidualVQ(dim=dim, num_quantizers=3, shared_codebook=True, codebook_params=_params(dim, ema_update=False),
                          rotation_trick=True)
    elif kind == "rvq_dropout":
        m = vq.ResidualVQ(dim=dim, num_quantizers=3, quantize_dropout=True, codebook_params=_params(dim), rotation_trick=True)
    elif kind == "grvq":
        m = vq.GroupedResidualVQ(dim=dim, groups=2, num_quantizers=2, codebook_params=_params(dim // 2), rotation_trick=True)
    else:
        raise ValueError(kind)
    return m.to(DEV).train()


def _twin(module):
    twin = copy.deepcopy(module)
    for m in twin.modules():
        if hasattr(m, "rotation_trick"):
            m.rotation_trick = False
    return twin


def _layout(kind, module, t, indices):
    """-> (t as the launch's rows [H, M, D], the stage codebooks [H, Q | 1, K, D], idx [H, M, Q], per_head, share) on the CPU;
    ``module`` is a copy made BEFORE the step (the EMA update rewrites the codes)."""
    b, n, dim = t.shape
    rows = b * n
    t, indices = t.detach().cpu(), indices.cpu()
    if kind.startswith("vq"):
        codes = module._codebook.embeddings.detach().cpu()
        if kind == "vq_heads":
            h = codes.shape[0]
            return (t.reshape(rows, h, dim // h).permute(1, 0, 2), codes[:, None], indices.reshape(rows, h).t()[..., None], False,
                    False)
        return t.reshape(1, rows, dim), codes[:, None], indices.reshape(1, rows, 1), False, False
    if kind.startswith("rvq"):
        share = kind == "rvq_shared"
        layers = module.layers[:1] if share else module.layers
        cb = torch.stack([layer._codebook.embeddings.detach()[0] for layer in layers])[None].cpu()
        return t.reshape(1, rows, dim), cb, indices.reshape(1, rows, -1), False, share
    G = module.groups
    cb = torch.stack([torch.stack([layer._codebook.embeddings.detach()[0] for layer in rvq.layers]) for rvq in module.rvqs]).cpu()
    return t.reshape(rows, G, dim // G).permute(1, 0, 2), cb, indices.reshape(G, rows, -1), True, False


def _step(module, x, go, seed=None, **kw):
    if seed is not None:
        torch.manual_seed(seed)
    xs = x.clone().requires_grad_(True)
    out, indices, loss = module(xs, **kw)[:3]
    ((out * go).sum() + loss.sum()).backward()
    return out.detach(), indices, loss.detach(), xs.grad


def _model(kind, before, x, go, indices, grad, *, denom=None):
    """-> (error / bound of ``grad``, the model, the bound); the commitment loss is weight 1 times the mean over the rows of a
    launch (of a head, for grouped stacks), so every stage's sq_err enters with 1 / denom."""
    flat, cb, idx, per_head, share = _layout(kind, before, x, indices)
    H, M, D = flat.shape
    run = int((idx[0, 0] >= 0).sum())  # (quantize dropout: the stages that ran)
    idx = idx[..., :run]
    if not share:
        cb = cb[:, :run]
    denom = denom if denom is not None else (M * D if per_head or kind.startswith("rvq") else H * M * D)
    ge = torch.full((H, run) if per_head else (run,), 1.0 / denom, dtype=torch.float64)
    g64, tol = rd.rotate_backward_model(flat, cb, idx, _layout(kind, before, go, indices)[0], ge, share=share, per_head=per_head)
    got = _layout(kind, before, grad, indices)[0].numpy()
    assert np.isfinite(got).all()
    return td.error_ratio(got, g64, tol), g64, tol


def _inputs(dim=DIM, n=N, seed=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, n, dim), generator=g).to(DEV), torch.randn((B, n, dim), generator=g).to(DEV)


@pytest.mark.parametrize("kind", ["vq", "vq_expiry", "vq_heads", "vq_cosine", "vq_learnable", "rvq", "rvq_shared", "grvq"])
def test_one_train_step_against_the_twin(kind, monkeypatch):
    module = _build(kind)
    twin, unfused, before = _twin(module), copy.deepcopy(module), copy.deepcopy(module)
    x, go = _inputs()
    out, indices, loss, grad = _step(module, x, go, seed=11)
    out_t, indices_t, loss_t, grad_t = _step(twin, x, go, seed=11)
    assert torch.equal(out, out_t) and torch.equal(indices, indices_t) and torch.equal(loss, loss_t)
    for (name, buf), (_, buf_t) in zip(module.named_buffers(), twin.named_buffers()):
        assert torch.equal(buf, buf_t), name
    for (name, p), (_, p_t) in zip(module.named_parameters(), twin.named_parameters()):
        assert (p.grad is None) == (p_t.grad is None), name
        if p.grad is not None:
            assert p.grad.abs().max() > 0 and torch.equal(p.grad, p_t.grad), name
    assert not torch.equal(grad, grad_t)
    ratio, g64, tol = _model(kind, before, x, go, indices, grad)
    print(f"{kind}: x.grad error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    twin_ratio = td.error_ratio(_layout(kind, before, grad_t, indices)[0].numpy(), g64, tol)
    assert twin_ratio > 1e2  # the straight-through gradient is another one
    # the torch formulas, stage by stage
    monkeypatch.setenv("VQ_ROTATE_NO_FUSED", "1")
    out_u, indices_u, loss_u, grad_u = _step(unfused, x, go, seed=11)
    assert torch.equal(out, out_u) and torch.equal(indices, indices_u) and torch.equal(loss, loss_u)
    ratio_u = td.error_ratio(_layout(kind, before, grad_u, indices)[0].numpy(), _layout(kind, before, grad, indices)[0].numpy(),
                             2.0 * tol)
    print(f"{kind}: fused against the torch formulas, difference / (2 bound) = {ratio_u:.3f}")
    assert ratio_u <= 1.0
    assert not torch.equal(grad, grad_u)  # (the switch switched: another order of operations, other last bits)


def test_masked_residual_stack(monkeypatch):
    """With the trick a masked stack walks its layers; the twin is sent the same way (VQ_RVQ_NO_FUSED_MASK=1), so that
    everything but x.grad on the kept rows is bit-identical."""
    monkeypatch.setenv("VQ_RVQ_NO_FUSED_MASK", "1")
    module = _build("rvq")
    twin, before = _twin(module), copy.deepcopy(module)
    x, go = _inputs()
    mask = torch.rand((B, N), generator=torch.Generator().manual_seed(4)) < 0.7
    assert 0 < int(mask.sum()) < B * N
    mask = mask.to(DEV)
    out, indices, loss, grad = _step(module, x, go, mask=mask)
    out_t, indices_t, loss_t, grad_t = _step(twin, x, go, mask=mask)
    assert torch.equal(out, out_t) and torch.equal(loss, loss_t) and torch.equal(indices, indices_t)
    for (name, buf), (_, buf_t) in zip(module.named_buffers(), twin.named_buffers()):
        assert torch.equal(buf, buf_t), name
    assert torch.equal(grad[~mask], grad_t[~mask])  # masked-out rows: the gradient they have without the trick
    assert not torch.equal(grad[mask], grad_t[mask])
    kept = int(mask.sum())
    _ratio, g64, tol = _model("rvq", before, x, go, indices, grad, denom=kept * DIM)
    keep = mask.reshape(-1).cpu().numpy()
    got = grad.detach().cpu().reshape(1, B * N, DIM).numpy()
    ratio = td.error_ratio(got[:, keep], g64[:, keep], tol[:, keep])
    print(f"masked rvq: kept rows' x.grad error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_quantize_dropout_with_a_fixed_seed():
    seed = next(s for s in range(100) if random.Random(s).randrange(0, 3) == 1)  # stages 0 and 1 run, stage 2 is dropped
    module = _build("rvq_dropout")
    twin, before = _twin(module), copy.deepcopy(module)
    x, go = _inputs()
    out, indices, loss, grad = _step(module, x, go, rand_quantize_dropout_fixed_seed=seed)
    out_t, indices_t, loss_t, grad_t = _step(twin, x, go, rand_quantize_dropout_fixed_seed=seed)
    assert torch.equal(out, out_t) and torch.equal(indices, indices_t) and torch.equal(loss, loss_t)
    assert (indices[..., 2] == -1).all() and (indices[..., :2] >= 0).all()
    for (name, buf), (_, buf_t) in zip(module.named_buffers(), twin.named_buffers()):
        assert torch.equal(buf, buf_t), name
    ratio, _g64, _tol = _model("rvq_dropout", before, x, go, indices, grad)
    print(f"rvq with quantize dropout: x.grad error / bound = {ratio:.3f}")
    assert ratio <= 1.0 and not torch.equal(grad, grad_t)


def test_stochastic_sampling_composes_with_the_trick():
    module = _build("vq_stochastic")
    twin, before = _twin(module), copy.deepcopy(module)
    x, go = _inputs()
    out, indices, loss, grad = _step(module, x, go, seed=21)
    out_t, indices_t, loss_t, grad_t = _step(twin, x, go, seed=21)
    assert torch.equal(indices, indices_t) and torch.equal(out, out_t) and torch.equal(loss, loss_t)
    ratio, _g64, _tol = _model("vq_stochastic", before, x, go, indices, grad)
    print(f"stochastic vq: x.grad error / bound = {ratio:.3f}")
    assert ratio <= 1.0 and not torch.equal(grad, grad_t)


def test_rows_wider_than_the_kernel_take_the_torch_formulas():
    from vector_quantization import native

    dim = 1028
    assert dim > native.ROTATE_MAX_DIM
    module = _build("vq", dim=dim)
    twin, before = _twin(module), copy.deepcopy(module)
    x, go = _inputs(dim=dim, n=5)
    out, indices, loss, grad = _step(module, x, go)
    out_t, indices_t, loss_t, grad_t = _step(twin, x, go)
    assert torch.equal(out, out_t) and torch.equal(indices, indices_t) and torch.equal(loss, loss_t)
    ratio, _g64, _tol = _model("vq", before, x, go, indices, grad)
    print(f"D = 1028 through the torch formulas: x.grad error / bound = {ratio:.3f}")
    assert ratio <= 1.0 and not torch.equal(grad, grad_t)
