"""What the host and the GPU tests of the masked residual stack share: the seeded inputs of tests/golden/rvq_mask_cases.py,
the drop-in module built on them, one forward (+ backward) of it, and the comparison with the fixture.  A plain module: it
holds no test."""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

from helpers import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from gen import CB_SEED, make_rvq_codebooks, make_x, poison_  # noqa: E402
from rvq_mask_cases import BY_NAME, CASES, DIM, GROUPS, K, Q, X_SHAPE, make_mask  # noqa: E402,F401


def q_weights(shape):
    """Same seeded weights as tests/golden/make_golden.py:q_weights."""
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(4242))


def case_inputs(c):
    """-> (x [b, n, G * DIM], codebooks [G, Q, K, DIM] as the generator placed them, mask [b, n])."""
    G = GROUPS if c["kind"] == "grvq" else 1
    cbs = torch.stack([make_rvq_codebooks(Q, K, DIM, "S", seed=CB_SEED + 100 * g) for g in range(G)])
    if c["shared_codebook"]:
        cbs = cbs[:, :1].expand(G, Q, K, DIM).contiguous()
    x = make_x((*X_SHAPE[:-1], G * DIM), "S")
    poison_(x, cbs[0], c["nonfinite"])
    return x, cbs, make_mask()


def dropout_cut(c):
    """The last stage that runs: python's random.Random(seed), as the reference draws it."""
    extra = c["rvq_extra"]
    if not (extra.get("quantize_dropout") and c["training"]):
        return Q - 1
    return random.Random(c["fwd_extra"]["rand_quantize_dropout_fixed_seed"]).randrange(extra["quantize_dropout_cutoff_index"], Q)


def same(got, want):
    """torch.equal, with a NaN equal to a NaN (the non-finite cases)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(got, want, equal_nan=True))


def rel_close(got, want, rtol=1e-5):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= rtol * np.abs(want)))


def grad_close(got, want, rtol=1e-5):
    """1e-5 of the gradient's scale: its elements are sums of terms of either sign."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.abs(got - want).max() <= rtol * np.abs(want).max())


def layers_of(mod):
    return [layer for rvq in (mod.rvqs if hasattr(mod, "rvqs") else [mod]) for layer in rvq.layers]


def build_module(c, cbs, device="cpu", **rvq_extra):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    params = CodebookParams(dim=DIM, codebook_size=cbs.shape[-2], **c["cb_extra"])
    extra = {**c["rvq_extra"], **rvq_extra}
    if c["kind"] == "grvq":
        mod = vq.GroupedResidualVQ(dim=cbs.shape[0] * DIM, groups=cbs.shape[0], num_quantizers=cbs.shape[1], codebook_params=params,
                                   **extra)
        rvqs = list(mod.rvqs)
    else:
        mod = vq.ResidualVQ(dim=DIM, num_quantizers=cbs.shape[1], codebook_params=params, shared_codebook=c["shared_codebook"],
                            **extra)
        rvqs = [mod]
    with torch.no_grad():
        for g, rvq in enumerate(rvqs):
            for i, layer in enumerate(rvq.layers):
                layer._codebook.embeddings.copy_(cbs[g, i][None])
                layer._codebook.embed_avg.copy_(cbs[g, i][None])
    mod = mod.to(device)
    return mod.train() if c["training"] else mod.eval()


def forward_backward(mod, c, x, mask, fwd_extra=None):
    """One forward (and, for the cases with ``grad``, the backward of losses.sum() + <q, q_weights>) ->
    (q, idx, losses, x.grad | None), detached."""
    kwargs = dict(mask=mask)
    if c["kind"] != "grvq":
        kwargs.update(c["fwd_extra"] if fwd_extra is None else fwd_extra)
    if c["training"]:
        kwargs["freeze_codebook"] = c["freeze_codebook"]
    x = x.detach().clone().requires_grad_(c["grad"])
    with torch.set_grad_enabled(c["grad"]):
        q, idx, losses = mod(x, **kwargs)[:3]
    grad = None
    if c["grad"]:
        (losses.sum() + (q * q_weights(q.shape).to(q.device)).sum()).backward()
        grad = x.grad
    return q.detach(), idx, losses.detach(), grad


def run_case(c, device="cpu"):
    x, cbs, mask = case_inputs(c)
    mod = build_module(c, cbs, device)
    return (mod, *forward_backward(mod, c, x.to(device), mask.to(device)))


def ema_state(mod):
    return {attr: torch.stack([getattr(layer._codebook, attr) for layer in layers_of(mod)]).detach().cpu()
            for attr in ("embeddings", "embed_avg", "cluster_size")}


def check_against_fixture(c, mod, q, idx, losses, grad):
    arrays, _ = load_golden(c["name"])
    assert np.array_equal(idx.cpu().numpy(), arrays["idx"].astype(np.int64)), "indices"
    assert same(q.cpu().numpy(), arrays["q_full"]), "quantized output"
    assert rel_close(losses.cpu().numpy(), arrays["loss"]), "losses"
    if c["grad"]:
        assert grad_close(grad.cpu().numpy(), arrays["g_full"]), "d loss / d x"
    if c["training"] and not c["freeze_codebook"]:
        for attr, got in ema_state(mod).items():
            assert np.allclose(got.numpy(), arrays["ema_" + attr], rtol=1e-5, atol=1e-6), attr
