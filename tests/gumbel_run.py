"""Shared by the host and the GPU test of the Gumbel relaxations: run one tests/golden/data/gumbel_<case>.npz fixture
through this package and compare with what the reference recorded; fp64 closed forms of the gradients."""
from __future__ import annotations

import numpy as np
import torch

from gumbel_cases import DIM, GUMBEL_CASES, K
from helpers import load_golden

GRAD_ATOL_OF_MAX, GRAD_RTOL = 2e-5, 2e-4  # the project's tolerance for vq_ce_backward_f32


def assert_grad_close(got, want, what, atol_of_max=GRAD_ATOL_OF_MAX, rtol=GRAD_RTOL):
    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    atol = atol_of_max * float(want.abs().max())
    err = (got - want).abs()
    worst = float((err - rtol * want.abs()).max())
    print(f"{what}: max err {float(err.max()):.3e} = {float(err.max()) / max(float(want.abs().max()), 1e-300):.2e} of the "
          f"largest entry (atol {atol:.3e})")
    assert worst <= atol, (what, float(err.max()), atol)


def run_fixture(name, device="cpu"):
    """-> (arrays, dict(quantize, embed_ind, loss, gx, gcb | None, module))"""
    import vector_quantization as vq
    from vector_quantization.codebook import Codebook
    from vector_quantization.codebooks import CodebookParams, GumbelParams

    c = GUMBEL_CASES[name]
    arrays, _meta = load_golden("gumbel_" + name)
    x = torch.from_numpy(arrays["x"]).to(device).requires_grad_(True)
    r = torch.from_numpy(arrays["r"]).to(device)
    cb = torch.from_numpy(arrays["cb"])
    if c["kind"] == "codebook":
        mod = Codebook(dim=DIM, codebook_size=K, ema_update=True, threshold_ema_dead_code=0,
                       gumbel_params=GumbelParams(**c["gumbel"]))
        with torch.no_grad():
            mod.embeddings.copy_(cb)
            mod.embed_avg.copy_(cb * 10.0)
            mod.cluster_size.fill_(10.0)
        mod = mod.to(device).train()
        q, ind, _ = mod(x, return_similarities=False)
        (q * r).sum().backward()
        return arrays, dict(quantize=q, embed_ind=ind, loss=torch.zeros(1), gx=x.grad, gcb=None, module=mod)
    vq_kw = dict(c.get("vq", {}))
    cos = c.get("cosine", False)
    norm = "l2norm" if cos else "identity"
    params = CodebookParams(dim=vq_kw.get("codebook_dim", DIM), codebook_size=K, learnable_codebook=True, ema_update=False,
                            use_cosine_sim=cos, transform_input=norm, weights_regularization=norm,
                            gumbel_params=GumbelParams(**c["gumbel"]))
    if "sgd_lr" in c:
        vq_kw["in_place_codebook_optimizer"] = lambda p: torch.optim.SGD(p, lr=c["sgd_lr"])
    mod = vq.VectorQuantize(dim=DIM, codebook_params=params, **vq_kw)
    with torch.no_grad():
        mod._codebook.embeddings.copy_(cb)
    mod = mod.to(device).train()
    kwargs = {}
    if "mask" in arrays:
        kwargs["mask"] = torch.from_numpy(arrays["mask"]).to(device)
    q, ind, loss, parts = mod(x, return_loss_breakdown=True, **kwargs)
    ((q * r).sum() + loss.sum()).backward()
    return arrays, dict(quantize=q, embed_ind=ind, loss=loss, gx=x.grad, gcb=mod._codebook.embeddings.grad, module=mod,
                        parts=parts)


def check_fixture(name, device="cpu"):
    arrays, res = run_fixture(name, device)
    assert np.array_equal(res["embed_ind"].cpu().numpy(), arrays["embed_ind"]), "indices differ from the reference"
    np.testing.assert_allclose(res["quantize"].detach().cpu().numpy(), arrays["quantize"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(res["loss"].detach().cpu().numpy(), arrays["loss"], rtol=1e-6, atol=1e-7)
    assert_grad_close(res["gx"], arrays["gx"], f"{name} dL/dx")
    if "gcb" in arrays:
        assert_grad_close(res["gcb"], arrays["gcb"], f"{name} dL/dcodebook")
    if "cb_after" in arrays:
        mod = res["module"]
        codes = (mod._codebook.embeddings if hasattr(mod, "_codebook") else mod.embeddings).detach().cpu().numpy()
        np.testing.assert_allclose(codes, arrays["cb_after"], rtol=1e-5, atol=1e-6)
    if "inplace_loss" in arrays:
        np.testing.assert_allclose(float(res["parts"].inplace_optimize.detach()), float(arrays["inplace_loss"]), rtol=1e-6)
    return arrays, res


# ------------------------------------------------------------------------------------------------ fp64 closed forms
def similarities64(x, c, metric_dot):
    return x @ c.transpose(-1, -2) if metric_dot else -torch.cdist(x, c)


def logsumexp64(x, c, tau, metric_dot, dtype=torch.float64):
    """Natural-log logsumexp_k(tau s) [H, M] in ``dtype`` (what vq_gumbel_stats_f32 returns as lse2, times log 2)."""
    return (similarities64(x.to(dtype), c.to(dtype), metric_dot) * tau).logsumexp(-1)


def closed_form64(x, c, g, ind, tau, metric_dot, reinmax=False, dtype=torch.float64):
    """(delta, gx, gc_sim, gc) of the module docstring of vector_quantization.gumbel, dense, in ``dtype``: x [H, M, D],
    c [H, K, D], g [H, M, D], ind [H, M].  ``dtype=torch.float32`` is the reference's own op sequence at its precision."""
    x, c, g = x.to(dtype), c.to(dtype), g.to(dtype)
    s = similarities64(x, c, metric_dot)
    a = g @ c.transpose(-1, -2)
    onehot = torch.nn.functional.one_hot(ind, c.shape[1]).to(dtype)
    if reinmax:
        p0 = s.softmax(-1)
        p1 = ((onehot + (s * tau).softmax(-1)) / 2).clamp(min=1e-5)
        pi = p1 / p1.sum(dim=1, keepdim=True)
        e = (pi * a).sum(dim=1, keepdim=True)
        delta = (p0 * a).sum(-1, keepdim=True)
        w = 2 * pi * (a - e) - 0.5 * p0 * (a - delta)
    else:
        p = (s * tau).softmax(-1)
        delta = (p * a).sum(-1, keepdim=True)
        w = tau * p * (a - delta)
    if metric_dot:
        gx, gc = w @ c, w.transpose(-1, -2) @ x
    else:
        ratio = torch.where(s == 0, torch.zeros_like(w), w / s)
        gx = x * ratio.sum(-1, keepdim=True) - ratio @ c
        gc = c * ratio.sum(-2).unsqueeze(-1) - ratio.transpose(-1, -2) @ x
    return delta[..., 0], gx, gc, gc + onehot.transpose(-1, -2) @ g
