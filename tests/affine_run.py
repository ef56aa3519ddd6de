"""Shared by the host and the GPU tests of use_affine codebooks: run one tests/golden/data/affine_<case>.npz fixture through
this package, step by step, and compare with what the reference recorded after every step."""
from __future__ import annotations

import json

import numpy as np
import torch

from affine_cases import AFFINE, AFFINE_CASES, DIM, K
from check_case import Q_TOL
from helpers import load_golden

STAT_RTOL = STAT_ATOL = 1e-6  # the statistics buffers: the same fp32 op sequence (host) / the bound of the kernel tests (GPU)


def build_module(name, device="cpu"):
    """-> (module, its Codebook, arrays, case)"""
    import vector_quantization as vq
    from vector_quantization.codebook import Codebook
    from vector_quantization.codebooks import AffineParameters, CodebookParams

    c = AFFINE_CASES[name]
    arrays, _meta = load_golden("affine_" + name)
    h = c.get("heads", 1)
    cos = c.get("cosine", False)
    learnable = c.get("learnable", False)
    common = dict(dim=DIM, codebook_size=K, num_codebooks=h, threshold_ema_dead_code=0, learnable_codebook=learnable,
                  ema_update=not learnable, use_affine=True, affine_params=AffineParameters(**AFFINE), use_cosine_sim=cos,
                  weights_regularization="l2norm" if cos else "identity")
    if c["kind"] == "codebook":
        mod = book = Codebook(**common)
    else:
        mod = vq.VectorQuantize(dim=DIM, codebook_params=CodebookParams(**common), **c.get("vq", {}))
        book = mod._codebook
    cb = torch.from_numpy(arrays["cb"])
    with torch.no_grad():
        book.embeddings.copy_(cb)
        book.embed_avg.copy_(cb * 10.0)
        book.cluster_size.fill_(10.0)
    return mod.to(device), book, arrays, c


def run_step(mod, book, arrays, c, s, device="cpu"):
    """One forward (+ backward) of step ``s`` -> dict(quantize, embed_ind, loss | None, gx | None, gcb | None)"""
    step = c["steps"][s]
    mod.train(step["train"])
    x = torch.from_numpy(arrays[f"x{s}"]).to(device).requires_grad_(True)
    r = torch.from_numpy(arrays[f"r{s}"]).to(device)
    kwargs = {}
    if step["mask"]:
        kwargs["mask"] = torch.from_numpy(arrays[f"mask{s}"]).to(device)
    loss = None
    if c["kind"] == "vq":
        q, ind, loss = mod(x, **kwargs)
        objective = (q * r).sum() + loss.sum()
    else:
        q, ind, _ = mod(x, return_similarities=False, **kwargs)
        objective = (q * r).sum()
    if objective.requires_grad:
        book.embeddings.grad = None
        objective.backward()
    gcb = book.embeddings.grad if c.get("learnable", False) else None
    return dict(quantize=q, embed_ind=ind, loss=loss, gx=x.grad, gcb=gcb)


def check_buffers(book, arrays, s, stat_rtol=STAT_RTOL, stat_atol=STAT_ATOL):
    for name in ("batch_mean", "batch_variance", "codebook_mean", "codebook_variance"):
        got = getattr(book, name).detach().cpu().numpy()
        np.testing.assert_allclose(got, arrays[f"{name}{s}"], rtol=stat_rtol, atol=stat_atol, err_msg=f"{name} after step {s}")
    for name in ("codebook_mean_needs_init", "codebook_variance_needs_init"):
        assert np.array_equal(getattr(book, name).cpu().numpy(), arrays[f"{name}{s}"]), name
    # the project's tolerances for the EMA buffers (check_case.compare)
    np.testing.assert_allclose(book.cluster_size.detach().cpu().numpy(), arrays[f"cluster_size{s}"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(book.embed_avg.detach().cpu().numpy(), arrays[f"embed_avg{s}"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(book.embeddings.detach().cpu().numpy(), arrays[f"embeddings{s}"], rtol=1e-4, atol=1e-5)


def check_fixture(name, device="cpu", **stat_tol):
    mod, book, arrays, c = build_module(name, device)
    for s in range(len(c["steps"])):
        res = run_step(mod, book, arrays, c, s, device)
        got_ind = res["embed_ind"].cpu().numpy()
        assert res["embed_ind"].dtype == torch.int64 and got_ind.shape == arrays[f"embed_ind{s}"].shape
        assert np.array_equal(got_ind, arrays[f"embed_ind{s}"]), f"step {s}: indices differ from the reference"
        np.testing.assert_allclose(res["quantize"].detach().cpu().numpy(), arrays[f"quantize{s}"], atol=Q_TOL, rtol=0)
        if res["loss"] is not None:
            np.testing.assert_allclose(res["loss"].detach().cpu().numpy(), arrays[f"loss{s}"], atol=Q_TOL, rtol=1e-5)
        want_gx = arrays[f"gx{s}"]
        got_gx = res["gx"].cpu().numpy() if res["gx"] is not None else np.zeros_like(want_gx)
        scale = max(float(np.abs(want_gx).max()), 1e-12)
        np.testing.assert_allclose(got_gx, want_gx, atol=1e-5 * scale, rtol=1e-4, err_msg=f"step {s}: dL/dx")
        if f"gcb{s}" in arrays:
            want = arrays[f"gcb{s}"]
            np.testing.assert_allclose(res["gcb"].cpu().numpy(), want, atol=1e-5 * float(np.abs(want).max()), rtol=1e-4,
                                       err_msg=f"step {s}: dL/dembeddings")
        check_buffers(book, arrays, s, **stat_tol)
        if s == 0:
            assert list(book.state_dict().keys()) == json.loads(bytes(arrays["state_keys_json"]).decode())
    return mod, book, arrays


def dense_effective_codes(book):
    """fp64 model of the codes a forward searches, from the module's buffers as they stand."""
    cstd = book.codebook_variance.double().clamp(min=1e-5).sqrt()
    bstd = book.batch_variance.double().clamp(min=1e-5).sqrt()
    return (book.embeddings.detach().double() - book.codebook_mean.double()) * (bstd / cstd) + book.batch_mean.double()
