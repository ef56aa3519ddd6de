"""Shared by the host and the GPU test of the fused orthogonal regularisation loss (vq_orthogonal_gram_f32, the kOrth role of
the sweep; losses._OrthogonalFn): the fp64 closed form without autograd, the reference's five ops with autograd at a chosen
precision, and the project's tolerance rule (tests/gumbel_run.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from gumbel_run import GRAD_ATOL_OF_MAX, GRAD_RTOL, assert_grad_close  # noqa: F401  (re-exported: the project's tolerance)

EPS = 1e-12  # F.normalize's clamp of the norm


def gram64(rows):
    """rows [h, n, d] AS GIVEN (no normalisation), fp64 -> (rowsq [h, n], G [h, n, d]): what vq_orthogonal_gram_f32 computes."""
    rows = rows.double()
    cos = rows @ rows.transpose(-1, -2)
    return (cos * cos).sum(-1), cos @ rows


def closed_form64(codes):
    """-> dict(loss, rowsq, G, grad) in fp64, no autograd: the loss of utils/losses.py:23-28, the row sums of squared cosines,
    the gram matrix times the normalised rows, and d loss / d codes through F.normalize (its clamp of the norm included)."""
    codes = codes.detach().double()
    h, n, _ = codes.shape
    norm = codes.norm(dim=-1, keepdim=True)
    denom = norm.clamp_min(EPS)
    normed = codes / denom
    rowsq, G = gram64(normed)
    loss = rowsq.sum() / (h * n ** 2) - 1 / n
    gn = 4 * G / (h * n ** 2)  # d loss / d normed: cos is symmetric, row i appears on both sides
    # normed = codes / denom, denom = max(|codes|, eps): the clamp passes the gradient on where |codes| >= eps, and the
    # norm's (sub)gradient at 0 is 0
    through = torch.where(norm >= EPS, (gn * codes).sum(-1, keepdim=True) / (denom ** 2 * norm.clamp_min(1e-300)), torch.zeros_like(norm))
    # grad_scale: the size of the two terms whose difference the gradient is (the normalisation removes the radial part: at
    # n = 1 all of it), which is what a rounding error of the gradient is relative to
    return dict(loss=loss, rowsq=rowsq, G=G, grad=gn / denom - through * codes, normed=normed, grad_scale=float((gn / denom).abs().max()))


def reference_sequence(codes, dtype, normalize=True):
    """The reference's five ops with autograd in ``dtype`` on the device of ``codes`` -> dict(loss, rowsq, G, grad): rowsq and G
    are what its own sequence holds for them -- (cos ** 2).sum(-1), and d loss / d normed * h n^2 / 4 from autograd.
    ``normalize=False``: the rows as given stand for ``normed`` (the kernel's view of general rows)."""
    leaf = codes.detach().to(dtype).requires_grad_(True)
    h, n = leaf.shape[:2]
    normed = F.normalize(leaf, p=2, dim=-1) if normalize else leaf * 1
    normed.retain_grad()
    cos = normed @ normed.transpose(-1, -2)
    sq = cos ** 2
    loss = sq.sum() / (h * n ** 2) - (1 / n)
    loss.backward()
    return dict(loss=loss.detach(), rowsq=sq.detach().sum(-1), G=normed.grad * (h * n ** 2 / 4), grad=leaf.grad)


def make_codes(h, n, d, seed, unit=False):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randn((h, n, d), generator=g, dtype=torch.float32)
    return F.normalize(codes, dim=-1) if unit else codes


def rule(case, what, have, want, r32):
    """assert_grad_close with atol = max(GRAD_ATOL_OF_MAX, 4 x the error of the reference's own fp32 sequence ``r32`` against
    fp64 ``want``) of the largest fp64 entry, and GRAD_RTOL; prints the reference's error and the kernel's."""
    want = torch.as_tensor(want).detach().double().cpu()
    have = torch.as_tensor(have).detach().double().cpu().reshape(want.shape)
    r32 = torch.as_tensor(r32).detach().double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(have).all()), (case, what)
    ref_err = float((r32 - want).abs().max() / max(float(want.abs().max()), 1e-300))
    print(f"{case} {what}: the reference's fp32 sequence is {ref_err:.2e} of the largest entry off fp64")
    assert_grad_close(have, want, f"{case} {what}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * ref_err))
