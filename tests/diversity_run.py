"""Shared by the host and the GPU test of the fused codebook diversity loss (vq_diversity_*_f32): inputs, the fp64 closed
form of the loss and of its gradient with respect to the rows, and the reference's own op sequence built from plain torch
ops and autograd (vector_quantize_pytorch.py:324-334 with utils/general.py:25-30), both on the CPU.

Rows: x [H, M, D]; the sequence position of row m of every head is (m // pos_div) % N, every position has C = H * M / N
rows over all heads.  With ``live`` the gradient flows through the similarities the way _SimilarityFn does it for an EMA
codebook: the weights from ``c``, the contraction with ``live``."""
from __future__ import annotations

import torch

CLAMP = 1e-5


def make_inputs(h, b, n, k, d, metric_dot, seed, pos_div=1):
    """x [H, B * N * pos_div, D], c [H, K, D] on the CPU (fp32).  Dot products are kept small so that softmax(-T s) at T = 100
    spreads over more than one code."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((h, b * n * pos_div, d), generator=g)
    c = torch.randn((h, k, d), generator=g)
    if metric_dot:
        x = x * (0.25 / max(1.0, d ** 0.5))
    return x, c


def positions(m, n, pos_div):
    return (torch.arange(m) // pos_div) % n


def similarities(x, c, metric_dot):
    return x @ c.transpose(-1, -2) if metric_dot else -torch.cdist(x, c)


class _LiveSimilarity(torch.autograd.Function):
    """similarities(x, c) whose backward multiplies with ``live`` instead of c (losses._SimilarityFn with live_codes)."""

    @staticmethod
    def forward(ctx, x, c, live, metric_dot):
        s = similarities(x, c, metric_dot)
        ctx.save_for_backward(x, live, s)
        ctx.metric_dot = metric_dot
        return s

    @staticmethod
    def backward(ctx, g):
        x, live, s = ctx.saved_tensors
        if ctx.metric_dot:
            return g @ live, None, None, None
        ratio = torch.where(s == 0, torch.zeros_like(g), g / s)
        return x * ratio.sum(-1, keepdim=True) - ratio @ live, None, None, None


def reference_sequence(x, c, temperature, n, pos_div, metric_dot, dtype=torch.float32, live=None, g_loss=1.0):
    """The reference's op sequence in ``dtype`` with autograd -> dict(loss, A [N, K], gx [H, M, D], lse [H, M] natural log)."""
    x = x.to(dtype).clone().requires_grad_(True)
    c = c.to(dtype)
    h, m, _ = x.shape
    k = c.shape[1]
    if live is None:
        s = similarities(x, c, metric_dot)
    else:
        s = _LiveSimilarity.apply(x, c, live.to(dtype), metric_dot)
    z = -s * temperature
    prob = z.softmax(dim=-1)
    # reduce(prob, "... n l -> n l", "mean"): rows are (batch, position, pos_div) in this order
    avg = prob.reshape(h, m // (n * pos_div), n, pos_div, k).mean(dim=(0, 1, 3))
    ent = (-avg * avg.clamp(min=CLAMP).log()).sum(dim=-1)
    loss = -ent.mean()
    (loss * g_loss).backward()
    return dict(loss=loss.detach(), A=avg.detach(), gx=x.grad, lse=z.detach().logsumexp(-1))


def closed_form64(x, c, temperature, n, pos_div, metric_dot, live=None, g_loss=1.0, dtype=torch.float64):
    """The formulas of DESIGN.md ("Codebook diversity loss") in ``dtype``, no autograd -> dict(loss, A, U, delta [H, M], gx,
    lse [H, M] natural log).  ``dtype=torch.float32`` gives delta and U at the precision of the reference's op sequence."""
    x, c = x.to(dtype), c.to(dtype)
    l = c if live is None else live.to(dtype)
    h, m, _ = x.shape
    k = c.shape[1]
    count = h * m // n
    pos = positions(m, n, pos_div)
    s = similarities(x, c, metric_dot)
    z = -temperature * s
    p = z.softmax(-1)
    A = torch.zeros((n, k), dtype=dtype).index_add_(0, pos, p.sum(0)) / count
    loss = (A * A.clamp(min=CLAMP).log()).sum() / n
    U = g_loss / (n * count) * (A.clamp(min=CLAMP).log() + (A >= CLAMP).to(dtype))
    Ur = U[pos]  # [M, K]
    delta = (p * Ur).sum(-1)
    w = -temperature * p * (Ur - delta[..., None])
    if metric_dot:
        gx = w @ l
    else:
        r = torch.where(s == 0, torch.zeros_like(w), w / s)
        gx = x * r.sum(-1, keepdim=True) - r @ l
    return dict(loss=loss, A=A, U=U, delta=delta, gx=gx, lse=z.logsumexp(-1))


def clamp_margin(A):
    """Smallest |A / 1e-5 - 1| over the entries: how far the discontinuous mask [A >= 1e-5] is from flipping."""
    return float((A.double() / CLAMP - 1).abs().min())
