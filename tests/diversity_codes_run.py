"""Shared by the host and the GPU test of the diversity loss's gradient with respect to a learnable codebook
(vq_diversity_backward_codes_f32): the fp64 closed form of gc, built on the U and delta of diversity_run.closed_form64, and
the reference's own op sequence with autograd with respect to the codes (vector_quantize_pytorch.py:324-334 with
utils/general.py:25-30), both on the CPU.

    w_mk = -T p_mk (U[n(m)][k] - delta_m)
    dot     gc_k = sum_m w_mk x_m
    Euclid  r = w / s (0 where s == 0, s = -dist)     gc_k = c_k sum_m r_mk - sum_m r_mk x_m
The sums run over all rows of the head."""
from __future__ import annotations

import torch

from diversity_run import CLAMP, closed_form64, positions, similarities


def codes_gradient64(x, c, temperature, n, pos_div, metric_dot, g_loss=1.0, dtype=torch.float64):
    """-> dict(gc [H, K, D], and loss, A, U, delta, gx, lse of closed_form64) in ``dtype``, no autograd."""
    ref = closed_form64(x, c, temperature, n, pos_div, metric_dot, g_loss=g_loss, dtype=dtype)
    x, c = x.to(dtype), c.to(dtype)
    pos = positions(x.shape[1], n, pos_div)
    s = similarities(x, c, metric_dot)
    p = (-temperature * s).softmax(-1)
    w = -temperature * p * (ref["U"][pos] - ref["delta"][..., None])
    if metric_dot:
        gc = w.transpose(-1, -2) @ x
    else:
        r = torch.where(s == 0, torch.zeros_like(w), w / s)
        gc = c * r.sum(-2).unsqueeze(-1) - r.transpose(-1, -2) @ x
    return dict(ref, gc=gc)


def reference_sequence_codes(x, c, temperature, n, pos_div, metric_dot, dtype=torch.float32, g_loss=1.0):
    """The reference's op sequence in ``dtype`` with autograd with respect to the rows AND the codes
    -> dict(loss, A [N, K], gx [H, M, D], gc [H, K, D])."""
    x = x.to(dtype).clone().requires_grad_(True)
    c = c.to(dtype).clone().requires_grad_(True)
    h, m, _ = x.shape
    k = c.shape[1]
    z = -similarities(x, c, metric_dot) * temperature
    prob = z.softmax(dim=-1)
    avg = prob.reshape(h, m // (n * pos_div), n, pos_div, k).mean(dim=(0, 1, 3))
    ent = (-avg * avg.clamp(min=CLAMP).log()).sum(dim=-1)
    loss = -ent.mean()
    (loss * g_loss).backward()
    return dict(loss=loss.detach(), A=avg.detach(), gx=x.grad, gc=c.grad)
