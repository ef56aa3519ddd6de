"""fp64 restatement of ResidualLFQ's losses and dL/dx (test helper; imports neither oracle/ nor the reference).

The residual chain itself runs in fp32, op for op as the reference writes it (soft clamp, l2norm, sign, straight-through
value, residual -= quantized), so every stage sees the reference's stage input.  Each stage's losses and gradient are then
restated in fp64: the entropy terms by tests/lfq_dense.py, the commitment term and the clamp / l2norm Jacobians by fp64
autograd.  Everything is allocated on x's device.  The residual's detach makes d r_q / d x the identity, so dL/dx is the
sum of the stages' terms.
"""
from __future__ import annotations

from math import log2

import torch
import torch.nn.functional as F

from lfq_dense import dense_entropy


def stage_params(kwargs: dict, q: int):
    """(codebook_scale, soft clamp value or None, code magnitude) of stage q."""
    scale = 2.0**-q
    c = kwargs.get("soft_clamp_input_value")
    clamp = None if c is None else c * 0.5**q
    d = int(log2(kwargs["codebook_size"]))
    mag = scale
    if kwargs.get("spherical", False):
        mag = float(F.normalize(torch.full((1, d), scale, dtype=torch.float32), dim=-1)[0, 0] * scale)
    return scale, clamp, mag


def stage_rows(N: int, mask, frac: float, stages: int):
    """The entropy rows of each stage, drawn from the global CPU generator in stage order (LFQ._entropy_rows)."""
    out = []
    for _ in range(stages):
        rows = None if mask is None else mask.reshape(-1).nonzero().squeeze(1)
        if frac < 1.0:
            num_tokens = N if rows is None else int(rows.numel())
            picked = (torch.randn(num_tokens).argsort(dim=-1) < int(num_tokens * frac)).nonzero().squeeze(1)
            rows = picked if rows is None else rows[picked]
        out.append(rows)
    return out


def _front(u64, scale, clamp, spherical):
    if clamp is not None:
        u64 = (u64 / clamp).tanh() * clamp
    if spherical:
        u64 = F.normalize(u64, dim=-1) * scale
    return u64


def restate(kwargs: dict, sd: dict, x: torch.Tensor, mask, g_out: torch.Tensor, stages: int, rows: list,
            g_loss: float = 1.0):
    """x [..., dim] fp32, g_out [..., dim] (upstream gradient of the module's output), stages = the active stage count,
    rows[q] the entropy rows of stage q.  Returns dict(grad fp64 like x, losses fp64 [stages], out fp32)."""
    d = int(log2(kwargs["codebook_size"]))
    ew = kwargs.get("entropy_loss_weight", 0.1)
    cw = kwargs.get("commitment_loss_weight", 0.25)
    gamma = kwargs.get("diversity_gamma", 1.0)
    softplus = kwargs.get("experimental_softplus_entropy_loss", False)
    offset = kwargs.get("entropy_loss_offset", 5.0)
    spherical = kwargs.get("spherical", False)
    proj = "project_in.weight" in sd
    x64 = x.detach().double().reshape(-1, x.shape[-1])
    g_out64 = g_out.detach().double().reshape(-1, x.shape[-1])
    if proj:
        xp = F.linear(x.detach().float().reshape(-1, x.shape[-1]), sd["project_in.weight"], sd["project_in.bias"])
        g_out64 = g_out64 @ sd["project_out.weight"].double()  # project_out's backward
    else:
        xp = x.detach().float().reshape(-1, d)
    N = xp.shape[0]
    m = None if mask is None else mask.reshape(-1)
    kept = N if m is None else int(m.sum())
    residual = xp.clone()
    out_sum = torch.zeros_like(xp)
    g_xp = torch.zeros(N, d, dtype=torch.float64, device=x.device)
    losses = []
    for q in range(stages):
        scale, clamp, mag = stage_params(kwargs, q)
        u = residual
        if clamp is not None:
            u = (u / clamp).tanh() * clamp
        v = F.normalize(u, dim=-1) * scale if spherical else u
        qv = torch.where(v > 0, mag, -mag)
        out = v + (qv - v)
        # fp64 stage terms
        r64 = residual.double().requires_grad_(True)
        v64 = _front(r64, scale, clamp, spherical)
        ent = dense_entropy(v64.detach().reshape(N, 1, d), rows[q], mag, 100.0)
        aux = ent["per_sample"] - gamma * ent["codebook"]
        dsp = 1.0
        if softplus:
            dsp = float(torch.sigmoid(aux + offset))
            aux = F.softplus(aux + offset)
        g_ent = dense_entropy(v64.detach().reshape(N, 1, d), rows[q], mag, 100.0, g_ps=g_loss * ew * dsp,
                              g_cb=-g_loss * ew * dsp * gamma)["grad"].reshape(N, d)
        loss = aux * ew
        gv = g_out64 + g_ent
        if cw > 0.0:
            e = v.double() - qv.double()
            if m is not None:
                e = e * m.reshape(-1, 1).double()
            loss = loss + cw * (e * e).sum() / (kept * d)
            gv = gv + g_loss * cw * 2.0 * e / (kept * d)
        (g_r,) = torch.autograd.grad(v64, r64, gv)
        g_xp += g_r
        losses.append(float(loss))
        residual = residual - out
        out_sum = out_sum + out
    grad = g_xp @ sd["project_in.weight"].double() if proj else g_xp
    return dict(grad=grad.reshape(x.shape), losses=torch.tensor(losses, dtype=torch.float64, device=x.device), out=out_sum)
