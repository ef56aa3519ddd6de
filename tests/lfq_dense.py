"""Dense fp64 torch restatement of the LFQ entropy aux loss (test helper; imports neither oracle/ nor the reference).

The softmax over the 2^d codes {-a, +a}^d is built explicitly, a chunk of rows at a time, exactly as the reference writes it:
logits 2 tau a sum_i v_i (2 b_{k,i} - 1), entropy -sum p log(max(p, 1e-5)), avg_prob the mean over the selected rows.
Everything is allocated on v's device, so GPU tests run the restatement on the GPU in fp64.
"""
from __future__ import annotations

import torch

EPS = 1e-5


def _entropy(p):
    return (-p * p.clamp(min=EPS).log()).sum(dim=-1)


def code_signs(d: int, device) -> torch.Tensor:
    """[2^d, d] of -1 / +1, dim 0 the most significant bit of the code index."""
    k = torch.arange(1 << d, device=device)
    bits = (k[:, None] >> torch.arange(d - 1, -1, -1, device=device)) & 1
    return (2 * bits - 1).to(torch.float64)


def dense_entropy(v: torch.Tensor, rows: torch.Tensor | None, code_scale: float, inv_temperature: float,
                  g_ps: float = 1.0, g_cb: float = 1.0, max_elems: int = 1 << 24):
    """v [N, C, d] -> dict(per_sample, codebook, avg_prob [C, 2^d], grad [N, C, d]), all fp64, where grad is
    d/dv (g_ps * per_sample + g_cb * codebook) (zero on rows not selected)."""
    N, C, d = v.shape
    P = 1 << d
    dev = v.device
    sel = torch.arange(N, device=dev) if rows is None else rows.to(dev)
    vs = v.detach().to(torch.float64)[sel]
    R = vs.shape[0]
    codes = code_signs(d, dev) * code_scale
    chunk = max(1, max_elems // (C * P))

    def probs(vc):
        return torch.softmax(2.0 * inv_temperature * torch.einsum("rcd,pd->rcp", vc, codes), dim=-1)

    ps_sum = torch.zeros((), dtype=torch.float64, device=dev)
    avg = torch.zeros((C, P), dtype=torch.float64, device=dev)
    with torch.no_grad():
        for r0 in range(0, R, chunk):
            p = probs(vs[r0:r0 + chunk])
            ps_sum += _entropy(p).sum()
            avg += p.sum(dim=0)
    avg /= R
    per_sample = ps_sum / (R * C)
    avg_ = avg.clone().requires_grad_(True)
    codebook = _entropy(avg_).mean()
    (g_avg,) = torch.autograd.grad(codebook, avg_)
    grad_sel = torch.zeros_like(vs)
    for r0 in range(0, R, chunk):
        vc = vs[r0:r0 + chunk].clone().requires_grad_(True)
        p = probs(vc)
        loss = g_ps * _entropy(p).sum() / (R * C) + g_cb * (g_avg * p).sum() / R
        (g,) = torch.autograd.grad(loss, vc)
        grad_sel[r0:r0 + chunk] = g
    grad = torch.zeros((N, C, d), dtype=torch.float64, device=dev)
    grad[sel] = grad_sel
    return dict(per_sample=per_sample.detach(), codebook=codebook.detach(), avg_prob=avg, grad=grad)


def dense_entropy_weighted(v: torch.Tensor, rows: torch.Tensor | None, code_scale: float, inv_temperature: float,
                           w_ps: float, w_cb: torch.Tensor, max_elems: int = 1 << 24) -> torch.Tensor:
    """fp64 d/dv of w_ps * sum_rows sum_c H(p_row,c) + sum_rows sum_c sum_k w_cb[c, k] p_row,c,k over the selected rows of
    v [N, C, d] (zero on the others): the (w_ps, w_cb) interface of native.lfq_entropy_backward, so each term can be driven
    on its own and w_cb chosen freely."""
    N, C, d = v.shape
    P = 1 << d
    dev = v.device
    sel = torch.arange(N, device=dev) if rows is None else rows.to(dev)
    vs = v.detach().to(torch.float64)[sel]
    R = vs.shape[0]
    codes = code_signs(d, dev) * code_scale
    wc = w_cb.detach().to(device=dev, dtype=torch.float64).reshape(C, P)
    chunk = max(1, max_elems // (C * P))
    grad_sel = torch.zeros_like(vs)
    for r0 in range(0, R, chunk):
        vc = vs[r0:r0 + chunk].clone().requires_grad_(True)
        p = torch.softmax(2.0 * inv_temperature * torch.einsum("rcd,pd->rcp", vc, codes), dim=-1)
        loss = float(w_ps) * _entropy(p).sum() + (wc * p).sum()
        (g,) = torch.autograd.grad(loss, vc)
        grad_sel[r0:r0 + chunk] = g
    grad = torch.zeros((N, C, d), dtype=torch.float64, device=dev)
    grad[sel] = grad_sel
    return grad
