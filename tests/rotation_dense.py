"""Plain numpy model of the rotation trick's backward (csrc/vq_rotate.inc, vq_rotate_backward_kernel), its error bound and
the inputs the tests feed it (test helper; CPU only, imports neither oracle/ nor the reference).

The formula (Fifty et al., arXiv 2410.06424, section 4.2; include/vq_mi355x.h states it).  Per stage, r the residual the stage
quantized, c its code, g the incoming gradient of the output, eps = 1e-6:

    a = max(|r|, eps)   b = max(|c|, eps)   u = r / a   qh = c / b   s = u + qh   w = s / max(|s|, eps)   lam = |c| / a
    grad_x = sum_q lam (g - 2 (g.w) w + 2 (g.qh) u)  +  sum_q 2 ge[q] (r_q - c_q)

which the kernel evaluates as sum_q (t0 - t1 + t2 + L) with

    t0 = lam g     t1 = alpha s,  alpha = 2 lam (g.s) / n2,  n2 = max(|s|, eps)^2     t2 = beta r,  beta = 2 lam (g.c) / (a b)
    L = coef (r - c),  coef = 2 ge[q].

The residual chain is train_dense.residual_chain: elementwise IEEE add / sub, the device's chain bit for bit.  Everything after
the chain is evaluated here in fp64 from those fp32 values.

Error bound.  u = 2^-24; every rounding of the kernel's fp32 arithmetic is counted, the first-order propagation is written
out, and the total is doubled.  Nothing is fitted to a measurement, and nothing is assumed about the conditioning of the row:
where a quantity is ill-conditioned (s close to 0: c close to -r) the bound grows with the data instead of being assumed away.

  dot products.  A lane adds at most steps = 4 ceil(D / 256) products (the vector variant holds 4 per slot, the scalar one
    ceil(D / 64) <= steps; slots beyond D hold zeros, and adding 0 is exact), then 6 butterfly steps add the lanes: every
    product passes through at most T = steps + 6 additions (fused into the product in the lane, which only removes its
    rounding), so a computed sum of products p_i is off by at most (T + 1) u sum |p_i| (1 + O(u)) -- relative to the sum of
    ABSOLUTE products, not to its value.
  one-instruction square root and reciprocal (v_sqrt_f32, v_rcp_f32): 1 ulp each, that is 2u.
  norms.  |r|^2 and |c|^2 are sums of non-negative terms: relative error (T + 1) u; the square root halves it and adds 2u:
    e_a = ((T + 1) / 2 + 2) u for a, b and |c| (max(., eps) is 1-Lipschitz and exact).  1 / a, 1 / b: e_i = e_a + 2u.
    lam = |c| * (1 / a): e_lam = e_a + e_i + u = (T + 8) u.
  s.  s_d = r_d (1 / a) + c_d (1 / b): each product carries e_i + u, the sum rounds once on |s_d| <= m_d = |r_d| / a + |c_d| / b:
        ds_d = (e_i + 2u) m_d = ((T + 1) / 2 + 6) u m_d           (absolute: s_d itself may be 0).
  g.s and |s|^2 (second reduction, from the rounded s).
        E_gs = (T + 1) u sum |g_d| |s_d| + sum |g_d| ds_d
        E_ss = (T + 1) u |s|^2 + 2 sum |s_d| ds_d
    n2 = max(ss, eps^2) = max(|s|, eps)^2, exact and 1-Lipschitz: |n2' - n2| <= E_ss =: rho n2.  For rho < 1 the reciprocal
    of the denominator is off by rho' = rho / (1 - rho) relative, and by 2u more for the instruction.
  alpha = ((2 lam) * gs) * (1 / n2): lam's error, two products, one reciprocal:
        d_alpha = (2 lam / n2) (E_gs (1 + rho') + |g.s| (rho' + (e_lam + 4u) (1 + rho')))
    t1_d = alpha s_d:   e1_d = d_alpha (|s_d| + ds_d) + |alpha| ds_d + u |t1_d|.
    Whatever the rounding did, |t1| <= 2 lam |g| both exactly and as computed (Cauchy-Schwarz: |(g.s) s_d| <= |g| |s|^2), so
    e1_d <= 4.01 lam |g|_2 always: that cap replaces the first-order expression where it is larger (and where rho >= 1).
  beta = ((2 lam) * gc) * (1 / a) * (1 / b): E_gc = (T + 1) u sum |g_d| |c_d|, three products, two reciprocals:
        d_beta = (2 lam / (a b)) (E_gc + |g.c| (e_lam + 3u + 2 e_i));      e2_d = d_beta |r_d| + u |t2_d|.
  t0_d = g_d lam: e0_d = (e_lam + u) |t0_d|.
  L_d: r - c, float(2 ge[q]) and their product, 3u |L_d| (as in train_dense's backward bound).
  accumulation.  Every stage adds t0, -t1, t2 and L into the accumulator, one fused multiply-add each: 4Q additions (the first
    one into 0, exact), each at most u times a partial sum of at most S = sum_q (|t0| + |t1| + |t2| + |L|):  4Q u S.  (The
    products inside those fused operations are not rounded; their u |t| terms above are kept, which only widens the bound.)

        tol = 2 ( sum_q (e0 + min(e1, cap) + e2 + 3u |L|) + 4Q u S ).
"""
from __future__ import annotations

import math

import numpy as np
import torch

import train_dense as td

U = td.U
F32 = np.float32
EPS = float(F32(1e-6))  # the kernel's 1e-6f


def _f64(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def _dot(a, b):
    return (a * b).sum(-1, keepdims=True)


def rotate_backward_model(x, cb, idx, go, ge, *, share, per_head, ste=True, chain_dtype=F32, eps=EPS, drop_u_term=False,
                          unit_lam=False):
    """-> (g, tol) fp64 [H, M, D]: the gradient and its elementwise error bound (module docstring).  go [H, M, D] or None,
    ge [Q] ([H, Q] with per_head) or None.  `drop_u_term` (no 2 (g.qh) u) and `unit_lam` (lam = 1) build deliberately wrong
    models (tests of the bound's bite)."""
    idx = td._idx(idx)
    H, M, Q = idx.shape
    stages = td.residual_chain(x, cb, idx, ste=ste, share=share, dtype=chain_dtype)
    D = stages[0][0].shape[-1]
    T = 4 * math.ceil(D / 256) + 6
    e_a = ((T + 1) / 2 + 2) * U
    e_i = e_a + 2 * U
    e_lam = e_a + e_i + U
    k_s = e_i + 2 * U
    g_out = np.zeros((H, M, D)) if go is None else _f64(go)
    if ge is not None:
        ge = _f64(ge)
        ge = ge.reshape(H, Q) if per_head else np.broadcast_to(ge.reshape(1, Q), (H, Q))
    grad = np.zeros((H, M, D))
    first = np.zeros((H, M, D))  # sum_q of the per-stage first-order terms
    S = np.zeros((H, M, D))
    gnorm = np.sqrt(_dot(g_out, g_out))
    for q, (r, c, _live) in enumerate(stages):
        r, c = r.astype(np.float64), c.astype(np.float64)
        nc = np.sqrt(_dot(c, c))
        a, b = np.maximum(np.sqrt(_dot(r, r)), eps), np.maximum(nc, eps)
        lam = np.ones_like(a) if unit_lam else nc / a
        s = r / a + c / b
        m = np.abs(r) / a + np.abs(c) / b
        ss = _dot(s, s)
        n2 = np.maximum(np.sqrt(ss), eps) ** 2
        gs, gc = _dot(g_out, s), _dot(g_out, c)
        alpha = 2.0 * lam * gs / n2
        beta = 2.0 * lam * gc / (a * b)
        t0, t1, t2 = lam * g_out, alpha * s, (0.0 if drop_u_term else 1.0) * beta * r
        loss = 0.0 * r if ge is None else 2.0 * ge[:, q][:, None, None] * (r - c)
        grad += t0 - t1 + t2 + loss
        # the bound
        ds = k_s * m
        E_gs = (T + 1) * U * _dot(np.abs(g_out), np.abs(s)) + _dot(np.abs(g_out), ds)
        E_ss = (T + 1) * U * ss + 2.0 * _dot(np.abs(s), ds)
        rho = E_ss / n2
        with np.errstate(divide="ignore", invalid="ignore"):
            rho1 = np.where(rho < 1.0, rho / (1.0 - rho), np.inf)
            d_alpha = 2.0 * lam / n2 * (E_gs * (1.0 + rho1) + np.abs(gs) * (rho1 + (e_lam + 4 * U) * (1.0 + rho1)))
            e1 = d_alpha * (np.abs(s) + ds) + np.abs(alpha) * ds + U * np.abs(t1)
        e1 = np.where(np.isfinite(e1), e1, np.inf)
        e1 = np.minimum(e1, 4.01 * lam * gnorm)
        E_gc = (T + 1) * U * _dot(np.abs(g_out), np.abs(c))
        d_beta = 2.0 * lam / (a * b) * (E_gc + np.abs(gc) * (e_lam + 3 * U + 2 * e_i))
        e2 = d_beta * np.abs(r) + U * np.abs(t2)
        e0 = (e_lam + U) * np.abs(t0)
        first += e0 + e1 + e2 + 3 * U * np.abs(loss)
        S += np.abs(t0) + np.abs(t1) + np.abs(t2) + np.abs(loss)
    return grad, 2.0 * (first + 4 * Q * U * S)


def literal_autograd(x, cb, idx, go, ge, *, share, per_head, eps=EPS):
    """torch fp64 autograd of the literal composition: every stage's output is rot(r_q) with u, qh, w, lam detached, every
    residual is x minus detached terms, sq_err_q = sum (c_q - r_q)^2.  -> (grad_x [H, M, D], the largest |rot(r_q) - c_q|
    relative to |c_q|'s largest entry over the rows with r_q != 0)."""
    idx = torch.as_tensor(td._idx(idx))
    H, M, Q = idx.shape
    xs = torch.as_tensor(_f64(x)).clone().requires_grad_(True)
    cbd = torch.as_tensor(_f64(cb))
    god = torch.as_tensor(_f64(go))
    harange = torch.arange(H)[:, None]
    gev = None
    if ge is not None:
        gev = torch.as_tensor(_f64(ge))
        gev = gev.reshape(H, Q) if per_head else gev.reshape(1, Q).expand(H, Q)
    r, out, loss, worst = xs, 0.0, 0.0, 0.0
    for q in range(Q):
        c = cbd[:, 0 if share else q][harange, idx[..., q]]
        rd = r.detach()
        a = rd.norm(dim=-1, keepdim=True).clamp(min=eps)
        b = c.norm(dim=-1, keepdim=True).clamp(min=eps)
        u, qh = rd / a, c / b
        s = u + qh
        w = s / s.norm(dim=-1, keepdim=True).clamp(min=eps)
        lam = c.norm(dim=-1, keepdim=True) / a
        rot = lam * (r - 2.0 * (r * w).sum(-1, keepdim=True) * w + 2.0 * (r * u).sum(-1, keepdim=True) * qh)
        moved = (rd != 0).any(-1)  # (r = 0 has no direction to rotate: u = 0 and rot(0) = 0, the one row whose value is not c)
        worst = max(worst, float(((rot.detach() - c).abs().amax(-1) / c.abs().amax(-1).clamp(min=1e-300))[moved].max()))
        if gev is not None:
            loss = loss + (gev[:, q] * ((c - r) ** 2).sum(dim=(1, 2))).sum()
        out = out + rot
        r = r - (rd + (c - rd))
    ((out * god).sum() + loss).backward()
    return xs.grad.numpy(), worst


def degenerate_inputs(H, M, D, Q, K, seed, *, per_head=False, share=False):
    """train_dense.backward_inputs with the exact and degenerate rows of the issue embedded in head H - 1 (M >= 8, K >= 4):
    row 1: c_0 = -r_0 (s = 0, w = 0);   row 2: c_0 = r_0 (the next stage's residual is exactly 0: u = 0 there);
    row 3: x = 0 (u = 0, lam = |c| 1e6);   row 4: its stage-0 code is all zero (lam = 0).   -> (x, cb, idx, go, ge, rows)."""
    assert M >= 8 and K >= 4
    x, cb, idx, go, ge = td.backward_inputs(H, M, D, Q, K, seed, per_head=per_head, share=share)
    h = H - 1
    idx[h, 1, 0], idx[h, 2, 0], idx[h, 4, 0] = 0, 1, 2
    idx[h, 3, 0] = 3
    x[h, 1] = -cb[h, 0, 0]
    x[h, 2] = cb[h, 0, 1]
    x[h, 3] = 0.0
    cb[h, 0, 2] = 0.0
    if share:  # one codebook for every stage: keep the later stages of the special rows off the edited codes' special roles
        idx[h, 1:5, 1:] = 3
    return x, cb, idx, go, ge, (1, 2, 3, 4)
