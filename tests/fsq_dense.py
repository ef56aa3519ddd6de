"""fp64 restatement of the FSQ / residual FSQ chain and its straight-through gradient, and a numpy fp32 restatement of
the index expression (what the kernel computes: per-dim terms ((c * hw) + hw) * basis, summed in the order torch's CPU
sum uses for a row of d <= 7 values, truncated to int32).

    chain64(x, levels, scales, prebound)   x [..., d] fp64 torch (autograd through round_ste) -> (out, margin)
    restate(kind, kwargs, sd, x, r, stages)  -> dict(out, grad): the module's forward in fp64, dL/dx of (out * r).sum()
    indices_np(codes, levels)             codes [..., d] fp32 numpy -> int32 indices (fp32 arithmetic, torch's order)
    torch_sum_order_np(t)                 t [..., d] fp32 -> the fp32 sum in that order
    levels_for(d), sweep_input(rows, width, seed, scale), whole_terms(codes, levels), exact_indices(codes, levels)
                                          the levels and inputs of the every-d sweeps, their order-free rows and the
                                          integer index
"""
from __future__ import annotations

import numpy as np
import torch

EPS = 1e-3


def consts64(levels, device=None):
    L = torch.tensor(levels, dtype=torch.float64, device=device)
    half_l = (L - 1) * (1 + EPS) / 2
    offset = torch.where(torch.tensor(levels, device=device) % 2 == 0, 0.5, 0.0).to(torch.float64)
    shift = torch.atanh(offset / half_l)
    hw = torch.tensor([v // 2 for v in levels], dtype=torch.float64, device=device)
    return half_l, offset, shift, hw


def bound64(z, levels):
    half_l, offset, shift, _ = consts64(levels, z.device)
    return torch.tanh(z + shift) * half_l - offset


def chain64(x, levels, scales=None, prebound=False):
    """x [..., d] fp64 -> (out: the sum over stages of code * scale, margin: the smallest distance of any stage's bound
    value from a rounding boundary (k + 0.5), per element of x's leading dims)."""
    _, _, _, hw = consts64(levels, x.device)
    if scales is None:
        scales = torch.ones((1, len(levels)), dtype=torch.float64, device=x.device)
    r = bound64(x, levels) if prebound else x
    out = torch.zeros_like(x)
    margin = torch.full(x.shape[:-1], np.inf, dtype=torch.float64, device=x.device)
    for s in range(scales.shape[0]):
        b = bound64(r / scales[s], levels)
        frac = (b - torch.floor(b)).detach()
        m = (frac - 0.5).abs()
        m = torch.where(torch.isfinite(m), m, torch.full_like(m, np.inf))
        margin = torch.minimum(margin, m.min(dim=-1).values)
        q = b + (torch.round(b) - b).detach()
        o = q / hw * scales[s]
        r = r - o.detach()
        out = out + o
    return out, margin


def _fsq_forward64(kw, sd, x, scales=None, prebound=False):
    """FSQ.forward (or one ResidualFSQ's chain when scales is given) in fp64 on x (channel-last, [b, ..., dim])."""
    levels = kw["levels"]
    d = len(levels)
    c = kw.get("num_codebooks", 1)
    lead = x.shape[:-1]
    xf = x.reshape(-1, x.shape[-1])
    if "project_in.weight" in sd:
        xf = xf @ sd["project_in.weight"].double().T
        if "project_in.bias" in sd:
            xf = xf + sd["project_in.bias"].double()
    xf = xf.reshape(-1, c, d)
    out, margin = chain64(xf, levels, scales, prebound)
    out = out.reshape(-1, c * d)
    if "project_out.weight" in sd:
        out = out @ sd["project_out.weight"].double().T
        if "project_out.bias" in sd:
            out = out + sd["project_out.bias"].double()
    return out.reshape(*lead, out.shape[-1]), margin.reshape(*lead, c).min(dim=-1).values


def forward64(kind, kw, sd, x, stages=None):
    """The module's forward in fp64 on x (any float dtype; its layout as the module takes it) -> (out, margin per row)."""
    x = x.double()
    if kind == "fsq":
        cf = kw.get("channel_first", False)
        xc = x.movedim(1, -1) if cf else x
        out, margin = _fsq_forward64(kw, sd, xc)
        return (out.movedim(-1, 1) if cf else out), margin
    levels = kw["levels"]
    Q = kw["num_quantizers"]
    S = Q if stages is None else stages
    scales = torch.stack([(torch.tensor(levels, dtype=torch.float32) - 1) ** -q for q in range(Q)]).double()[:S].to(x.device)
    if kind == "rfsq":
        return _fsq_forward64(dict(levels=levels), sd, x, scales, prebound=True)
    G = kw["groups"]
    outs, margins = [], []
    for g, chunk in enumerate(x.chunk(G, dim=-1)):
        sdg = {k[len(f"rvqs.{g}."):]: t for k, t in sd.items() if k.startswith(f"rvqs.{g}.")}
        o, m = _fsq_forward64(dict(levels=levels), sdg, chunk, scales, prebound=True)
        outs.append(o)
        margins.append(m)
    return torch.cat(outs, dim=-1), torch.stack(margins).min(dim=0).values


def restate(kind, kw, sd, x, r, stages=None):
    """-> dict(out, grad): fp64 out and dL/dx of (out * r).sum() (straight-through rounding)."""
    x64 = x.detach().double().requires_grad_(True)
    sd64 = {k: t.detach().double() for k, t in sd.items()}
    out, _ = forward64(kind, kw, sd64, x64, stages)
    (out * r.double()).sum().backward()
    return dict(out=out.detach(), grad=x64.grad)


def torch_sum_order_np(t):
    """fp32 sum over the last axis in torch's CPU order for d <= 7: partial k starts at term k (k < 4), terms 4 .. d-1 go
    into partial 0, then p0 += p1, p0 += p2, p0 += p3."""
    t = np.asarray(t, dtype=np.float32)
    d = t.shape[-1]
    s = t[..., 0].copy()
    for i in range(4, d):
        s = (s + t[..., i]).astype(np.float32)
    for i in range(1, min(d, 4)):
        s = (s + t[..., i]).astype(np.float32)
    return s


def indices_np(codes, levels):
    """codes [..., d] fp32 (the quantized codes c = round(bound) / hw) -> int32 indices as the kernel computes them."""
    codes = np.asarray(codes, dtype=np.float32)
    hw = np.array([v // 2 for v in levels], dtype=np.float32)
    basis = np.cumprod([1] + list(levels[:-1])).astype(np.int32).astype(np.float32)
    with np.errstate(invalid="ignore"):
        terms = (((codes * hw).astype(np.float32) + hw).astype(np.float32) * basis).astype(np.float32)
        s = torch_sum_order_np(terms)
        ok = (s >= -2147483648.0) & (s < 2147483648.0)
        out = np.where(ok, np.trunc(np.where(ok, s, 0)), -2147483648).astype(np.int64)
    return out.astype(np.int32)


def levels_for(d):
    """The levels of the every-d sweeps (tests/test_gpu_fsq_dims.py and its host self-check), d = 1 .. 16: every level is
    at most 25, where fl(fl(k / hw) * hw) == k for every code k, so every index term is a whole number; the codebook stays
    at most 2^24 (504 000 up to d = 7, 60 * 2^(d - 3) above), so the terms sum exactly in any order."""
    assert 1 <= d <= 16
    if d <= 7:
        return [8, 5, 7, 6, 25, 3, 4][:d]
    levels = [2] * d
    levels[0], levels[d // 2], levels[d - 1] = 5, 4, 3
    return levels


def sweep_input(rows, width, seed, scale=2.0):
    """randn * scale, fp32 [rows, width], the same values on every machine (torch's CPU generator)."""
    return (torch.randn(rows, width, generator=torch.Generator().manual_seed(seed)) * scale).numpy()


def terms_np(codes, levels):
    codes = np.asarray(codes, dtype=np.float32)
    hw = np.array([v // 2 for v in levels], dtype=np.float32)
    basis = np.cumprod([1] + list(levels[:-1])).astype(np.int64).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (((codes * hw).astype(np.float32) + hw).astype(np.float32) * basis).astype(np.float32)


def whole_terms(codes, levels):
    """Rows whose every index term is a whole number while the codebook holds at most 2^24 codes: their fp32 sum is exact
    in any order."""
    t = terms_np(codes, levels)
    with np.errstate(invalid="ignore"):
        whole = np.isfinite(t) & (t == np.trunc(t))
    return whole.all(axis=-1) & (int(np.prod(np.array(levels, dtype=np.int64))) <= 2**24)


def exact_indices(k, levels):
    """k [..., d] integer codes in [-hw, L - 1 - hw] -> sum_i (k_i + hw_i) * basis_i in int64."""
    hw = np.array([v // 2 for v in levels], dtype=np.int64)
    basis = np.cumprod([1] + list(levels[:-1])).astype(np.int64)
    return ((np.asarray(k, dtype=np.int64) + hw) * basis).sum(axis=-1)
