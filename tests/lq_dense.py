"""Restatement of LatentQuantize: a numpy fp32 model of one sub-row written operation by operation (what the kernel
computes), and an fp64 forward / loss / gradient.

    default_tables(levels)               the reference's initial value tables (fp32 numpy, one array per dimension)
    quantize_np(z, tables)               z [..., d] fp32 -> (c, j): the straight-through values c_i = z_i + (q_i - z_i) and the
                                         selected positions (linear scan, strict <, a NaN distance beats any non-NaN best, the
                                         first NaN stays)
    terms_np(c, levels)                  t_i = ((c_i * 2) * hw_i + hw_i) * basis_i in fp32
    indices_np(c, levels)                (int32) of the terms' sum in torch's CPU order for d <= 7 (fsq_dense), truncated;
                                         NaN or out of range -> INT32_MIN
    order_free(c, levels)                rows whose every term is an integer while the codebook size is at most 2^24: the sum
                                         is exact in any order
    smallest_gap(z, tables)              per sub-row, the smallest difference between the two smallest distances of any dim
    restate64(kwargs, sd, x, r, train)   the module's forward in fp64 -> dict(out, loss, grad of (out * r).sum() + loss)
    levels_for(d), learned_tables(levels, seed), sweep_input(rows, width, seed)
                                         the levels, trained-looking tables and inputs of the every-d sweeps
    nearest64(z, tables)                 the fp64 nearest table value per element
"""
from __future__ import annotations

import numpy as np
import torch

from fsq_dense import sweep_input as fsq_sweep_input, torch_sum_order_np


def levels_of(kwargs):
    levels = kwargs["levels"]
    return [levels] * kwargs["codebook_dim"] if isinstance(levels, int) else list(levels)


def default_tables(levels):
    return [torch.linspace(-0.5, 0.5, L).numpy() if L % 2 == 1 else (torch.arange(L) / L - 0.5).numpy() for L in levels]


def quantize_np(z, tables):
    z = np.asarray(z, dtype=np.float32)
    c = np.empty_like(z)
    sel = np.zeros(z.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i, tab in enumerate(tables):
            tab = np.asarray(tab, dtype=np.float32)
            zi = z[..., i]
            q = np.full(zi.shape, tab[0], dtype=np.float32)
            best = np.abs((zi - q).astype(np.float32))
            for j in range(1, len(tab)):
                dist = np.abs((zi - tab[j]).astype(np.float32))
                take = (dist < best) | (np.isnan(dist) & ~np.isnan(best))
                best = np.where(take, dist, best)
                q = np.where(take, tab[j], q).astype(np.float32)
                sel[..., i] = np.where(take, j, sel[..., i])
            c[..., i] = (zi + (q - zi).astype(np.float32)).astype(np.float32)
    return c, sel


def terms_np(c, levels):
    c = np.asarray(c, dtype=np.float32)
    hw = np.array([v // 2 for v in levels], dtype=np.float32)
    basis = np.cumprod([1] + list(levels[:-1])).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (c * np.float32(2)).astype(np.float32)
        t = ((t * hw).astype(np.float32) + hw).astype(np.float32)
        return (t * basis).astype(np.float32)


def indices_np(c, levels):
    with np.errstate(invalid="ignore", over="ignore"):
        s = torch_sum_order_np(terms_np(c, levels))
        ok = (s >= -2147483648.0) & (s < 2147483648.0)
        out = np.where(ok, np.trunc(np.where(ok, s, 0)), -2147483648).astype(np.int64)
    return out.astype(np.int32)


def order_free(c, levels):
    t = terms_np(c, levels)
    with np.errstate(invalid="ignore"):
        whole = np.isfinite(t) & (t == np.trunc(t))
    return whole.all(axis=-1) & (int(np.prod(np.array(levels, dtype=np.int64))) <= 2**24)


def smallest_gap(z, tables):
    z = np.asarray(z, dtype=np.float64)
    gap = np.full(z.shape[:-1], np.inf)
    for i, tab in enumerate(tables):
        if len(tab) < 2:
            continue
        with np.errstate(invalid="ignore"):
            dist = np.sort(np.abs(z[..., i, None] - np.asarray(tab, dtype=np.float64)), axis=-1)
            gap = np.minimum(gap, dist[..., 1] - dist[..., 0])
    return gap


def levels_for(d):
    """The levels of the every-d sweeps (tests/test_gpu_lq_dims.py and its host self-check), d = 1 .. 16.  d <= 7: levels 6
    and 7 are in, so that terms that are not whole numbers meet the pinned torch order.  d >= 8: only levels whose default
    tables are dyadic (2, 3, 4, 5, 8), so that z + (q - z) is q, every term a whole number and the sum exact in any order;
    the codebook stays at 480 * 2^(d - 4) <= 2^21 entries."""
    assert 1 <= d <= 16
    if d <= 7:
        return [5, 8, 3, 6, 7, 4, 2][:d]
    levels = [2] * d
    levels[0], levels[3], levels[d // 2], levels[d - 1] = 5, 8, 4, 3
    return levels


def learned_tables(levels, seed):
    """Tables as training leaves them: the default values + 0.01 * randn, shuffled, one value of each table duplicated."""
    rng = np.random.default_rng(seed)
    out = []
    for tab in default_tables(levels):
        t = (tab + np.float32(0.01) * rng.standard_normal(len(tab)).astype(np.float32)).astype(np.float32)
        rng.shuffle(t)
        a, b = rng.choice(len(t), 2, replace=False)
        t[b] = t[a]
        out.append(t)
    return out


def sweep_input(rows, width, seed):
    """randn * 0.5, fp32 [rows, width], the same values on every machine (torch's CPU generator)."""
    return fsq_sweep_input(rows, width, seed, 0.5)


def nearest64(z, tables):
    """The table value nearest to every z[..., i] in fp64 (the first one on an exact tie)."""
    z = np.asarray(z, dtype=np.float64)
    q = np.empty_like(z)
    for i, tab in enumerate(tables):
        t = np.asarray(tab, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            q[..., i] = t[np.argmin(np.abs(z[..., i, None] - t), axis=-1)]
    return q


def restate64(kwargs, sd, x, r, train, tables=None):
    """x [b, dim, ...] -> fp64 out, loss (with the fp32 weights' values) and dL/dx of (out * r).sum() + loss.  tables: the
    value tables when they are not in sd (optimize_values=False)."""
    levels = levels_of(kwargs)
    d = len(levels)
    C = kwargs.get("num_codebooks", 1)
    if tables is None:
        tables = [sd[f"values_per_latent.{i}"] for i in range(d)] if "values_per_latent.0" in sd else default_tables(levels)
    tables = [torch.as_tensor(np.asarray(t)).double() for t in tables]
    w_c = float(np.float32(kwargs.get("commitment_loss_weight", 0.1)))
    w_q = float(np.float32(kwargs.get("quantization_loss_weight", 0.1)))
    x64 = torch.as_tensor(x).detach().double().requires_grad_(True)
    b = x64.shape[0]
    z = x64.movedim(1, -1)
    lead = z.shape[1:-1]
    z = z.reshape(b, -1, z.shape[-1])
    if "project_in.weight" in sd:
        z = z @ torch.as_tensor(sd["project_in.weight"]).double().T + torch.as_tensor(sd["project_in.bias"]).double()
    z = z.reshape(b, z.shape[1], C, d)
    q = torch.stack([tables[i][torch.argmin((z[..., i, None] - tables[i]).abs(), dim=-1)] for i in range(d)], dim=-1)
    codes = (z + (q - z).detach()).reshape(b, -1, C * d)
    out = codes
    if "project_out.weight" in sd:
        out = out @ torch.as_tensor(sd["project_out.weight"]).double().T + torch.as_tensor(sd["project_out.bias"]).double()
    out = out.reshape(b, *lead, out.shape[-1]).movedim(-1, 1)
    loss = torch.zeros((), dtype=torch.float64)
    if train:
        mse_c = ((x64.detach() - out) ** 2).mean() if w_c != 0 else 0.0
        mse_q = ((out.detach() - x64) ** 2).mean() if w_q != 0 else 0.0
        loss = w_c * mse_c + w_q * mse_q + loss
    ((out * torch.as_tensor(r).double()).sum() + loss).backward()
    return dict(out=out.detach(), loss=loss.detach(), grad=x64.grad)
