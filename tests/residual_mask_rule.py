"""A numpy statement of the mask pass of a residual stack (include/vq_mi355x.h, vq_residual_mask_f32 and its backward): what
ResidualVQ / GroupedResidualVQ compute with ``mask=``, given the indices a search wrote for every row.  A plain module: it
holds no test.

Per row, with r_0 = x and acc = +0.0, for q = 0 .. Q-1, every operation one fp32 operation in this order:

    kept row:        c = cb_q[idx_q];  e_q += sum_d (c - r_q)^2;  quant = train ? r_q + (c - r_q) : c
    masked-out row:  quant = r_q       (idx_q is still the search result for r_q)
    both:            acc = acc + quant;  r_{q+1} = r_q - quant;   out = acc after the last stage

idx of stage q >= 1 on a masked-out row is the answer of stage q's codebook to r_q: zero_idx[q] for a row that is finite in
every element (r_q = 0), 0 for a row holding a non-finite element (r_1 has a NaN there; a row holding a NaN answers code 0).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def nearest(rows, cb):
    """The reference's search on fp64 distances for rows [M, D] against cb [K, D]: argmax of -cdist, first index on ties, a row
    holding a NaN answers 0.  (Only used where the winner is clear or exact: the all-zero row, seeded class-S rows.)"""
    rows, cb = np.asarray(rows, dtype=np.float64), np.asarray(cb, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = ((rows[:, None, :] - cb[None, :, :]) ** 2).sum(-1)
    idx = np.argmin(np.where(np.isnan(d2), -np.inf, d2), axis=1)  # NaN is argmax's maximum: the first NaN wins
    return idx.astype(np.int64)


def zero_indices(cbs, Q):
    """cbs [Qc, K, D] -> [Q]: every stage's answer to the all-zero row."""
    cbs = np.asarray(cbs)
    z = np.array([nearest(np.zeros((1, cbs.shape[-1])), cbs[q])[0] for q in range(cbs.shape[0])], dtype=np.int64)
    return np.broadcast_to(z, (Q,)).copy() if cbs.shape[0] == 1 else z


def forward(x, cbs, idx, mask, zero_idx, *, train):
    """x [M, D] fp32, cbs [Q | 1, K, D] fp32, idx [M, Q] int64 (the search's results: stage 0 of every row and every stage of
    a kept row are read), mask [M] bool, zero_idx [Q] -> dict(out [M, D] fp32, idx [M, Q] as the pass leaves it,
    sq_err [Q] fp64 sums of the fp32 squares over the kept rows, terms: what the backward needs)."""
    x = np.ascontiguousarray(x, dtype=F32)
    cbs = np.asarray(cbs, dtype=F32)
    idx = np.array(idx, dtype=np.int64)
    mask = np.asarray(mask, dtype=bool)
    M, D = x.shape
    Q = idx.shape[1]
    finite = np.isfinite(x).all(axis=1)
    r = x.copy()
    acc = np.zeros_like(x)
    sq_err = np.zeros(Q, dtype=np.float64)
    residuals, codes = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            if q >= 1:
                idx[~mask, q] = np.where(finite[~mask], zero_idx[q], 0)
            c = cbs[q if cbs.shape[0] > 1 else 0][idx[:, q]]
            residuals.append(r.copy())
            codes.append(c)
            diff = (c - r).astype(F32)
            hit = (r + diff).astype(F32) if train else c
            quant = np.where(mask[:, None], hit, r).astype(F32)
            sq = (diff * diff).astype(F32)
            sq_err[q] = sq[mask].astype(np.float64).sum()
            acc = (acc + quant).astype(F32)
            r = (r - quant).astype(F32)
    return dict(out=acc, idx=idx, sq_err=sq_err, residuals=residuals, codes=codes)


def search_chain(x, cbs, mask, *, train, stage0=None):
    """The whole reference loop without a search kernel: every stage's index is ``nearest`` of the residual the rule gives.
    -> the dict of ``forward`` (its idx is the reference's).  For seeded class-S inputs, whose winners are clear.
    ``stage0`` [M]: entries >= 0 replace the stage-0 index (a row holding an inf: which code ATen's cdist answers there is the
    search's business, pinned by the non-finite goldens, not this rule's)."""
    x = np.ascontiguousarray(x, dtype=F32)
    cbs = np.asarray(cbs, dtype=F32)
    mask = np.asarray(mask, dtype=bool)
    M, D = x.shape
    Q = cbs.shape[0]  # (a shared codebook is given expanded to its stages)
    idx = np.zeros((M, Q), dtype=np.int64)
    r = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            idx[:, q] = nearest(r, cbs[q])
            if q == 0 and stage0 is not None:
                idx[:, 0] = np.where(np.asarray(stage0) >= 0, stage0, idx[:, 0])
            c = cbs[q][idx[:, q]]
            hit = (r + (c - r).astype(F32)).astype(F32) if train else c
            quant = np.where(mask[:, None], hit, r).astype(F32)
            r = (r - quant).astype(F32)
    return forward(x, cbs, idx, mask, zero_indices(cbs, Q), train=train)


def backward(fwd, mask, grad_out, grad_sq_err, *, train):
    """fp64 gradient of the rule: grad_x = (train ? Q * grad_out : 0) + (mask ? sum_q 2 * grad_sq_err[q] * (r_q - c_q) : 0),
    with r_q, c_q the fp32 chain of ``fwd``.  -> (grad_x [M, D] fp64, S [M, D]: the sum of the absolute terms, for a bound)."""
    mask = np.asarray(mask, dtype=bool)
    Q = len(fwd["residuals"])
    M, D = fwd["out"].shape
    g = np.zeros((M, D), dtype=np.float64)
    S = np.zeros((M, D), dtype=np.float64)
    if train and grad_out is not None:
        g += Q * np.asarray(grad_out, dtype=np.float64)
        S += np.abs(g)
    if grad_sq_err is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            for q in range(Q):
                coef = 2.0 * float(grad_sq_err[q])
                t = coef * (fwd["residuals"][q].astype(np.float64) - fwd["codes"][q].astype(np.float64))
                t = np.where(mask[:, None], t, 0.0)
                g += t
                S += np.abs(t)
    return g, S
