"""Straight-through and reinmax Gumbel relaxations of the code selection (reference: utils/general.py:112-151,
codebooks.py:386-397), without the ``[h, M, K]`` tensors the reference differentiates through.

The forward VALUE of the relaxed selection is the selected code (the reference's ``onehot + p - p.detach()`` contracted with
the codebook differs from the gather by fp32 rounding only); what the relaxation changes is the gradient.  With

    s = similarities [M, K]      g = dL/dquantize [M, D]      a = g c^T [M, K]      tau = 1 / temperature

the gradient with respect to the similarities is ``w``:

    straight-through   p = softmax_k(tau s)           delta_m = sum_k p_mk a_mk      w = tau p (a - delta)
    reinmax            p0 = softmax_k(s)              p1 = max((onehot + softmax_k(tau s)) / 2, 1e-5)
                       pi_mk = p1_mk / sum_m' p1_m'k  (the reference normalises over the ROWS of the head: ``.softmax(dim=1)``)
                       e_k = sum_m pi_mk a_mk         delta0_m = sum_k p0_mk a_mk
                       w = 2 pi (a - e) - 0.5 p0 (a - delta0)

and it reaches ``x`` and the codes through the similarity's own backward (``losses._SimilarityFn``).  A codebook that
requires grad also receives the ordinary gradient of the gather, ``scatter_add(ind, g)``.

Straight-through on fp32 rows of up to 256 dims is three native sweeps (``vq_gumbel_*``: row statistics, d/dx, d/dcodes),
none of which writes anything of ``[M, K]``.  Reinmax on the same rows is four (``vq_gumbel_reinmax_*``): row statistics
(both log-sum-exps and delta0), column statistics (``col_k = sum_m p1_mk`` and ``e_k``: the normalisation over the rows of
the head, summed per row split and added in split order), d/dx and d/dcodes; the selection ``ind`` is an input that the
kernels only compare with code indices.  Everything else -- wider rows, backends without the kernels, the live-codes quirk
of an EMA step between forward and backward -- runs on bounded row chunks of the similarity matrix, like the cross-entropy
backward (reinmax there: three chunked passes).
"""
from __future__ import annotations

import torch

from . import losses, search


def draw_seed(device) -> torch.Tensor:
    """The seed of one Gumbel-max sampling call (native.sample_codes): two int64 words drawn on ``device`` from its default
    generator, so ``torch.manual_seed`` governs the sampled codes; they stay on the device (no host synchronisation)."""
    return torch.randint(-(2 ** 63), 2 ** 63 - 1, (2,), dtype=torch.int64, device=device)


def _harange(t):
    return torch.arange(t.shape[0], device=t.device)[:, None]


def _chunked_backward(x, codes, live, ind, g, metric, tau, reinmax, need_x, need_c):
    """(gx, gc_sim) on bounded row chunks.  ``codes`` gave the similarities; ``live`` (or ``codes``) is what the reference's
    autograd multiplies with at backward time (losses.similarity_matrix: live_codes)."""
    h, m, _ = x.shape
    k = codes.shape[1]
    mult = (codes if live is None else live).detach()
    chunks = losses._row_slices(m, losses._rows_per_chunk(h, k))
    backend = search.get_backend()

    def sims_of(rows):
        return backend.similarities(x[:, rows], codes, metric=metric)

    col = e = None
    if reinmax:
        def p1_of(s, rows):
            p = (s * tau).softmax(dim=-1)
            p.scatter_add_(-1, ind[:, rows, None], torch.ones_like(p[..., :1]))
            return (p * 0.5).clamp_(min=1e-5)

        col = torch.zeros((h, k), dtype=torch.float32, device=x.device)
        for rows in chunks:
            col += p1_of(sims_of(rows), rows).sum(dim=1)
        e = torch.zeros_like(col)
        for rows in chunks:
            e += (p1_of(sims_of(rows), rows) / col[:, None] * (g[:, rows] @ mult.transpose(-1, -2))).sum(dim=1)

    def chunk_value(xc, cc, rows):
        sims = losses.similarity_matrix(xc, cc, metric, live)
        with torch.no_grad():
            s = sims.detach()
            a = g[:, rows] @ mult.transpose(-1, -2)
            if reinmax:
                pi = p1_of(s, rows) / col[:, None]
                p0 = s.softmax(dim=-1)
                w = 2.0 * pi * (a - e[:, None]) - 0.5 * p0 * (a - (p0 * a).sum(-1, keepdim=True))
            else:
                p = (s * tau).softmax(dim=-1)
                w = tau * p * (a - (p * a).sum(-1, keepdim=True))
        return (w * sims).sum()

    one = torch.ones((), dtype=torch.float32, device=x.device)
    return losses._chunk_grads(chunk_value, x, codes, chunks, one, need_x, need_c)


class _RelaxedGatherFn(torch.autograd.Function):
    """quantize = codes[ind], with the gradient of the relaxed one-hot selection (module docstring)."""

    @staticmethod
    def forward(ctx, x, codes, ind, metric, temperature, reinmax, live_codes=None):
        ctx.save_for_backward(x, codes, ind)
        ctx.metric, ctx.tau, ctx.reinmax, ctx.live = metric, 1.0 / temperature, reinmax, live_codes
        return codes.detach()[_harange(codes), ind]

    @staticmethod
    def backward(ctx, g):
        x, codes, ind = ctx.saved_tensors
        x, codes = x.detach(), codes.detach()
        need_x, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g.to(torch.float32)
        backend = search.get_backend()
        grads = None
        fused = getattr(backend, "reinmax_backward" if ctx.reinmax else "gumbel_backward", None)
        if fused is not None and ctx.live is None:  # (None: outside the kernels' range, D > 256)
            if ctx.reinmax:
                grads = fused(x, codes, g, ind, metric=ctx.metric, tau=ctx.tau, need_x=need_x, need_codes=need_c)
            else:
                grads = fused(x, codes, g, metric=ctx.metric, tau=ctx.tau, need_x=need_x, need_codes=need_c)
        if grads is None:
            grads = _chunked_backward(x, codes, ctx.live, ind, g, ctx.metric, ctx.tau, ctx.reinmax, need_x, need_c)
        gx, gc = grads
        if need_c:  # the gather's own gradient
            gc = gc + backend.ema_accumulate(g.contiguous(), ind.contiguous(), codes.shape[1])[1]
        return gx, gc, None, None, None, None, None


def relaxed_gather(x: torch.Tensor, codes: torch.Tensor, ind: torch.Tensor, metric: int, temperature: float,
                   reinmax: bool = False, live_codes=None) -> torch.Tensor:
    """x [H, M, D] (strided rows fine), codes [H, K, D], ind [H, M] int64 -> codes[ind] [H, M, D], differentiable with
    respect to ``x`` and ``codes`` as the reference's straight-through (or reinmax) Gumbel softmax at ``temperature``.
    ``live_codes``: see losses.similarity_matrix()."""
    return _RelaxedGatherFn.apply(x.float(), codes, ind, metric, float(temperature), bool(reinmax), live_codes)
