"""What the three residual families share (``residual.py``, ``residual_lfq.py``, ``residual_fsq.py``): plain functions, no
base class.  The stacks differ in what a stage is -- a codebook search, sign bits, a rounding grid -- and in what they return;
they agree in everything around the stages, which the reference writes out once per file: the quantize-dropout draw, the
padding of the stages that did not run, the assertion on coarse indices, the layout of a grouped module's rows on the way in
and out, its loop over the groups when the fused path does not take the call, and the buffers of its fused decode.

A "stack" below is one of ``ResidualVQ`` / ``ResidualLFQ`` / ``ResidualFSQ`` (anything with ``num_quantizers``,
``quantize_dropout``, ``project_in`` and ``project_out``); "stacks" are a grouped module's ``rvqs``.
"""
from __future__ import annotations

import random
from math import ceil, prod

import torch


def dropout_cut(cutoff_index: int, num_quantizers: int, multiple_of: int, rng=None) -> int:
    """The last stage that runs under quantize dropout (residual_vq.py:194-207 of the reference, the same lines in its
    residual_lfq.py and residual_fsq.py): one ``randrange`` from ``rng`` -- a generator, a seed for a fresh ``random.Random``,
    or None for the process-wide one -- rounded up to a whole multiple of stages."""
    if rng is None:
        rng = random
    elif not hasattr(rng, "randrange"):
        rng = random.Random(rng)
    cut = rng.randrange(cutoff_index, num_quantizers)
    if multiple_of != 1:
        cut = ceil((cut + 1) / multiple_of) * multiple_of - 1
    return cut


def check_coarse(stack, stages_given: int) -> None:
    """Indices of fewer stages than the stack has decode only on a stack trained with quantize dropout."""
    if stages_given < stack.num_quantizers:
        assert stack.quantize_dropout > 0.0, (
            "quantize dropout must be greater than 0 if you wish to reconstruct from a signal with less fine quantizations"
        )


def pad_stages(idx: torch.Tensor, num_quantizers: int, losses=None):
    """The stages that did not run: index columns of -1, int64 like the reference's null indices (so a stack of int32
    indices is promoted, as its ``torch.stack`` does), and loss columns of 0 when ``losses`` [..., stages] is given."""
    missing = num_quantizers - idx.shape[-1]
    if missing:
        idx = torch.cat([idx.long(), idx.new_full((*idx.shape[:-1], missing), -1, dtype=torch.long)], dim=-1)
        if losses is not None:
            losses = torch.cat([losses, losses.new_zeros((*losses.shape[:-1], missing))], dim=-1)
    return idx, losses


def rows_contiguous(xg: torch.Tensor) -> torch.Tensor:
    """xg [G, N, d] with each row's d values contiguous (the kernels' layout; any group and row strides): a copy only
    when they are not, e.g. a batch-1 [b, d, t] feature map passed as .transpose(1, 2)."""
    if xg.shape[2] > 1 and xg.stride(2) != 1:
        xg = xg.contiguous()
    return xg


def group_rows_in(x: torch.Tensor, stacks, d: int, has_projections: bool):
    """x [..., dim] of a grouped module -> (xg [G, N, d] fp32 with contiguous rows, the dtype its losses take).  Without
    projections the ``x.chunk`` views are read in place (group stride d, row stride G * d); with them every group's
    ``project_in`` runs on its chunk and the results are stacked."""
    G = len(stacks)
    if has_projections:
        xp = [stack.project_in(chunk) for stack, chunk in zip(stacks, x.chunk(G, dim=-1))]
        return torch.stack([t.float().reshape(-1, d) for t in xp]), xp[0].dtype
    return rows_contiguous(x.float().reshape(-1, G, d).transpose(0, 1)), x.dtype


def group_rows_out(out: torch.Tensor, stacks, lead, d: int, has_projections: bool) -> torch.Tensor:
    """out [G, N, d] -> [*lead, dim]: the groups side by side on the feature axis, through their ``project_out`` if any."""
    if has_projections:
        return torch.cat([stack.project_out(out[g].reshape(*lead, d)) for g, stack in enumerate(stacks)], dim=-1)
    return out.transpose(0, 1).reshape(*lead, len(stacks) * d)


def grouped_fallback(stacks, x: torch.Tensor, split_dim: int, seed, return_all_codes: bool, combine_codes, **kwargs):
    """A grouped module as the reference runs it: every stack on its chunk of ``x``, all with the same dropout ``seed`` (drawn
    by the caller, whose business it is when), the quantized chunks concatenated and everything else stacked over the groups
    -- except the optional all-codes entry, which ``combine_codes`` joins (``torch.stack``, or ``tuple``)."""
    outs = tuple(stack(chunk, return_all_codes=return_all_codes, rand_quantize_dropout_fixed_seed=seed, **kwargs)
                 for stack, chunk in zip(stacks, x.chunk(len(stacks), dim=split_dim)))
    quantized, *rest = zip(*outs)
    codes = (combine_codes(rest.pop()),) if return_all_codes else ()
    return (torch.cat(quantized, dim=split_dim), *(torch.stack(r) for r in rest), *codes)


def grouped_decode_rows(indices: torch.Tensor):
    """indices [G, b, ..., q] of a grouped module -> (flat [G, N, q], lead = (b, ...))."""
    lead = indices.shape[1:-1]
    return indices.reshape(indices.shape[0], prod(lead), indices.shape[-1]), lead


def grouped_decode_dest(flat: torch.Tensor, lead, d: int, stages=None):
    """(result, view) of a fresh fp32 buffer for one decode call over all groups of ``flat`` [G, N, q]; the call writes through
    ``view``, whose leading axis is the group.  ``stages`` None: the groups' sums side by side on the feature axis, result
    [*lead, G * d], view [G, N, d].  Else every stage's codes: result [G, stages, *lead, d], view [stages, G, N, d]."""
    G, N = flat.shape[:2]
    if stages is None:
        buf = torch.empty((N, G, d), dtype=torch.float32, device=flat.device)
        return buf.reshape(*lead, G * d), buf.transpose(0, 1)
    buf = torch.empty((G, stages, N, d), dtype=torch.float32, device=flat.device)
    return buf.reshape(G, stages, *lead, d), buf.transpose(0, 1)
