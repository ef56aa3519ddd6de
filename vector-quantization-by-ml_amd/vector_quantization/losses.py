"""Losses that consume the similarity matrix, built so that ``[M, K]`` never exists for all rows.

The reference hands the full ``similarities [h, M, K]`` tensor (its ``distances``) to three rare consumers:

* cross-entropy of the similarities against code indices -- commitment variant and ``indices=`` teacher forcing
  (vector_quantize_pytorch.py:284-299,338-346);
* the codebook diversity loss: entropy of the batch-averaged softmax (vector_quantize_pytorch.py:324-334);
* the orthogonal regulariser, which only looks at the codebook (utils/losses.py:23-28).

Here the forward of the cross entropy is ONE native sweep with an online-softmax epilogue
(``vq_softmax_stats_f32``: per row log-sum-exp + target logit).  Everything that needs actual matrix entries
(backward passes outside the fused kernels' range or below their measured cuts) works on bounded row chunks: ``vq_similarities_f32`` emits a chunk, the
chunk's contribution is evaluated with ordinary tensor ops, and gradients flow through ``_SimilarityFn`` whose
backward is ATen's ``_euclidean_dist_backward`` formula (two library GEMMs per chunk).  The cross entropy's backward with
respect to x is one fused native sweep instead (``vq_ce_backward_f32``; with an EMA codebook, whose update rewrites the codes
between forward and backward, ``vq_ce_backward_live_f32``) wherever the kernels reach: D <= 512, with live codes D <= 256.
A learnable codebook gets the cross entropy's gradient from one more fused sweep (``vq_ce_backward_codes_f32``, D <= 256) from
``CE_CODES_FUSED_MIN_ROWS`` rows per head on (``ce_codes_runs_fused``), unless its codes are rewritten before backward (live
codes); VQ_CE_CODES_NO_FUSED=1 keeps the chunks.
The diversity loss is four fused sweeps (``vq_diversity_*_f32``: row log-sum-exps, the position table [N, K], delta per row,
grad_x -- against the live codes of an EMA codebook) for D <= 256, from ``DIVERSITY_FUSED_MIN_ROWS`` rows per sequence
position on (``diversity_runs_fused``); a learnable codebook gets its gradient from a fifth sweep
(``vq_diversity_backward_codes_f32``) from ``DIVERSITY_CODES_FUSED_MIN_ROWS`` rows on (``diversity_codes_runs_fused``), unless
its codes are rewritten before backward (live codes): such a call runs on the chunks, forward and backward.
The orthogonal regulariser is one fused sweep over the normalised codes (``vq_orthogonal_gram_f32``: row sums of squared
cosines and the gram matrix times the rows, nothing of ``[n, n]``; the backward is a scale of the saved product) for CUDA fp32
codes of d <= 256 dims from ``ORTHOGONAL_FUSED_MIN_CODES`` codes per head on (``orthogonal_runs_fused``, measured per padded
row width and head count); everything else -- CPU
tensors, wider rows, smaller codebooks, VQ_ORTHOGONAL_NO_FUSED=1 -- is the reference's GEMM.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import search

CHUNK_BYTES = 256 << 20  # bound on one materialised [H, rows, K] fp32 chunk


def _rows_per_chunk(h: int, k: int) -> int:
    rows = CHUNK_BYTES // (4 * max(1, h) * max(1, k))
    return max(128, rows // 128 * 128)


class _SimilarityFn(torch.autograd.Function):
    """sims = -cdist(x, c) (Euclid) or x @ c^T (dot) for x [H, M, D], c [H, K, D].

    Backward (same formulas autograd uses for the reference's ops):
      Euclid  ratio = g / sims (0 where sims == 0);  gx = x * ratio.sum(-1) - ratio @ c;  gc = c * ratio.sum(-2) - ratio^T @ x
              (ATen _euclidean_dist_backward with grad_dist = -g and dist = -sims)
      dot     gx = g @ c;  gc = g^T @ x
    """

    @staticmethod
    def forward(ctx, x, codes, metric, live_codes=None):
        sims = search.get_backend().similarities(x.detach(), codes.detach(), metric=metric)
        ctx.save_for_backward(x, codes, sims)
        ctx.metric = metric
        ctx.live_codes = live_codes  # see `live_codes` in similarity_matrix()
        return sims

    @staticmethod
    def backward(ctx, g):
        x, codes, sims = ctx.saved_tensors
        x, codes = x.detach(), (codes if ctx.live_codes is None else ctx.live_codes).detach()
        gx = gc = None
        if ctx.metric == search.EUCLID:
            ratio = torch.where(sims == 0, torch.zeros_like(g), g / sims)
            if ctx.needs_input_grad[0]:
                gx = x * ratio.sum(-1, keepdim=True) - ratio @ codes
            if ctx.needs_input_grad[1]:
                gc = codes * ratio.sum(-2).unsqueeze(-1) - ratio.transpose(-1, -2) @ x
        else:
            if ctx.needs_input_grad[0]:
                gx = g @ codes
            if ctx.needs_input_grad[1]:
                gc = g.transpose(-1, -2) @ x
        return gx, gc, None, None


def similarity_matrix(x: torch.Tensor, codes: torch.Tensor, metric: int, live_codes=None) -> torch.Tensor:
    """The full [H, M, K] matrix (only for callers that really want the reference's third return value).

    ``live_codes``: in the reference the EMA step overwrites the codebook through ``.data`` right after the similarities
    were computed (codebooks.py:418-425), which autograd does not notice: cdist's backward then multiplies the ratio
    matrix -- computed from the OLD distances -- with the UPDATED codebook.  Passing the module's live buffer here
    (while ``codes`` is the pre-update snapshot) reproduces exactly that; with ``None`` the gradient is the consistent one.
    """
    x = x.float()
    if torch.is_grad_enabled() and (x.requires_grad or codes.requires_grad):
        return _SimilarityFn.apply(x, codes, metric, live_codes)
    return search.get_backend().similarities(x, codes, metric=metric)


def _rows_of(chunk):
    return chunk[0] if isinstance(chunk, tuple) else chunk


def _take(x, chunk):
    rows = _rows_of(chunk)
    return x[:, rows] if isinstance(rows, slice) else x.index_select(1, rows)


def _row_slices(m: int, step: int):
    return [slice(r, min(m, r + step)) for r in range(0, m, step)]


def _chunk_grads(chunk_value, x, codes, chunks, g, need_x, need_c):
    """d/d(x, codes) of  g * sum_chunks chunk_value(x[:, rows], codes, chunk), one chunk alive at a time."""
    x, codes = x.detach(), codes.detach()
    gx = torch.zeros_like(x) if need_x else None
    gc = torch.zeros_like(codes) if need_c else None
    for chunk in chunks:
        with torch.enable_grad():
            xc = _take(x, chunk).requires_grad_(need_x)
            cc = codes.requires_grad_(need_c) if need_c else codes
            wanted = [t for t, n in ((xc, need_x), (cc, need_c)) if n]
            grads = torch.autograd.grad(chunk_value(xc, cc, chunk), wanted, g)
        it = iter(grads)
        if need_x:
            rows = _rows_of(chunk)
            if isinstance(rows, slice):
                gx[:, rows] += next(it)
            else:
                gx.index_add_(1, rows, next(it))
        if need_c:
            gc += next(it)
    return gx, gc


class _ChunkedFn(torch.autograd.Function):
    """value = sum over row chunks of chunk_value(x[:, rows], codes, chunk);  recomputed chunk by chunk in backward, so
    only one [H, rows, K] chunk (and its temporaries) is alive at any time."""

    @staticmethod
    def forward(ctx, x, codes, chunk_value, chunks):
        total = None
        with torch.no_grad():
            for chunk in chunks:
                v = chunk_value(_take(x, chunk), codes, chunk)
                total = v if total is None else total + v
        ctx.save_for_backward(x, codes)
        ctx.chunk_value, ctx.chunks = chunk_value, chunks
        return total

    @staticmethod
    def backward(ctx, g):
        x, codes = ctx.saved_tensors
        gx, gc = _chunk_grads(ctx.chunk_value, x, codes, ctx.chunks, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gc, None, None


# ------------------------------------------------------------------------------------------------ cross entropy
class _CrossEntropyFn(torch.autograd.Function):
    """mean over non-ignored (h, m) of  logsumexp_k sims[h, m, k] - sims[h, m, target[h, m]]
    == F.cross_entropy(rearrange(distances, ...), codes, ignore_index=-1)   vector_quantize_pytorch.py:292-294.
    Forward: one native sweep (online softmax).  Backward: one fused sweep (vq_ce_backward_f32, with ``live_codes``
    vq_ce_backward_live_f32); codes that require grad get their gradient from one more sweep (vq_ce_backward_codes_f32) from
    CE_CODES_FUSED_MIN_ROWS rows on (``ce_codes_runs_fused``), unless they are rewritten before backward (live codes) or
    VQ_CE_CODES_NO_FUSED=1 is set.  Bounded chunks of the similarity matrix outside the kernels' range, for such a
    learnable codebook and under VQ_CE_NO_LIVE=1 (live codes only)."""

    @staticmethod
    def forward(ctx, x, codes, target, metric, live_codes=None, lse=None, tl=None, live_packed=None):
        ctx.live_codes, ctx.live_packed = live_codes, live_packed
        if lse is None:  # otherwise the search already produced them (vq_quantize_lse_f32): no second sweep
            lse, tl = search.get_backend().softmax_stats(x.detach(), codes.detach(), metric=metric, scale=1.0,
                                                         target=target)
        valid = target >= 0
        count = valid.sum()
        ctx.save_for_backward(x, codes, target, count, lse, tl)
        ctx.metric = metric
        # (select, not multiply: an ignored row may hold NaN / inf and NaN * 0 is NaN -- ATen's ignore_index never reads such a row)
        return torch.where(valid, lse - tl, torch.zeros_like(lse)).sum() / count

    @staticmethod
    def backward(ctx, g):
        x, codes, target, count, lse, tl = ctx.saved_tensors
        metric, live = ctx.metric, ctx.live_codes
        fused = getattr(search.get_backend(), "cross_entropy_backward", None)
        if live is not None and os.environ.get("VQ_CE_NO_LIVE"):  # (read per call: tests and A/B runs compare both paths)
            fused = None
        if fused is not None and not ctx.needs_input_grad[1]:
            # one fused sweep (S = x c^T, softmax weights, second contraction with the codebook) -- nothing of [M, K]
            coef = (g / count).reshape(1).to(torch.float32)
            if live is None:
                gx = fused(x.detach(), codes.detach(), lse, tl, target, coef, metric=metric)
            else:
                # the weights from `codes` (what the forward searched), the contraction with the codes as they are NOW: `live`
                # and its image are read here, at backward time
                packed = ctx.live_packed() if callable(ctx.live_packed) else ctx.live_packed
                gx = fused(x.detach(), codes.detach(), lse, tl, target, coef, metric=metric, live=live.detach(),
                           live_packed=packed)
            if gx is not None:
                return gx, None, None, None, None, None, None, None
        if fused is not None and ctx.needs_input_grad[1] and _ce_codes_fused(x, codes, live):
            # a learnable codebook: the same sweep for the rows (only when they need a gradient) and one more with the codes
            # resident for theirs (vq_ce_backward_codes_f32) -- nothing of [M, K] either
            backend = search.get_backend()
            coef = (g / count).reshape(1).to(torch.float32)
            gc = backend.cross_entropy_backward_codes(x.detach(), codes.detach(), lse, target, coef, metric=metric)
            gx = fused(x.detach(), codes.detach(), lse, tl, target, coef, metric=metric) if ctx.needs_input_grad[0] else None
            if gc is not None and (gx is not None or not ctx.needs_input_grad[0]):
                return gx, gc, None, None, None, None, None, None

        def chunk_value(xc, cc, rows):
            sims = similarity_matrix(xc, cc, metric, live)
            return F.cross_entropy(sims.reshape(-1, sims.shape[-1]), target[:, rows].reshape(-1), ignore_index=-1,
                                   reduction="sum") / count

        chunks = _row_slices(x.shape[1], _rows_per_chunk(x.shape[0], codes.shape[1]))
        gx, gc = _chunk_grads(chunk_value, x, codes, chunks, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gc, None, None, None, None, None, None


# Rows per head from which the fused backward of a cross entropy whose codes require grad runs, per padded row width (32 / 64 /
# 128 / 256 dims).  The step is two sweeps: vq_ce_backward_f32 for the rows -- one workgroup per 128 rows streams ALL codes, so
# few rows of a large, wide codebook leave the chip idle -- and vq_ce_backward_codes_f32 for the codes; the chunked step is two
# library GEMMs on a matrix that is small when the rows are few.  Measured on an MI355X (profiles/ce_codes_bench.md): forward +
# backward of VectorQuantize(CodebookParams(learnable_codebook=True, ema_update=False), commitment_use_cross_entropy_loss=True)
# in train mode, x [B, N, D], ms, the parent commit's path (VQ_CE_CODES_NO_FUSED=1) / fused, two alternating runs each; "no" =
# the slower fused run was not faster than the faster chunked run:
#   D     K      32 rows                  256 rows                 1024 rows                4096 rows                16384 rows
#   32    1024   0.79 0.57 / 0.31 0.40    0.79 0.56 / 0.31 0.41    0.74 0.68 / 0.43 0.51    0.75 0.69 / 0.42 0.49    0.96 0.70 / 0.43 0.52
#   32    8192   0.83 0.75 / 0.65 0.65    0.80 0.80 / 0.67 0.67    1.08 0.88 / 0.68 0.68    1.26 1.26 / 0.73 0.73    3.25 3.24 / 0.96 0.95
#   64    1024   0.57 0.55 / 0.30 0.30    0.57 0.54 / 0.31 0.30    1.17 0.71 / 0.44 0.51    1.08 0.68 / 0.46 0.52    2.74 0.71 / 0.44 0.52
#   64    8192   1.01 1.01 / 1.01 1.01 no 1.07 1.07 / 1.02 1.02    1.15 1.15 / 1.05 1.05    2.77 1.53 / 1.14 1.14    3.67 3.67 / 1.47 1.46
#   128   1024   0.56 0.54 / 0.31 0.31    0.56 0.54 / 0.32 0.32    0.97 0.69 / 0.44 0.53    1.14 0.68 / 0.44 0.53    1.29 0.72 / 0.44 0.53
#   128   8192   1.49 1.49 / 1.74 1.74 no 1.53 1.53 / 1.76 1.76 no 1.63 1.63 / 1.80 1.80 no 2.10 2.11 / 1.94 1.92    4.66 4.66 / 2.41 2.41
#   256   1024   0.55 0.54 / 0.50 0.50    0.56 0.55 / 0.52 0.52    0.91 0.56 / 0.55 0.55    0.99 0.56 / 0.58 0.58 no 1.28 0.89 / 0.72 0.71
#   256   8192   2.48 2.49 / 3.09 3.09 no 2.55 2.55 / 3.12 3.12 no 2.68 2.68 / 3.19 3.19 no 3.24 3.24 / 3.45 3.44 no 6.77 6.78 / 4.29 4.28
# Per padded row width the cut is the fewest measured rows from which the fused step was faster at every measured K and at
# every larger measured row count; row counts between two measured ones take the higher cut, fewer than 32 rows were not
# measured.  The memory does not depend on the cut (16384 rows, K = 8192: 1.4 GiB -> 17 to 105 MiB): lower the entries to
# trade time for it.
CE_CODES_FUSED_MIN_ROWS = {32: 32, 64: 256, 128: 4096, 256: 16384}


def ce_codes_runs_fused(rows: int, dim: int) -> bool:
    """The dispatch rule of the cross entropy's gradient with respect to a learnable codebook, a pure function of the shape:
    ``rows`` = M rows per head against CE_CODES_FUSED_MIN_ROWS of the padded row width; wider rows keep the chunks."""
    cut = next((c for dp, c in sorted(CE_CODES_FUSED_MIN_ROWS.items()) if dim <= dp), None)
    return cut is not None and rows >= cut


def _ce_codes_fused(x, codes, live) -> bool:
    """The fused sweeps take the backward of a cross entropy whose codes require grad: no live codes (an EMA codebook that
    learns through the orthogonal loss is rewritten before backward), a backend with the codes sweep, the kernel's range, the
    measured cut; VQ_CE_CODES_NO_FUSED=1 keeps the chunks."""
    if live is not None or os.environ.get("VQ_CE_CODES_NO_FUSED"):  # (read per call: tests and A/B runs compare both paths)
        return False
    backend = search.get_backend()
    if getattr(backend, "cross_entropy_backward_codes", None) is None or not x.is_cuda:
        return False
    return ce_codes_runs_fused(x.shape[1], x.shape[2])  # (no entry for rows wider than 256 dims: they keep the chunks)


def cross_entropy_to_codes(x: torch.Tensor, codes: torch.Tensor, target: torch.Tensor, metric: int,
                           live_codes=None, stats=None, live_packed=None) -> torch.Tensor:
    """x [H, M, D] (strided rows fine), codes [H, K, D], target [H, M] int64 with -1 = ignore -> scalar.
    ``live_codes``: see similarity_matrix().  ``stats`` = (lse [H, M], target_logit [H, M]) when the search sweep already
    produced them for exactly this target (cross-entropy commitment loss: target = the chosen code).
    ``live_packed``: the packed image of ``live_codes`` for the fused backward, or a callable that returns it -- called when
    backward runs (``Codebook.packed_codes``: the image the next forward's search needs anyway); None: packed per call."""
    lse, tl = stats if stats is not None else (None, None)
    if lse is not None:
        lse, tl = lse.contiguous(), tl.contiguous()
    return _CrossEntropyFn.apply(x.float(), codes, target, metric, live_codes, lse, tl, live_packed)


# ------------------------------------------------------------------------------------------------ diversity
# Rows per sequence position (and head) from which the fused sweeps run.  The accumulate sweep pads every position's rows to
# whole 32-row sub-tiles, so below 32 rows its work grows by 32 / rows while the position table [N, K] approaches [M, K].
# Measured on an MI355X (profiles/diversity_bench.md): forward + backward of VectorQuantize(codebook_diversity_loss_weight=0.5)
# in train mode with the EMA codebook, ms, chunked (the parent commit) / fused, two alternating runs each:
#   rows  x [B, N, D], K        chunked        fused
#     1   [1, 1024, 64], 8192   2.77 / 2.64    2.96 / 2.94    fused slower
#     1   [1, 16384, 256], 1024 2.55 / 2.52    4.45 / 4.38    fused slower
#     1   [1, 16384, 64], 8192  13.1 / 12.8    12.3 / 12.2
#     2   [2, 1024, 64], 8192   2.96 / 2.89    2.98 / 2.93    no faster
#     2   [2, 16384, 64], 8192  20.6 / 20.2    12.5 / 12.3
#     4   [4, 1024, 64], 1024   1.66 / 1.79    1.06 / 1.20
#     4   [4, 1024, 64], 8192   3.49 / 3.54    2.85 / 2.95
#     4   [4, 16384, 64], 8192  35.1 / 35.0    14.2 / 14.1
#    16   [16, 1024, 64], 1024  1.82 / 1.88    1.07 / 1.19
#    16   [16, 1024, 64], 8192  8.49 / 8.46    3.02 / 3.09
# From 4 rows on the fused path was faster at every measured shape; at 1 and 2 rows it was not, at 3 it was not measured.
DIVERSITY_FUSED_MIN_ROWS = 4


def diversity_runs_fused(rows_per_position: int, heads: int = 1) -> bool:
    """The dispatch rule of the diversity loss, a pure function of the shape: ``rows_per_position`` = C = H * M / N rows of
    all ``heads`` (separate codebooks) at one sequence position.  C >= 32 always runs fused; below that the rows of one head,
    C / heads -- what the accumulate sweep pads to 32 -- decide against DIVERSITY_FUSED_MIN_ROWS."""
    if rows_per_position >= 32:
        return True
    return rows_per_position // max(1, heads) >= DIVERSITY_FUSED_MIN_ROWS


# The cut for a learnable codebook (codes that require grad).  Its gradient is one more sweep over the padded position-major
# image (vq_diversity_backward_codes_f32), so below 32 rows per position the fused step costs what 32 rows cost while the
# chunked step shrinks with the rows -- sooner the wider the rows.  Measured on an MI355X (profiles/diversity_codes_bench.md):
# forward + backward of VectorQuantize(CodebookParams(learnable_codebook=True, ema_update=False),
# codebook_diversity_loss_weight=0.5) in train mode, x [rows, 1024, D], ms, the parent commit (chunked) / fused, two
# alternating runs each; "no" = the slower fused run was not faster than the faster parent run:
#   D     K      4 rows                          8 rows                          16 rows
#   32    8192   3.04 3.17 / 2.61 2.64           4.33 4.41 / 2.62 2.70           -
#   64    1024   1.74 1.64 / 1.07 1.12           1.74 1.64 / 1.08 1.14           1.77 1.72 / 1.08 1.11
#   64    8192   3.49 3.45 / 3.50 3.57   no      4.68 4.69 / 3.51 3.58           9.08 8.72 / 3.59 3.65
#   128   1024   1.37 1.62 / 1.13 1.27           1.44 1.57 / 1.14 1.28           1.62 1.75 / 1.16 1.28
#   128   8192   3.95 4.04 / 5.28 5.34   no      5.29 5.37 / 5.32 5.39   no      9.95 10.07 / 5.48 5.49
#   256   1024   1.37 1.61 / 1.63 1.65   no      1.46 1.60 / 1.64 1.67   no      1.88 1.93 / 1.73 1.75
#   256   8192   5.25 5.42 / 9.04 8.95   no      6.80 6.93 / 9.12 9.09   no      12.89 13.04 / 9.33 9.33
# Per padded row width (32 / 64 / 128 / 256 dims) the cut is the fewest measured rows from which the fused step was faster at
# every measured K; row counts between two measured ones take the higher cut.  The cut of a codebook without a gradient
# (DIVERSITY_FUSED_MIN_ROWS) is not touched by this.
DIVERSITY_CODES_FUSED_MIN_ROWS = {32: 4, 64: 8, 128: 16, 256: 16}


def diversity_codes_runs_fused(rows_per_position: int, heads: int, dim: int) -> bool:
    """The additional dispatch rule when the codes require grad, a pure function of the shape: the rows of one head at one
    sequence position -- what the image pads to 32 -- against DIVERSITY_CODES_FUSED_MIN_ROWS of the padded row width.  32 rows
    of a head and more always run fused."""
    rows = rows_per_position // max(1, heads)
    if rows >= 32:
        return True
    cut = next((c for dp, c in sorted(DIVERSITY_CODES_FUSED_MIN_ROWS.items()) if dim <= dp), None)
    return cut is not None and rows >= cut


def _position_chunks(table: torch.Tensor):
    """Row slices of a position table [N, stride] whose element-wise temporaries stay below CHUNK_BYTES."""
    return _row_slices(table.shape[0], max(1, CHUNK_BYTES // (4 * table.shape[1])))


def diversity_upstream(table: torch.Tensor, g, n_positions: int, count: int, k: int):
    """U = dL/dp per (position, code) from the position table A [N, stride] (K real columns) and the upstream gradient g of
    the loss: d loss / d A = (log(max(A, 1e-5)) + [A >= 1e-5]) / N (ATen's clamp backward) and d A / d p = 1 / C.
    -> (U - centre, centre [N]): dL/ds = -T p (U - delta) does not change when a row of U is shifted (delta = sum_k p U
    shifts with it), so every row is handed to the sweeps minus its mean over the K codes: at a low temperature the entries
    of a row differ by a small fraction of their size, and U - delta would otherwise cancel most of its digits.  The padding
    of the table past K holds A = 0, which gives a finite value there (the sweeps read and discard it)."""
    scale = torch.as_tensor(g, dtype=torch.float32, device=table.device) / (n_positions * count)
    u = torch.empty_like(table)
    centre = torch.empty(table.shape[0], dtype=table.dtype, device=table.device)
    for rows in _position_chunks(table):  # (the temporaries stay below CHUNK_BYTES)
        t = table[rows]
        v = (t.clamp(min=1e-5).log() + (t >= 1e-5).to(t.dtype)) * scale
        centre[rows] = v[:, :k].mean(dim=-1)
        u[rows] = v - centre[rows, None]
    return u, centre


class _DiversityFn(torch.autograd.Function):
    """The diversity loss through the fused sweeps (vq_diversity_*_f32): nothing of [M, K].  Forward: row log-sum-exps, the
    position table A [N, K], then the entropy with the reference's own tensor ops on A.  Backward: U [N, K] from A and the
    upstream gradient, delta per row, one sweep for grad_x -- against ``live_codes`` when the codes were rewritten since
    (weights from ``codes``, contraction with ``live_codes``: the convention of _CrossEntropyFn).  A learnable codebook
    (``codes`` requires grad, no live codes: _diversity_fused_backend admits nothing else) gets its gradient from one more
    sweep (vq_diversity_backward_codes_f32) that shares delta with the rows' sweep; the rows' sweep is skipped when only the
    codes need a gradient."""

    @staticmethod
    def forward(ctx, x, codes, metric, temperature, n_positions, pos_div, live_codes, live_packed, backend):
        lse2, table, packed = backend.diversity_table(x.detach(), codes.detach(), metric=metric, temperature=temperature,
                                                      n_positions=n_positions, pos_div=pos_div)
        total = None
        for rows in _position_chunks(table):  # (one chunk unless [N, K] itself outgrows CHUNK_BYTES)
            avg = table[rows, :codes.shape[1]]
            ent = (-avg * avg.clamp(min=1e-5).log()).sum(-1)  # utils/general.py:25-30
            total = ent.sum() if total is None else total + ent.sum()
        ctx.save_for_backward(x, codes, lse2, table, packed)
        ctx.args = (metric, temperature, n_positions, pos_div)
        ctx.live_codes, ctx.live_packed, ctx.backend = live_codes, live_packed, backend
        return -total / n_positions

    @staticmethod
    def backward(ctx, g):
        x, codes, lse2, table, packed = ctx.saved_tensors
        metric, temperature, n_positions, pos_div = ctx.args
        count = x.shape[0] * x.shape[1] // n_positions  # C: rows per position over all heads
        u, _ = diversity_upstream(table, g, n_positions, count, codes.shape[1])
        live, live_packed = ctx.live_codes, ctx.live_packed
        if ctx.needs_input_grad[1]:
            gx, gc = ctx.backend.diversity_backward_codes(x.detach(), codes.detach(), lse2, u.contiguous(), metric=metric,
                                                          temperature=temperature, n_positions=n_positions, pos_div=pos_div,
                                                          packed=packed, need_x=ctx.needs_input_grad[0])
            return gx, gc, None, None, None, None, None, None, None
        if live is not None:  # read here, at backward time: the codes as they are NOW and their image
            live = live.detach()
            live_packed = live_packed() if callable(live_packed) else live_packed
        gx = ctx.backend.diversity_backward(x.detach(), codes.detach(), lse2, u.contiguous(), metric=metric, temperature=temperature,
                                            n_positions=n_positions, pos_div=pos_div, packed=packed, live=live,
                                            live_packed=live_packed)
        return gx, None, None, None, None, None, None, None, None


def _diversity_fused_backend(x, codes, n_positions, pos_div, live_codes=None):
    """The backend whose fused sweeps take this call, or None: the chunked path."""
    if os.environ.get("VQ_DIVERSITY_NO_FUSED"):  # (read per call: tests and A/B runs compare both paths)
        return None
    backend = search.get_backend()
    if not (hasattr(backend, "diversity_table") and hasattr(backend, "diversity_backward")):
        return None
    if not x.is_cuda:
        return None
    # a learnable codebook: the backend needs the codes sweep, and codes that are rewritten before backward (live codes: an
    # EMA codebook whose codes require grad for the orthogonal loss) keep the chunked path
    learnable = torch.is_grad_enabled() and codes.requires_grad
    if learnable and (live_codes is not None or getattr(backend, "diversity_backward_codes", None) is None):
        return None
    h, m, d = x.shape
    if pos_div is None or n_positions <= 0 or m == 0 or m % (n_positions * pos_div):
        return None
    if not diversity_runs_fused(h * m // n_positions, h):
        return None
    if learnable and not diversity_codes_runs_fused(h * m // n_positions, h, d):
        return None
    if not backend.diversity_supported(h, m, codes.shape[1], d, n_positions, pos_div):
        return None
    if learnable and not backend.diversity_codes_supported(h, m, codes.shape[1], d, n_positions, pos_div):
        return None
    return backend


def codebook_diversity_loss(x: torch.Tensor, codes: torch.Tensor, metric: int, temperature: float,
                            position: torch.Tensor, n_positions: int, live_codes=None, pos_div=None,
                            live_packed=None) -> torch.Tensor:
    """-mean_n entropy(avg_prob[n]),  avg_prob[n] = mean over all (head, batch) rows at sequence position n of
    softmax(-similarities * temperature)   -- vector_quantize_pytorch.py:324-334 (sign and all).

    x [H, M, D]; position [M] int64 = sequence position of each row, or a callable that returns it (only the chunked path
    asks).  ``pos_div``: position[m] == (m // pos_div) % n_positions -- with it the fused sweeps run (_DiversityFn) wherever
    they reach: D <= 256, diversity_runs_fused(), and -- when ``codes`` requires grad (a learnable codebook) -- no
    ``live_codes`` and diversity_codes_runs_fused(); VQ_DIVERSITY_NO_FUSED=1 keeps the chunked path.  ``live_packed``: as in cross_entropy_to_codes.
    Chunked over positions otherwise: every chunk holds all rows of a set of positions, so its entropies are complete and
    the loss is a plain sum over chunks.
    """
    backend = _diversity_fused_backend(x, codes, n_positions, pos_div, live_codes)
    if backend is not None:
        return _DiversityFn.apply(x.float(), codes, metric, float(temperature), int(n_positions), int(pos_div), live_codes,
                                  live_packed, backend)
    if callable(position):
        position = position()
    h, m, _ = x.shape
    k = codes.shape[1]
    counts = torch.bincount(position, minlength=n_positions)
    rows_per_pos = max(1, m // max(1, n_positions))
    pos_per_chunk = max(1, _rows_per_chunk(h, k) // rows_per_pos)
    if pos_per_chunk >= n_positions:
        chunks = [(slice(0, m), 0, n_positions)]
    else:
        order = torch.argsort(position, stable=True)  # rows grouped by position
        bounds = [0] + torch.cumsum(counts, 0).tolist()
        chunks = [(order[bounds[p0]:bounds[min(n_positions, p0 + pos_per_chunk)]], p0, min(n_positions, p0 + pos_per_chunk))
                  for p0 in range(0, n_positions, pos_per_chunk)]

    def chunk_value(xc, cc, chunk):
        rows, p0, p1 = chunk
        sims = similarity_matrix(xc, cc, metric, live_codes)
        prob = (-sims * temperature).softmax(dim=-1)  # [H, R, K]
        local = (position[rows] if isinstance(rows, slice) else position.index_select(0, rows)) - p0
        acc = torch.zeros((p1 - p0, k), dtype=prob.dtype, device=prob.device).index_add(0, local, prob.sum(0))
        avg = acc / (counts[p0:p1, None].to(prob.dtype) * h)
        ent = (-avg * avg.clamp(min=1e-5).log()).sum(-1)  # utils/general.py:25-30
        return -ent.sum() / n_positions

    return _ChunkedFn.apply(x.float(), codes, chunk_value, chunks)


# ------------------------------------------------------------------------------------------------ orthogonal
# Codes per head from which the fused sweep runs: per padded row width (32 / 64 / 128 / 256 dims) a map {heads: cut}; the cuts
# of the listed head counts <= h apply to h heads (the smallest wins: more heads only add workgroups), a width without an entry
# for the head count keeps the GEMM.  A wave owns 32 rows for the whole sweep and nothing splits the streamed side, so one head
# of n codes is n / 32 waves on a chip of 1 024 SIMDs: a single codebook of 4 096 or 8 192 wide codes runs on a quarter of the
# CUs and loses to the library GEMMs, eight of them fill the chip.  Measured on an MI355X (profiles/orthogonal_bench.md):
# losses.orthogonal_loss forward + backward, ms, the parent commit (GEMM) / fused, two alternating runs each; "no" = the slower
# fused run was not faster than the faster parent run:
#   h  n       d = 32                     d = 64                     d = 128                       d = 256
#   1  256     0.40 0.39 / 0.30 0.29      0.40 0.40 / 0.22 0.30      0.40 0.40 / 0.22 0.29         0.39 0.30 / 0.22 0.30  no
#   1  512     0.41 0.42 / 0.30 0.30      0.41 0.41 / 0.22 0.30      0.41 0.41 / 0.21 0.30         0.40 0.29 / 0.22 0.30  no
#   1  1024    0.41 0.41 / 0.30 0.30      0.41 0.41 / 0.22 0.29      0.41 0.41 / 0.22 0.30         0.41 0.29 / 0.33 0.33  no
#   1  2048    0.41 0.41 / 0.30 0.30      0.41 0.41 / 0.23 0.30      0.41 0.41 / 0.34 0.34         0.40 0.29 / 0.59 0.59  no
#   1  4096    0.41 0.41 / 0.31 0.31      0.40 0.41 / 0.38 0.38      0.41 0.36 / 0.61 0.61  no     0.42 0.42 / 1.09 1.09  no
#   1  8192    0.74 0.74 / 0.45 0.45      0.80 0.80 / 0.70 0.69      0.97 0.97 / 1.14 1.14  no     1.32 1.32 / 2.08 2.08  no
#   1  16384   2.53 2.54 / 0.83 0.83      2.78 2.80 / 1.31 1.32      3.54 3.60 / 2.20 2.19         4.92 5.09 / 4.06 4.05
#   8  8192    4.91 4.93 / 0.78 0.78      5.62 5.59 / 1.25 1.28      7.02 7.01 / 2.18 2.17         10.09 10.08 / 4.35 4.34
# Per padded width and measured head count the cut is the fewest measured codes from which the fused step was faster at every
# larger measured size; sizes (and head counts) between two measured ones take the higher cut.  The memory does not depend on
# the cut (h = 8, n = 8192: 8.4 GiB -> 49 to 385 MiB): lower the entries, or set {dp: {1: 1}}, to trade time for it.
ORTHOGONAL_FUSED_MIN_CODES = {32: {1: 256}, 64: {1: 256}, 128: {1: 16384, 8: 8192}, 256: {1: 16384, 8: 8192}}
ORTHOGONAL_MAX_DIM = 256  # vq_orthogonal_gram_f32: rows of one launch


def orthogonal_runs_fused(n_codes: int, dim: int, heads: int = 1) -> bool:
    """The dispatch rule of the orthogonal loss, a pure function of the shape: ``n_codes`` per head against the cuts that
    ORTHOGONAL_FUSED_MIN_CODES lists for the padded row width at head counts up to ``heads``."""
    by_heads = next((c for dp, c in sorted(ORTHOGONAL_FUSED_MIN_CODES.items()) if dim <= dp), None)
    cuts = [c for hh, c in (by_heads or {}).items() if heads >= hh]
    return bool(cuts) and n_codes >= min(cuts)


class _OrthogonalFn(torch.autograd.Function):
    """sum_{h,i,j} cos_ij^2 of rows that are already normalised, through one fused sweep (vq_orthogonal_gram_f32): nothing of
    [n, n].  Forward: rowsq_i = sum_j cos_ij^2 and -- only when a gradient is needed -- G_i = sum_j cos_ij normed_j, saved.
    Backward: d/d normed_i = 4 G_i (cos is symmetric: row i appears on both sides), a scale of the saved G; no second sweep."""

    @staticmethod
    def forward(ctx, normed, backend):
        rowsq, gram = backend.orthogonal_gram(normed.detach(), want_g=ctx.needs_input_grad[0])
        ctx.save_for_backward(gram)
        return rowsq.sum(dtype=torch.float64).to(torch.float32)  # (no host synchronisation)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (gram,) = ctx.saved_tensors
        return g * 4 * gram, None


def _orthogonal_fused_backend(codes):
    """The backend whose fused sweep takes this call, or None: the GEMM."""
    if os.environ.get("VQ_ORTHOGONAL_NO_FUSED"):  # (read per call: tests and A/B runs compare both paths)
        return None
    if not (codes.is_cuda and codes.dtype == torch.float32 and codes.dim() == 3):
        return None
    h, n, d = codes.shape
    if h == 0 or n == 0 or d == 0 or d > ORTHOGONAL_MAX_DIM or not orthogonal_runs_fused(n, d, h):
        return None
    backend = search.get_backend()
    return backend if getattr(backend, "orthogonal_gram", None) is not None else None


def orthogonal_loss(codes: torch.Tensor) -> torch.Tensor:
    """Eq. (2) of arXiv:2112.00384 on codes [h, n, d]  (utils/losses.py:23-28): mean squared cosine similarity
    between codes, minus 1/n.  Touches only the codebook.  CUDA fp32 codes of d <= 256 dims run as one fused sweep over the
    normalised codes (_OrthogonalFn: no [n, n] matrix, forward or backward) from ORTHOGONAL_FUSED_MIN_CODES codes on;
    VQ_ORTHOGONAL_NO_FUSED=1, CPU tensors, other dtypes, wider rows and smaller codebooks keep the library GEMM."""
    h, n = codes.shape[:2]
    normed = F.normalize(codes, p=2, dim=-1)
    backend = _orthogonal_fused_backend(codes)
    if backend is not None:
        return _OrthogonalFn.apply(normed, backend) / (h * n ** 2) - (1 / n)
    cos = normed @ normed.transpose(-1, -2)
    return (cos ** 2).sum() / (h * n ** 2) - (1 / n)
