"""Functional seam between the nn.Modules and the native op.

``quantize_rows`` is the ONE call every module makes for the hot path.  It dispatches to
``native.quantize`` (HIP kernels through the C ABI).  There is no CPU implementation in this package -- not for the
search, not for the similarity consumers, not for the EMA statistics: every device-side step goes through the backend
object below.  Tests may install a checker backend with ``set_backend`` (tests/ only) to exercise the host-side
layout logic on a machine without a GPU.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import native

EUCLID = native.EUCLID
DOT = native.DOT


LSE_MAX_DIM = 512  # vq_quantize_lse_f32: rows of one launch


def _want_deterministic(dim: int) -> bool:
    """torch.use_deterministic_algorithms(True) selects the reproducible EMA accumulation (rows of up to 2048 dims).
    Wider rows only have the float-atomic kernel: torch's own convention applies -- raise, or warn under ``warn_only``."""
    if not torch.are_deterministic_algorithms_enabled():
        return False
    if dim <= 2048:
        return True
    msg = (f"the EMA statistics of rows wider than 2048 dims (got {dim}) are accumulated with float atomics and have no "
           "deterministic implementation; turn torch.use_deterministic_algorithms off (or use warn_only=True) for this step")
    if torch.is_deterministic_algorithms_warn_only_enabled():
        import warnings

        warnings.warn(msg)
        return False
    raise RuntimeError(msg)


class _NativeBackend:
    name = "hip-gfx950"
    accepts_half_rows = True  # fp16 / bf16 rows are widened in the kernel's prologue (inference launches)
    uses_packed = True        # callers may hand over a cached packed image of the codebooks (``pack``)

    @staticmethod
    @torch.compiler.assume_constant_result  # host arithmetic in the library: a constant of (dim, want_sq_err) for a trace
    def max_fused_stages(dim, want_sq_err):
        """How many residual stages one launch can hold (vq_max_fused_stages); longer stacks run layer by layer."""
        return native.max_fused_stages(dim, want_sq_err)

    @staticmethod
    def pack(cb, metric):
        """cb [..., K, D] contiguous fp32 -> packed images [n, packed_floats] (vq_pack_codebooks_f32)."""
        if torch.compiler.is_compiling():
            from . import ops

            return ops.pack(cb, metric)
        return native.pack_codebooks(cb, metric)

    @staticmethod
    def pack_screen(packed, H, K, D, metric):
        """packed images of ``pack`` -> the screen image the screened sweep reads (vq_pack_screen_image_f32), or None where
        no screened sweep exists for the shape.  One image serves one stream."""
        return native.pack_screen(packed, H, K, D, metric)

    @staticmethod
    def quantize(x, cb, *, metric, ste, want_sq_err, share, want_best=False, out=None, idx=None, want_lse=False,
                 sq_err_per_head=False, packed=None, screen=None):
        """-> (out, idx, best, sq_err) and, with ``want_lse`` (single stage), a fifth element: the per-row log-sum-exp
        of the similarities from the same sweep (vq_quantize_lse_f32).  ``screen``: the cached image of ``pack_screen``
        (eager calls only: a traced call packs its own)."""
        if torch.compiler.is_compiling() and not (want_best or want_lse):
            # being traced by torch.compile / export: go through the registered op (ops.py) so the graph does not break here
            from . import ops

            H, M, D = x.shape
            Q = idx.shape[-1] if idx is not None else (1 if share else cb.shape[1])
            if out is None:
                out = torch.empty((H, M, D), dtype=torch.float32, device=x.device)
            if idx is None:
                idx = torch.empty((H, M, Q), dtype=torch.int64, device=x.device)
            sq_err = ops.quantize_into(x, cb, packed, out, idx, metric, ste, want_sq_err, share, sq_err_per_head)
            return out, idx, None, (sq_err if want_sq_err else None)
        r = native.quantize(x, cb, metric=metric, ste=ste, want_sq_err=want_sq_err, want_best=want_best or want_lse,
                            stages_share_codebook=share, out=out, idx=idx, want_lse=want_lse,
                            sq_err_per_head=sq_err_per_head, packed=packed, screen=screen)
        if want_lse:
            return r["out"], r["idx"], r["best"], r["sq_err"], r["lse"]
        return r["out"], r["idx"], r["best"], r["sq_err"]

    @staticmethod
    def shard_keys(x, cb, *, metric, idx_offset, packed=None):
        """Search ONE SHARD of a codebook: x [H, M, D], cb [H, K_local, D] -> packed signed 64-bit keys, candidate planes
        [P, H, M] ((order image of the winning value) << 32 | idx_offset + local index; vq_search_key_planes_f32: one
        launch, no init, no atomics -- P = the K splits that fill the chip for this shape).  The element-wise MIN over the
        planes of all shards is the whole codebook's winner, lowest index on ties."""
        return native.search_key_planes(x, cb, metric=metric, idx_offset=idx_offset, packed=packed)

    @staticmethod
    def finalize_keys(x, table, keys, *, metric):
        """Keys [H, M] or candidate planes [C, H, M] (MIN taken on the fly) + a FULL natural table [H, K, D] ->
        (quantized rows [H, M, D], idx [H, M]) (vq_finalize_key_planes_f32)."""
        r = native.finalize_keys(x, table, keys, metric=metric)
        return r["out"], r["idx"]

    @staticmethod
    def similarities(x, cb, *, metric, out=None):
        """x [H, M, D], cb [H, K, D] -> [H, M, K]  (vq_similarities_f32)."""
        return native.similarities(x, cb.contiguous(), metric=metric, out=out)

    @staticmethod
    def softmax_stats(x, cb, *, metric, scale, target=None):
        """-> (logsumexp_k scale * sim [H, M], logit of target [H, M] | None)  (vq_softmax_stats_f32)."""
        return native.softmax_stats(x, cb.contiguous(), metric=metric, scale=scale, target=target)


    @staticmethod
    def ema_accumulate(x, idx, k, mask=None):
        """-> (counts [H, K], sums [H, K, D]) of the rows assigned to each code (vq_ema_accumulate_f32; under
        torch.use_deterministic_algorithms(True) the atomics-free vq_ema_accumulate_det_f32)."""
        return native.ema_accumulate(x, idx, k, mask, deterministic=_want_deterministic(x.shape[-1]))

    @staticmethod
    def ema_accumulate_residual(x, cb, idx, *, ste, share):
        """-> (counts [H, Q, K], sums [H, Q, K, D]) for every stage of a residual stack (vq_ema_accumulate_residual_f32)."""
        return native.ema_accumulate_residual(x, cb, idx, ste=ste, stages_share_codebook=share,
                                              deterministic=_want_deterministic(x.shape[-1]))

    @staticmethod
    def ema_update(cluster_size, embed_avg, embeddings, hits, sums, *, decay, eps, l2norm):
        """In-place lerp / Laplace smoothing / normalise of the module buffers (vq_ema_update_f32)."""
        native.ema_update(cluster_size, embed_avg, embeddings, hits, sums, decay, eps, l2norm)

    @staticmethod
    def expire_codes(cluster_size, embed_avg, embeddings, pool=None, *, chain=None, stage=0, threshold, reset_cluster_size,
                     l2norm, seed):
        """Dead-code expiry decided on the device, in place on the three buffers (vq_expire_codes_f32): no host
        synchronisation.  ``pool`` [H | 1, N, D], or ``chain`` = (x [M, D], codes [Q | 1, K, D], idx [M, Q]) with ``stage``."""
        if torch.compiler.is_compiling():
            from . import ops

            cx, cc, ci = chain if chain is not None else (None, None, None)
            ops.expire_codes(cluster_size, embed_avg, embeddings, pool, cx, cc, ci, int(stage), float(threshold),
                             float(reset_cluster_size), bool(l2norm), seed)
            return
        native.expire_codes(cluster_size, embed_avg, embeddings, pool, chain=chain, stage=stage, threshold=threshold,
                            reset_cluster_size=reset_cluster_size, l2norm=l2norm, seed=seed)

    @staticmethod
    def column_stats(x, mask=None):
        """-> (count [H] int64, mean [H, D], m2 [H, D]) of the kept rows of x [H, M, D] in one read (vq_affine_stats_f32)."""
        return native.column_stats(x, mask)

    @staticmethod
    def affine_apply(src, codebook_mean, codebook_variance, batch_mean, batch_variance, *, mode, hits=None, out=None):
        """The affine codebook's moment-matching transform of codes (mode 0) or accumulated sums (mode 1), vq_affine_apply_f32."""
        return native.affine_apply(src, codebook_mean, codebook_variance, batch_mean, batch_variance, mode=mode, hits=hits,
                                   out=out)

    @staticmethod
    def quantize_backward(x, cb, idx, grad_out, grad_sq_err, *, ste, share, sq_err_per_head=False):
        """d/dx of the quantize step in one native pass (vq_quantize_backward_f32)."""
        return native.quantize_backward(x, cb, idx, grad_out, grad_sq_err, ste=ste, stages_share_codebook=share,
                                        sq_err_per_head=sq_err_per_head)

    @staticmethod
    def rotate_backward(x, cb, idx, grad_out, grad_sq_err, *, ste=True, share, sq_err_per_head=False):
        """d/dx of the quantize step under the rotation trick in one native pass (vq_rotate_backward_f32); None for rows the
        kernel does not hold in registers (D > native.ROTATE_MAX_DIM: the caller runs the same formulas stage by stage)."""
        if x.shape[-1] > native.ROTATE_MAX_DIM:
            return None
        return native.rotate_backward(x, cb, idx, grad_out, grad_sq_err, ste=ste, stages_share_codebook=share,
                                      sq_err_per_head=sq_err_per_head)

    @staticmethod
    def residual_mask(x, cb, idx, mask, zero_idx, *, train, want_sq_err, per_group=False, out=None):
        """The mask pass of a residual stack after the fused search (vq_residual_mask_f32): rewrites ``idx`` on the
        masked-out rows -> (out [G, M, D], sq_err over the kept rows | None)."""
        if torch.compiler.is_compiling():
            from . import ops

            if out is None:
                out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            sq_err = ops.residual_mask(x, cb, idx, mask, zero_idx, out, train, want_sq_err, per_group)
            return out, (sq_err if want_sq_err else None)
        return native.residual_mask(x, cb, idx, mask, zero_idx, train=train, want_sq_err=want_sq_err,
                                    sq_err_per_group=per_group, out=out)

    @staticmethod
    def residual_mask_backward(x, cb, idx, mask, grad_out, grad_sq_err, *, train, per_group=False):
        """d/dx of the mask pass in one native pass (vq_residual_mask_backward_f32)."""
        return native.residual_mask_backward(x, cb, idx, mask, grad_out, grad_sq_err, train=train, sq_err_per_group=per_group)

    @staticmethod
    def cross_entropy_backward(x, cb, lse, target_logit, target, coef, *, metric, live=None, live_packed=None):
        """Fused d/dx of the cross entropy (vq_ce_backward_f32); None when the shape is outside the kernel's range.
        ``live`` [H, K, D]: the codes as they are now when they were rewritten after ``cb`` was searched, ``live_packed`` their
        packed image if the caller holds one (vq_ce_backward_live_f32: D <= 256)."""
        if x.shape[-1] > (native.CE_BACKWARD_MAX_DIM if live is None else native.CE_BACKWARD_LIVE_MAX_DIM):
            return None
        return native.ce_backward(x, cb.contiguous(), lse, target_logit, target, coef, metric=metric, live=live,
                                  live_packed=live_packed)

    @staticmethod
    def cross_entropy_backward_codes(x, cb, lse, target, coef, *, metric):
        """Fused d/dcodes of the cross entropy for a learnable codebook (vq_ce_backward_codes_f32) -> gc [H, K, D]; None when
        the shape is outside the kernel's range (D > 256, 2^31 rows, a packed row image of 2 GiB: the caller works on row
        chunks)."""
        h, m, d = x.shape
        if d > native.CE_CODES_MAX_DIM or (m > 0 and not native.ce_codes_supported(h, m, cb.shape[1], d)):
            return None
        return native.ce_backward_codes(x, cb.contiguous(), lse.contiguous(), target, coef, metric=metric)

    @staticmethod
    def diversity_supported(H, M, K, D, n_positions, pos_div):
        """The fused sweeps of the codebook diversity loss take this shape (native.diversity_supported)."""
        return native.diversity_supported(H, M, K, D, n_positions, pos_div)

    @staticmethod
    def diversity_table(x, cb, *, metric, temperature, n_positions, pos_div):
        """Forward of the fused diversity loss: -> (lse2 [H, stride(M)], A [n_positions, stride(K)], the packed codes) from
        vq_diversity_stats_f32 and vq_diversity_accumulate_f32; A[n] = mean softmax(-temperature * sim) over the rows (of all
        heads) at sequence position n = (row // pos_div) % n_positions."""
        cb = cb.contiguous()
        packed = native.pack_codebooks(cb, metric)
        lse2 = native.diversity_stats(x, cb, metric=metric, temperature=temperature, packed=packed)
        table = native.diversity_accumulate(x, cb, lse2, metric=metric, temperature=temperature, n_positions=n_positions,
                                            pos_div=pos_div)
        return lse2, table, packed

    @staticmethod
    def diversity_backward(x, cb, lse2, u, *, metric, temperature, n_positions, pos_div, packed=None, live=None, live_packed=None):
        """Backward of the fused diversity loss with respect to the rows: vq_diversity_delta_f32 + vq_diversity_backward_x_f32;
        ``u`` [n_positions, stride(K)] carries the upstream gradient, ``live`` / ``live_packed`` as in cross_entropy_backward."""
        cb = cb.contiguous()
        kw = dict(metric=metric, temperature=temperature, n_positions=n_positions, pos_div=pos_div, packed=packed)
        delta = native.diversity_delta(x, cb, lse2, u, **kw)
        return native.diversity_backward_x(x, cb, lse2, delta, u, live=live, live_packed=live_packed, **kw)

    @staticmethod
    def diversity_codes_supported(H, M, K, D, n_positions, pos_div):
        """The fused codes sweep of the diversity loss takes this shape (native.diversity_codes_supported)."""
        return native.diversity_codes_supported(H, M, K, D, n_positions, pos_div)

    @staticmethod
    def diversity_backward_codes(x, cb, lse2, u, *, metric, temperature, n_positions, pos_div, packed=None, need_x=True):
        """Backward of the fused diversity loss for a learnable codebook (no live codes: the searched codes are the ones that
        learn) -> (gx | None, gc [H, K, D]): vq_diversity_delta_f32 once for both sweeps, vq_diversity_backward_x_f32 only when
        the rows need a gradient, vq_diversity_backward_codes_f32."""
        cb = cb.contiguous()
        kw = dict(metric=metric, temperature=temperature, n_positions=n_positions, pos_div=pos_div)
        delta = native.diversity_delta(x, cb, lse2, u, packed=packed, **kw)
        gx = native.diversity_backward_x(x, cb, lse2, delta, u, packed=packed, **kw) if need_x else None
        return gx, native.diversity_backward_codes(x, cb, lse2, delta, u, **kw)

    @staticmethod
    def orthogonal_gram(x, *, want_g=True):
        """The fused sweep of the orthogonal regularisation loss (vq_orthogonal_gram_f32) over the rows x [H, n, D] as given:
        -> (rowsq [H, n], G [H, n, D] | None), nothing of [n, n]."""
        return native.orthogonal_gram(x, want_g=want_g)

    @staticmethod
    def sample_codes(x, cb, *, metric, tau, seed, packed=None):
        """Gumbel-max sampling of the code in one sweep (vq_gumbel_sample_f32): -> idx [H, M] int64 = argmax_k of
        similarity * tau + Gumbel noise, the noise counter-based from ``seed`` (two int64 words on the device,
        gumbel.draw_seed); None when the shape is outside the kernel's range (D > 512: the caller works on row chunks)."""
        if x.shape[-1] > native.SAMPLE_MAX_DIM:
            return None
        if torch.compiler.is_compiling():
            from . import ops

            return ops.gumbel_sample(x, cb.contiguous(), packed, seed, metric, float(tau))
        return native.sample_codes(x, cb.contiguous(), metric=metric, tau=tau, seed=seed, packed=packed)

    @staticmethod
    def decode(cb, indices, *, num_stages=None, drop_null=True, want_sum=True, want_all=False, sum_out=None, all_out=None):
        """Indices -> code vectors in one pass (vq_decode_f32): cb [G | 1, Q | 1, K, D], indices [G, N, Qg] ->
        (codes_sum [G, N, D] | None, all_codes [Q, G, N, D] | None); see native.decode_codes."""
        if torch.compiler.is_compiling() and sum_out is None and all_out is None:
            from . import ops

            q = int(num_stages) if num_stages is not None else cb.shape[1]
            s, a = ops.decode_codes(cb, indices, q, drop_null, want_sum, want_all)
            return (s if want_sum else None), (a if want_all else None)
        return native.decode_codes(cb, indices, num_stages=num_stages, drop_null=drop_null, want_sum=want_sum,
                                   want_all=want_all, sum_out=sum_out, all_out=all_out)

    @staticmethod
    def lfq_decode(indices, mag, d, *, drop_null=True, want_sum=True, want_all=False, sum_out=None, all_out=None):
        """Indices -> code vectors of the lookup-free family in one pass (vq_lfq_decode_f32): indices [G, N, Qg], one code
        magnitude per stage -> (codes_sum [G, N, d] | None, all_codes [len(mag), G, N, d] | None); see native.lfq_decode."""
        if torch.compiler.is_compiling() and sum_out is None and all_out is None:
            from . import ops

            s, a = ops.lfq_decode(indices, list(mag), d, drop_null, want_sum, want_all)
            return (s if want_sum else None), (a if want_all else None)
        return native.lfq_decode(indices, mag, d, drop_null=drop_null, want_sum=want_sum, want_all=want_all,
                                 sum_out=sum_out, all_out=all_out)

    @staticmethod
    def gumbel_backward(x, cb, g, *, metric, tau, need_x=True, need_codes=True):
        """Fused backward of the straight-through Gumbel softmax through the similarities: (gx | None, gc_sim | None) from
        vq_gumbel_stats_f32 + vq_gumbel_backward_x_f32 / vq_gumbel_backward_codes_f32; None when the shape is outside the
        kernels' range (the caller then works on row chunks)."""
        ready = _gumbel_inputs(x, cb, g, metric, need_codes)
        if ready is None:
            return None
        cb, g, packed = ready
        lse2, delta = native.gumbel_stats(x, cb, g, metric=metric, tau=tau, packed=packed)
        gx = native.gumbel_backward_x(x, cb, g, lse2, delta, metric=metric, tau=tau, packed=packed) if need_x else None
        gc = native.gumbel_backward_codes(x, cb, g, lse2, delta, metric=metric, tau=tau) if need_codes else None
        return gx, gc

    @staticmethod
    def reinmax_backward(x, cb, g, ind, *, metric, tau, need_x=True, need_codes=True):
        """Fused backward of the reinmax Gumbel softmax through the similarities: (gx | None, gc_sim | None) from
        vq_gumbel_reinmax_stats_f32, vq_gumbel_reinmax_columns_f32 (the normalisation over the rows of a head) and
        vq_gumbel_reinmax_backward_x_f32 / vq_gumbel_reinmax_backward_codes_f32; ``ind`` [H, M] int64 is the selection the
        forward made (any selection: it is only compared with code indices).  None when the shape is outside the kernels'
        range (the caller then works on row chunks)."""
        ready = _gumbel_inputs(x, cb, g, metric, True)  # (the column sweep is codes-resident whatever is asked for)
        if ready is None:
            return None
        cb, g, packed = ready
        stats = native.gumbel_reinmax_stats(x, cb, g, metric=metric, tau=tau, packed=packed)
        col, e, ws = native.gumbel_reinmax_columns(x, cb, g, stats[0], ind, metric=metric, tau=tau)
        gx = native.gumbel_reinmax_backward_x(x, cb, g, stats, ind, col, e, metric=metric, tau=tau, packed=packed) if need_x else None
        gc = native.gumbel_reinmax_backward_codes(x, cb, g, stats, col, e, ws, metric=metric, tau=tau) if need_codes else None
        return gx, gc


def _gumbel_inputs(x, cb, g, metric, codes_resident):
    """What both fused Gumbel backwards start from: None when the shape is outside the kernels' range (``codes_resident``: a
    codes-resident sweep will run), else (cb contiguous, g with contiguous dims, the packed codebook)."""
    H, M, D = x.shape
    K = cb.shape[1]
    if D > native.GUMBEL_MAX_DIM or M == 0 or (codes_resident and not native.gumbel_codes_supported(H, M, K, D)):
        return None
    cb = cb.contiguous()
    if g.stride(-1) != 1 and g.shape[-1] != 1:
        g = g.contiguous()
    return cb, g, native.pack_codebooks(cb, metric)


_backend = _NativeBackend


def set_backend(backend) -> None:
    """Install a different backend object exposing ``quantize`` / ``similarities`` / ``softmax_stats`` (used by the
    CPU-only host-logic tests)."""
    global _backend
    _backend = backend if backend is not None else _NativeBackend


def get_backend():
    return _backend


# ------------------------------------------------------------------------------------------------
# the rotation trick (Fifty et al., arXiv 2410.06424, section 4.2): the gradient of the quantize step with respect to x
# ------------------------------------------------------------------------------------------------
ROTATE_EPS = 1e-6


def _rotate_stage(r, c, g):
    """One stage's rotation term lam (g - 2 (g.w) w + 2 (g.qh) u) for rows r, their codes c and the incoming gradient g
    (all [..., D]); the formula is stated in include/vq_mi355x.h (vq_rotate_backward_f32)."""
    nc = c.norm(dim=-1, keepdim=True)
    a, b = r.norm(dim=-1, keepdim=True).clamp(min=ROTATE_EPS), nc.clamp(min=ROTATE_EPS)
    u, qh = r / a, c / b
    s = u + qh
    w = s / s.norm(dim=-1, keepdim=True).clamp(min=ROTATE_EPS)
    return (nc / a) * (g - 2.0 * (g * w).sum(dim=-1, keepdim=True) * w + 2.0 * (g * qh).sum(dim=-1, keepdim=True) * u)


def rotate_backward_rows(x, cb, idx, grad_out, grad_sq_err, *, ste=True, share=False, sq_err_per_head=False):
    """grad_x [H, M, D] of the quantize step under the rotation trick: x [H, M, D], cb [H, Q | 1, K, D], idx [H, M, Q],
    grad_out [H, M, D] | None, grad_sq_err [Q] ([H, Q] with ``sq_err_per_head``) | None.  One native pass
    (``rotate_backward``) where the backend has it; the same formulas in torch, stage by stage, for rows wider than the
    kernel holds, for a backend without the entry and with VQ_ROTATE_NO_FUSED=1 in the environment (read per call: A/B
    timing, and tests that compare the two paths in one process).  Neither path waits for the device."""
    fused = getattr(_backend, "rotate_backward", None)
    if fused is not None and os.environ.get("VQ_ROTATE_NO_FUSED") != "1":
        gx = fused(x, cb, idx, grad_out, grad_sq_err, ste=ste, share=share,
                   **({"sq_err_per_head": True} if sq_err_per_head else {}))
        if gx is not None:
            return gx
    H, M, D = x.shape
    gx = torch.zeros((H, M, D), dtype=x.dtype, device=x.device)
    harange = torch.arange(H, device=x.device)[:, None]
    r = x
    for q in range(idx.shape[-1]):
        c = cb[:, 0 if share else q][harange, idx[..., q]]  # [H, M, D]
        if grad_out is not None:
            gx = gx + _rotate_stage(r, c, grad_out)
        if grad_sq_err is not None:
            w = (grad_sq_err[:, q, None, None] if sq_err_per_head else grad_sq_err[q]).to(x.dtype)
            gx = gx + 2.0 * w * (r - c)
        r = r - (r + (c - r) if ste else c)
    return gx


class _RotateSteFn(torch.autograd.Function):
    """x + (picked - x) as the straight-through output computes it, with the rotation trick's gradient for x; ``picked``
    (the selected code of every row, [H, M, D]) receives none.  For the callers that gather the codes themselves (sampled
    codes, masked rows); the fused launches take ``quantize_rows(rotate=True)``."""

    @staticmethod
    def forward(ctx, x, picked):
        picked = picked.detach()
        ctx.save_for_backward(x, picked)
        return x + (picked - x)

    @staticmethod
    def backward(ctx, g):
        x, picked = ctx.saved_tensors
        H, M, _ = x.shape
        # every row's code is row m of ``picked``: a one-stage call whose codebook is the gathered rows themselves
        own = torch.arange(M, device=x.device)[None, :, None].expand(H, M, 1)
        return rotate_backward_rows(x.detach(), picked[:, None].contiguous(), own, g, None), None


def rotate_ste(x: torch.Tensor, picked: torch.Tensor) -> torch.Tensor:
    """The straight-through output x + (picked - x).detach() [H, M, D] with the rotation trick's gradient (fp32 rows)."""
    return _RotateSteFn.apply(x, picked)


class _QuantizeFn(torch.autograd.Function):
    """Autograd wrapper.  The native op has no backward of its own; the gradients are the reference's:

    * train (ste): out_q = r_q + (c_q - r_q).detach()  -> d out / d x = Q * I   (residual_vq.py:232-233,
      vector_quantize_pytorch.py:273: every stage's residual is x minus detached terms)
    * sq_err_q = sum (c_q.detach() - r_q)^2              -> d / d x = 2 (r_q - c_q)
    * a learnable codebook receives  2 (c_q - r_q)  from sq_err when ``codebook_grad_from_err``
      (commitment loss not detached, vector_quantize_pytorch.py:263-269) and, in eval, the scatter of
      grad_out (out = codebook[idx]).
    * ``rotate`` (the rotation trick; train only): the forward is the same launch, and the gradient of x is
      ``rotate_backward_rows``' -- the output passes lam (g - 2 (g.w) w + 2 (g.qh) u) per stage instead of g; the codebook's
      gradient is unchanged (the commitment-loss term only).
    """

    @staticmethod
    def forward(ctx, x, cb, metric, ste, want_sq_err, share, codebook_grad_from_err, out_buf, idx_buf, want_lse=False,
                per_head=False, packed=None, rotate=False):
        extra = {}
        if want_lse:
            extra["want_lse"] = True
        if per_head:
            extra["sq_err_per_head"] = True
        if packed is not None:
            extra["packed"] = packed
        res = _backend.quantize(x.detach(), cb.detach(), metric=metric, ste=ste, want_sq_err=want_sq_err, share=share,
                                out=out_buf, idx=idx_buf, **extra)
        out, idx, best, sq_err = res[:4]
        ctx.save_for_backward(x, cb, idx)
        ctx.ste, ctx.share, ctx.cb_err, ctx.per_head, ctx.rotate = ste, share, codebook_grad_from_err, per_head, rotate
        if sq_err is None:
            sq_err = torch.zeros((x.shape[0], idx.shape[-1]) if per_head else idx.shape[-1], dtype=torch.float64,
                                 device=x.device)
        if want_lse:
            ctx.mark_non_differentiable(idx, best, res[4])
            return out, idx, sq_err, best, res[4]
        ctx.mark_non_differentiable(idx)
        return out, idx, sq_err

    @staticmethod
    def backward(ctx, g_out, _g_idx, g_err, *_unused):
        x, cb, idx = ctx.saved_tensors
        H, M, D = x.shape
        Q = idx.shape[-1]
        gx = gcb = None
        need_x = ctx.needs_input_grad[0]
        need_cb = ctx.needs_input_grad[1]
        if getattr(ctx, "rotate", False) and need_x:
            gx = rotate_backward_rows(x.detach(), cb.detach(), idx, g_out, g_err, ste=ctx.ste, share=ctx.share,
                                      sq_err_per_head=ctx.per_head)
            if not need_cb:
                return gx, None, None, None, None, None, None, None, None, None, None, None, None
            need_x = False  # (the loop below then makes the codebook's gradient only)
        fused = getattr(_backend, "quantize_backward", None)
        if fused is not None and need_x and not need_cb:
            # one pass over x / grad_out; no host synchronisation (the torch path below inspects g_err on the host)
            return (fused(x.detach(), cb.detach(), idx, g_out if ctx.ste else None, g_err, ste=ctx.ste, share=ctx.share,
                          **({"sq_err_per_head": True} if ctx.per_head else {})),
                    None, None, None, None, None, None, None, None, None, None, None, None)
        if need_x:
            gx = g_out * float(Q) if ctx.ste else torch.zeros_like(x)
        if need_cb:
            gcb = torch.zeros_like(cb)
        has_err = g_err is not None and bool((g_err != 0).any())
        if (need_x and has_err) or need_cb:
            r = x.detach()
            harange = torch.arange(H, device=x.device)[:, None]
            for q in range(Q):
                cq = cb[:, 0 if ctx.share else q].detach()  # [H, K, D]
                i = idx[..., q]
                c = cq[harange, i]  # [H, M, D]
                if has_err:
                    w = (g_err[:, q, None, None] if ctx.per_head else g_err[q]).to(x.dtype)
                    if need_x:
                        gx = gx + 2.0 * w * (r - c)
                    if need_cb and ctx.cb_err:
                        gcb[:, 0 if ctx.share else q].index_put_((harange.expand_as(i), i), 2.0 * w * (c - r),
                                                                 accumulate=True)
                if need_cb and not ctx.ste and g_out is not None:
                    gcb[:, 0 if ctx.share else q].index_put_((harange.expand_as(i), i), g_out, accumulate=True)
                quant = r + (c - r) if ctx.ste else c
                r = r - quant
        return gx, gcb, None, None, None, None, None, None, None, None, None, None, None


def quantize_rows(x: torch.Tensor, cb: torch.Tensor, *, metric: int = EUCLID, ste: bool = False,
                  want_sq_err: bool = False, share: bool = False, codebook_grad_from_err: bool = False,
                  out: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None, want_lse: bool = False,
                  sq_err_per_head: bool = False, packed: Optional[torch.Tensor] = None,
                  screen: Optional[torch.Tensor] = None, rotate: bool = False):
    """x [H, M, D] (strided rows allowed), cb [H, Q, K, D] contiguous ([H, 1, K, D] when ``share``; the number
    of stages is then ``idx.shape[-1]``).  ``out`` / ``idx`` may be pre-allocated (strided) destination views.

    Returns (out [H, M, D], idx [H, M, Q] int64, sq_err [Q] float64 or None); with ``want_lse`` (single stage) a fourth
    element: dict(best [H, M, 1], lse [H, M]) -- the winner's distance / similarity and the log-sum-exp of the row's
    similarities, both from the same sweep (what the cross-entropy commitment loss needs).
    ``sq_err_per_head``: sq_err is [H, Q] (one sum per head: GroupedResidualVQ reports a loss per group).
    ``packed``: a cached packed image of ``cb`` from ``get_backend().pack`` (backends with ``uses_packed``); without it
    the native backend packs on every call.
    ``screen``: the cached screen image that goes with ``packed`` (``get_backend().pack_screen``); only a call that needs no
    gradient uses it.
    ``rotate``: the rotation trick -- with ``ste``, x receives the rotated and rescaled gradient of the output instead of
    the straight-through one (``rotate_backward_rows``); everything the forward returns is unchanged.
    """
    assert ste or not rotate, "the rotation trick replaces the straight-through gradient: it needs ste"
    if packed is not None and not getattr(_backend, "uses_packed", False):
        packed = None
    if packed is None or not hasattr(_backend, "pack_screen"):
        screen = None
    if not cb.is_contiguous():
        cb = cb.contiguous()
    # x receives a gradient only through the straight-through output or the squared error: an eval-mode gather
    # (out = codebook[idx]) is not differentiable with respect to x, exactly like the reference's batched_embedding
    needs_grad = torch.is_grad_enabled() and ((x.requires_grad and (ste or want_sq_err)) or cb.requires_grad)
    if x.dtype != torch.float32:
        half_rows = (x.dtype in (torch.float16, torch.bfloat16) and getattr(_backend, "accepts_half_rows", False)
                     and not needs_grad and not ste and not want_sq_err and not want_lse and cb.shape[1] == 1
                     and (idx is None or idx.shape[-1] == 1))
        if not half_rows:
            x = x.float()  # the reference's x.float() (codebooks.py:354); the native inference launch does it in-kernel
    if needs_grad:
        res = _QuantizeFn.apply(x, cb, metric, ste, want_sq_err, share, codebook_grad_from_err, out, idx, want_lse,
                                sq_err_per_head, packed, rotate)
        out, idx, sq_err = res[:3]
        if want_lse:
            return out, idx, (sq_err if want_sq_err else None), dict(best=res[3], lse=res[4])
        return out, idx, (sq_err if want_sq_err else None)
    pk = {"packed": packed} if packed is not None else {}
    if screen is not None:
        pk["screen"] = screen
    if want_lse:
        out, idx, best, sq_err, lse = _backend.quantize(x, cb, metric=metric, ste=ste, want_sq_err=want_sq_err,
                                                        share=share, out=out, idx=idx, want_lse=True, **pk)
        return out, idx, sq_err, dict(best=best, lse=lse)
    out, idx, _best, sq_err = _backend.quantize(x, cb, metric=metric, ste=ste, want_sq_err=want_sq_err, share=share,
                                                out=out, idx=idx, **pk,
                                                **({"sq_err_per_head": True} if sq_err_per_head else {}))
    return out, idx, sq_err


# ------------------------------------------------------------------------------------------------
# residual stacks with a mask: the fused search on all rows, then the mask pass
# ------------------------------------------------------------------------------------------------
def masked_backend():
    """The backend when the fused masked residual forward exists and is not switched off (VQ_RVQ_NO_FUSED_MASK=1 in the
    environment, read per call like VQ_NO_FUSED_DECODE), else None: the caller walks its layers."""
    if os.environ.get("VQ_RVQ_NO_FUSED_MASK") == "1" or not hasattr(_backend, "residual_mask"):
        return None
    return _backend


def zero_row_indices(cb: torch.Tensor, *, metric: int, packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cb [G, Qc, K, D] -> [G, Qc] int64: every stage codebook's answer to the all-zero row, from the search kernel itself (the
    stage codebooks on the head axis against one zero row each): its metric, its first-index rule, its NaN-code rule."""
    G, Qc, K, D = cb.shape
    heads = cb.reshape(G * Qc, 1, K, D)
    zeros = torch.zeros((G * Qc, 1, D), dtype=torch.float32, device=cb.device)
    pk = {"packed": packed} if (packed is not None and getattr(_backend, "uses_packed", False)) else {}
    _out, idx, _best, _err = _backend.quantize(zeros, heads, metric=metric, ste=False, want_sq_err=False, share=False, **pk)
    return idx.reshape(G, Qc)


class _MaskedQuantizeFn(torch.autograd.Function):
    """_QuantizeFn for a residual stack with a row mask: the fused search on every row, then the mask pass.  Gradients (the
    reference's, for a stack whose codebooks do not learn): every layer returns its INPUT on a masked-out row
    (vector_quantize_pytorch.py:415-418) and r_q + (c_q - r_q).detach() on a kept one, each residual being x minus detached
    terms, so in train mode d out / d x = Q * I on every row; sq_err_q sums over the kept rows only."""

    @staticmethod
    def forward(ctx, x, cb, mask, zero_idx, metric, ste, want_sq_err, share, out_buf, idx_buf, per_head, packed):
        extra = {"packed": packed} if packed is not None else {}
        xd, cbd = x.detach(), cb.detach()
        # (the search writes its own ``out`` first; the mask pass then rewrites all of it)
        out, idx = _backend.quantize(xd, cbd, metric=metric, ste=ste, want_sq_err=False, share=share, out=out_buf, idx=idx_buf,
                                     **extra)[:2]
        out, sq_err = _backend.residual_mask(xd, cbd, idx, mask, zero_idx, train=ste, want_sq_err=want_sq_err,
                                             per_group=per_head, out=out)
        ctx.save_for_backward(x, cb, idx, mask)
        ctx.ste, ctx.want_sq_err, ctx.per_head = ste, want_sq_err, per_head
        if sq_err is None:
            sq_err = torch.zeros((x.shape[0], idx.shape[-1]) if per_head else idx.shape[-1], dtype=torch.float64, device=x.device)
        ctx.mark_non_differentiable(idx)
        return out, idx, sq_err

    @staticmethod
    def backward(ctx, g_out, _g_idx, g_err):
        x, cb, idx, mask = ctx.saved_tensors
        gx = None
        if ctx.needs_input_grad[0]:
            gx = _backend.residual_mask_backward(x.detach(), cb.detach(), idx, mask, g_out if ctx.ste else None,
                                                 g_err if ctx.want_sq_err else None, train=ctx.ste, per_group=ctx.per_head)
        return gx, None, None, None, None, None, None, None, None, None, None, None


def quantize_rows_masked(x: torch.Tensor, cb: torch.Tensor, mask: torch.Tensor, zero_idx: torch.Tensor, *, metric: int = EUCLID,
                         ste: bool = False, want_sq_err: bool = False, share: bool = False, out: Optional[torch.Tensor] = None,
                         idx: Optional[torch.Tensor] = None, sq_err_per_head: bool = False,
                         packed: Optional[torch.Tensor] = None):
    """``quantize_rows`` for a residual stack with a row mask: x [H, M, D] fp32, cb [H, Q | 1, K, D] (not learnable), mask [M]
    or [H, M] (True = kept), zero_idx [H, Q] (``zero_row_indices``) -> (out, idx, sq_err over the kept rows | None)."""
    if packed is not None and not getattr(_backend, "uses_packed", False):
        packed = None
    if not cb.is_contiguous():
        cb = cb.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    if torch.is_grad_enabled() and x.requires_grad and (ste or want_sq_err):
        out, idx, sq_err = _MaskedQuantizeFn.apply(x, cb, mask, zero_idx, metric, ste, want_sq_err, share, out, idx,
                                                   sq_err_per_head, packed)
        return out, idx, (sq_err if want_sq_err else None)
    extra = {"packed": packed} if packed is not None else {}
    out, idx = _backend.quantize(x, cb, metric=metric, ste=ste, want_sq_err=False, share=share, out=out, idx=idx, **extra)[:2]
    out, sq_err = _backend.residual_mask(x, cb, idx, mask, zero_idx, train=ste, want_sq_err=want_sq_err,
                                         per_group=sq_err_per_head, out=out)
    return out, idx, sq_err


# ------------------------------------------------------------------------------------------------
# indices -> code vectors
# ------------------------------------------------------------------------------------------------
def decode_backend(cb: torch.Tensor, indices) -> Optional[object]:
    """The backend's ``decode`` when the fused decode takes this call, else None (the caller keeps its tensor-op
    expression): a backend that has one, device tensors, fp32 codes, int32 / int64 indices, and no VQ_NO_FUSED_DECODE=1 in
    the environment (read per call: A/B timing, and tests that compare the two paths in one process)."""
    fn = getattr(_backend, "decode", None)
    if fn is None or os.environ.get("VQ_NO_FUSED_DECODE") == "1":
        return None
    if not (isinstance(indices, torch.Tensor) and cb.is_cuda and indices.is_cuda and cb.dtype == torch.float32
            and indices.dtype in (torch.int32, torch.int64)):
        return None
    return fn


def lfq_decode_backend(indices, num_stages: int = 1) -> Optional[object]:
    """The backend's ``lfq_decode`` when the fused decode of the lookup-free family takes this call, else None (the caller
    keeps its tensor-op expression): the rule of ``decode_backend`` -- a backend that has one, device int32 / int64 indices,
    no VQ_NO_FUSED_DECODE=1 in the environment (read per call) -- and a stack the kernel's argument block holds."""
    fn = getattr(_backend, "lfq_decode", None)
    if fn is None or os.environ.get("VQ_NO_FUSED_DECODE") == "1":
        return None
    if not (isinstance(indices, torch.Tensor) and indices.is_cuda and indices.dtype in (torch.int32, torch.int64)
            and num_stages <= native.RLFQ_MAX_STAGES):
        return None
    return fn


def decode_grad_codes(cb_shape, indices, drop_null, g_sum, g_all):
    """d/d cb of the decode: every stage scatter-adds its incoming gradient by index (g_sum reaches every stage, g_all[q]
    stage q), dropped and out-of-range entries masked out, the wrap rule applied first.  One ``ema_accumulate`` per stage."""
    Gc, Qc, K, D = cb_shape
    G, N, Qg = indices.shape
    ref = g_sum if g_sum is not None else g_all
    gcb = torch.zeros(cb_shape, dtype=torch.float32, device=ref.device)
    for q in range(Qg):
        g = g_sum if g_all is None else (g_all[q] if g_sum is None else g_sum + g_all[q])
        i = indices[..., q].to(torch.int64)
        if not drop_null:
            i = torch.where(i < 0, i + K, i)
        valid = (i >= 0) & (i < K)
        i = torch.where(valid, i, torch.zeros_like(i))
        g = g.to(torch.float32).contiguous()
        if Gc == 1 and G > 1:  # one table for all groups: their rows are one list
            g, i, valid = g.reshape(1, G * N, D), i.reshape(1, G * N), valid.reshape(1, G * N)
        _hits, sums = _backend.ema_accumulate(g, i.contiguous(), K, valid)
        gcb[:, q if Qc > 1 else 0] += sums
    return gcb


class _DecodeFn(torch.autograd.Function):
    """The fused decode with the gradient of the tensor-op expression it replaces: out = codebook[idx] is differentiable
    with respect to a learnable codebook (a scatter-add of the incoming gradient by index); indices receive none."""

    @staticmethod
    def forward(ctx, cb, indices, num_stages, drop_null, want_sum, want_all):
        s, a = _backend.decode(cb.detach(), indices, num_stages=num_stages, drop_null=drop_null, want_sum=want_sum,
                               want_all=want_all)
        ctx.save_for_backward(indices)
        ctx.cb_shape, ctx.drop_null = tuple(cb.shape), drop_null
        return s, a

    @staticmethod
    def backward(ctx, g_sum, g_all):
        (indices,) = ctx.saved_tensors
        return decode_grad_codes(ctx.cb_shape, indices, ctx.drop_null, g_sum, g_all), None, None, None, None, None


def decode_rows(decode, cb: torch.Tensor, indices: torch.Tensor, *, num_stages: Optional[int] = None, drop_null: bool = True,
                want_sum: bool = True, want_all: bool = False, sum_out: Optional[torch.Tensor] = None,
                all_out: Optional[torch.Tensor] = None):
    """``decode`` (from ``decode_backend``) on cb [G | 1, Q | 1, K, D] and indices [G, N, Qg] ->
    (codes_sum [G, N, D] | None, all_codes [Q, G, N, D] | None).  A codebook that requires grad keeps its autograd edge
    (the results are then fresh tensors: ``sum_out`` / ``all_out`` must not be given -- see ``decode_needs_grad``)."""
    if decode_needs_grad(cb):
        assert sum_out is None and all_out is None
        return _DecodeFn.apply(cb, indices, num_stages, drop_null, want_sum, want_all)
    return decode(cb.detach(), indices, num_stages=num_stages, drop_null=drop_null, want_sum=want_sum, want_all=want_all,
                  sum_out=sum_out, all_out=all_out)


def decode_needs_grad(cb: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and cb.requires_grad


def nearest_with_distance(x: torch.Tensor, cb: torch.Tensor, *, metric: int = EUCLID):
    """Search only: (idx [H, M], best [H, M]) -- used by k-means seeding and diagnostics."""
    out, idx, best, _ = _backend.quantize(x.float(), cb[:, None].contiguous(), metric=metric, ste=False,
                                          want_sq_err=False, share=False, want_best=True)
    return idx[..., 0], best[..., 0], out
