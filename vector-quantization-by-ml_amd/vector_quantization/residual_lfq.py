"""Residual lookup-free quantization: the reference's ``ResidualLFQ`` and ``GroupedResidualLFQ``
(``vector_quantization/residual_lfq.py``), a stack of ``LFQ`` layers whose stage q quantizes what the stages before it left
over, with codebook scale 2^-q.

Fused path (the hot path).  After ``project_in``, every stage's quantize step is one HIP pass (``vq_rlfq_quantize_f32``:
one thread per row, the row's d <= 20 values held in registers across the stages), every stage's entropy terms one
stage-batched call (``vq_lfq_entropy_staged_{fwd,bwd}_f32``, each stage bitwise a single-stage LFQ call), and dL/dx one
per-row pass (``vq_rlfq_backward_f32``) that sums the stages' terms.  ``GroupedResidualLFQ`` runs its G groups as the
kernels' group axis: G groups x Q stages are still one launch each.  The loss arithmetic around the kernels is vectorised
over stages (and groups), and ``maybe_distributed_mean`` is one collective over all stages' ``avg_prob``.

Fallback path.  A stage-by-stage loop over the module's own ``LFQ`` layers, line for line the reference's ``forward``.  It
serves configurations the fused kernels do not cover: a straight-through activation other than ``nn.Identity``, more than
``MAX_FUSED_STAGES`` active stages, ``channel_first`` / several codebooks per layer, ``accept_image_fmap`` groups.

Both paths run only on the GPU: CPU tensors raise ``native.NativeUnavailable`` (``codebooks`` is pure torch and works
anywhere).  DESIGN.md section 11 states the accuracy contract between the two paths and against the reference.

Decode side.  ``get_codes_from_indices`` and ``get_output_from_indices`` of device indices are one HIP pass
(``vq_lfq_decode_f32``: every stage's code from its index bits, the stage-ordered sum, dropped stages as +0.0), for
``GroupedResidualLFQ`` one pass over all groups with the sum written into the concatenated result.  CPU indices,
``VQ_NO_FUSED_DECODE=1`` and stacks deeper than ``MAX_FUSED_STAGES`` keep the tensor-op expressions, which work anywhere
(DESIGN.md section 18).
"""
from __future__ import annotations

import random
from math import log2, prod

import torch
import torch.nn.functional as F
from torch import nn

from . import native, search
from .lookup_free_quantization import _EPS, LFQ, _entropy, _maybe_distributed_mean
from .residual_common import (check_coarse, dropout_cut, group_rows_in, group_rows_out, grouped_decode_dest, grouped_decode_rows,
                              grouped_fallback, pad_stages, rows_contiguous)

MAX_FUSED_STAGES = native.RLFQ_MAX_STAGES
_ENTROPY_WS_BUDGET = 2 << 30  # bytes of staged-entropy workspace per call; more stages than fit run in several calls
_INV_TEMPERATURE = 100.0  # ResidualLFQ.forward passes none to its layers: LFQ's default


def _compiling() -> bool:
    return torch.compiler.is_compiling()


def _staged_entropy_fwd(v: torch.Tensor, rows, scales, tau):
    """native.lfq_entropy_staged_forward over v [T, N, d], in as few calls as the workspace budget allows."""
    T, N, d = v.shape
    R = N if rows is None else int(rows.shape[-1])
    per_stage = int(native.load().vq_lfq_staged_workspace_bytes(max(R, 1), 1, d))
    chunk = max(1, _ENTROPY_WS_BUDGET // max(per_stage, 1))
    if T <= chunk:
        return native.lfq_entropy_staged_forward(v, rows, scales, tau)
    ps, avg = [], []
    S = len(scales)
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        r = rows[t0:t1] if rows is not None and rows.dim() == 2 else rows
        p, a = native.lfq_entropy_staged_forward(v[t0:t1], r, [scales[(t0 + j) % S] for j in range(S)], tau)
        ps.append(p)
        avg.append(a)
    return torch.cat(ps), torch.cat(avg)


def _staged_entropy_bwd(v: torch.Tensor, rows, scales, tau, w_ps, w_cb):
    T, N, d = v.shape
    R = N if rows is None else int(rows.shape[-1])
    per_stage = int(native.load().vq_lfq_staged_workspace_bytes(max(R, 1), 1, d))
    chunk = max(1, _ENTROPY_WS_BUDGET // max(per_stage, 1))
    if T <= chunk:
        return native.lfq_entropy_staged_backward(v, rows, scales, tau, w_ps, w_cb)
    S = len(scales)
    parts = []
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        r = rows[t0:t1] if rows is not None and rows.dim() == 2 else rows
        parts.append(native.lfq_entropy_staged_backward(v[t0:t1], r, [scales[(t0 + j) % S] for j in range(S)], tau,
                                                        w_ps[t0:t1], w_cb[t0:t1]))
    return torch.cat(parts)


class _RlfqTrain(torch.autograd.Function):
    """x [G, N, d] (the stage-0 residual of every group) -> out [G, N, d] (sum of the stages' straight-through values),
    idx [G, N, S], commitment squared-error sums [G, S] (float64), per-sample entropies [G, S], codebook entropies [G, S]."""

    @staticmethod
    def forward(ctx, x, mask, rows, qmag, clamp, scale, spherical, want_commit):
        G, N, d = x.shape
        S = len(qmag)
        out, idx, v_all, commit = native.rlfq_quantize(x.detach(), qmag, clamp, scale, spherical=spherical, ste=True,
                                                       mask=mask, want_v=True, want_commit=want_commit)
        if commit is None:
            commit = torch.zeros((G, S), dtype=torch.float64, device=x.device)
        v_flat = v_all.view(G * S, N, d)
        R = N if rows is None else int(rows.shape[-1])
        ps_sum, avg = _staged_entropy_fwd(v_flat, rows, qmag, _INV_TEMPERATURE)
        avg, world = _maybe_distributed_mean(avg)  # one collective for every stage: elementwise the per-stage ones
        per_sample = (ps_sum / R).to(torch.float32).view(G, S)
        codebook = _entropy(avg).view(G, S)
        ctx.save_for_backward(x, v_all, avg, mask if mask is not None else torch.empty(0),
                              rows if rows is not None else torch.empty(0))
        ctx.meta = (mask is not None, rows is not None, R, world, qmag, clamp, scale, spherical, want_commit)
        ctx.mark_non_differentiable(idx)
        return out, idx, commit, per_sample, codebook

    @staticmethod
    def backward(ctx, g_out, g_idx, g_commit, g_ps, g_cb):
        x, v_all, avg, mask, rows = ctx.saved_tensors
        has_mask, has_rows, R, world, qmag, clamp, scale, spherical, want_commit = ctx.meta
        mask = mask if has_mask else None
        rows = rows if has_rows else None
        G, S, N, d = v_all.shape
        dev = x.device
        g_ps = torch.zeros((G, S), device=dev) if g_ps is None else g_ps
        g_cb = torch.zeros((G, S), device=dev) if g_cb is None else g_cb
        w_ps = g_ps.to(torch.float32).reshape(G * S) / R
        # d/dx of -x log(max(x, eps)): -(log x + 1) above the clamp, -log eps below it (as LFQ's backward)
        dh = -(avg.clamp(min=_EPS).log() + (avg >= _EPS).to(avg.dtype))
        w_cb = dh * (g_cb.to(torch.float32).reshape(G * S, 1) / (R * world))
        g_ent = _staged_entropy_bwd(v_all.view(G * S, N, d), rows, qmag, _INV_TEMPERATURE, w_ps, w_cb).view(G, S, N, d)
        w_commit = None
        if want_commit and g_commit is not None:
            w_commit = 2.0 * g_commit.to(torch.float32)
        gx = native.rlfq_backward(x.detach(), qmag, clamp, scale, spherical=spherical, mask=mask, g_out=g_out,
                                  w_commit=w_commit, g_ent=g_ent)
        return gx, None, None, None, None, None, None, None


def _fused_ok(rvq: "ResidualLFQ", x: torch.Tensor, stages: int) -> bool:
    l0 = rvq.layers[0]
    return ((x.is_cuda or _compiling()) and 1 <= stages <= MAX_FUSED_STAGES
            and all(type(layer.activation) is nn.Identity for layer in rvq.layers)
            and not l0.channel_first and l0.num_codebooks == 1 and not l0.keep_num_codebooks_dim and not l0.has_projections)


def _fused_forward(rvqs, xg: torch.Tensor, mask, stages: int):
    """The fused path of G residual stacks with identical configurations: xg [G, N, d] (fp32, rows contiguous) ->
    (out [G, N, d], idx [G, N, stages], losses [G, stages])."""
    rvq = rvqs[0]
    layers = rvq.layers[:stages]
    l0 = layers[0]
    G, N, d = xg.shape
    qmag = [layer._code_mag for layer in layers]
    clamp = [float(layer.soft_clamp_input_value or 0.0) for layer in layers]
    scale = [float(layer.codebook_scale) for layer in layers]
    if mask is not None:
        mask = mask.reshape(N).to(xg.device)
    if not rvq.training:
        if _compiling():
            out, idx, _, _ = torch.ops.vq_mi355x.rlfq_quantize(xg, qmag, clamp, scale, l0.spherical, False, None, False, False)
        else:
            out, idx, _, _ = native.rlfq_quantize(xg.detach(), qmag, clamp, scale, spherical=l0.spherical, ste=False)
        return out, idx, torch.zeros((G, stages), dtype=torch.float32, device=xg.device)

    # entropy rows.  Without frac_per_sample_entropy every stage uses the mask's rows (or all rows): one selection.  With
    # it, each (group, stage) draws in the reference's order: group-major, then stage (LFQ._entropy_rows per layer).
    if l0.frac_per_sample_entropy >= 1.0:
        rows = l0._entropy_rows(N, mask, xg.device)
    else:
        rows = torch.stack([r.layers[s]._entropy_rows(N, mask, xg.device) for r in rvqs for s in range(stages)])
    want_commit = l0.commitment_loss_weight > 0.0
    out, idx, commit_sum, per_sample, codebook = _RlfqTrain.apply(xg, mask, rows, qmag, clamp, scale, l0.spherical,
                                                                   want_commit)
    entropy_aux = per_sample - l0.diversity_gamma * codebook
    if l0.experimental_softplus_entropy_loss:
        entropy_aux = F.softplus(entropy_aux + l0.entropy_loss_offset)
    if want_commit:
        kept = N if mask is None else mask.sum()
        commit_loss = (commit_sum / (kept * d)).to(torch.float32)
    else:
        commit_loss = torch.zeros((G, stages), dtype=torch.float32, device=xg.device)
    losses = entropy_aux * l0.entropy_loss_weight + commit_loss * l0.commitment_loss_weight
    return out, idx, losses


class ResidualLFQ(nn.Module):
    """Follows Algorithm 1. in https://arxiv.org/pdf/2107.03312.pdf"""

    def __init__(
        self,
        *,
        dim,
        num_quantizers,
        codebook_size,
        quantize_dropout=False,
        quantize_dropout_cutoff_index=0,
        quantize_dropout_multiple_of=1,
        soft_clamp_input_value=None,
        **kwargs,
    ):
        super().__init__()
        codebook_dim = int(log2(codebook_size))

        requires_projection = codebook_dim != dim
        self.project_in = nn.Linear(dim, codebook_dim) if requires_projection else nn.Identity()
        self.project_out = nn.Linear(codebook_dim, dim) if requires_projection else nn.Identity()
        self.has_projections = requires_projection

        self.num_quantizers = num_quantizers
        self.codebook_dim = codebook_dim

        self.layers = nn.ModuleList([])
        for ind in range(num_quantizers):
            codebook_scale = 2**-ind
            lfq = LFQ(dim=codebook_dim, codebook_scale=codebook_scale, soft_clamp_input_value=soft_clamp_input_value, **kwargs)
            self.layers.append(lfq)
            if soft_clamp_input_value is not None:
                soft_clamp_input_value *= 0.5

        assert all([not lfq.has_projections for lfq in self.layers])
        # one code magnitude per stage, as bits_to_codes gives it (unnormalised: +-codebook_scale), for the fused decode
        self._stage_mags = tuple(float(lfq.codebook_scale) for lfq in self.layers)

        self.quantize_dropout = quantize_dropout and num_quantizers > 1
        assert quantize_dropout_cutoff_index >= 0
        self.quantize_dropout_cutoff_index = quantize_dropout_cutoff_index
        self.quantize_dropout_multiple_of = quantize_dropout_multiple_of

    @property
    def codebooks(self):
        return torch.stack([layer.codebook for layer in self.layers], dim=0)

    def _decode(self, decode, indices, want_sum, want_all):
        """The fused decode (vq_lfq_decode_f32) of indices [b, ..., q]: (sum [b, ..., d] | None, all [Q, b, ..., d] | None)."""
        lead = indices.shape[:-1]
        flat = indices.reshape(1, prod(lead), indices.shape[-1])
        s, a = decode(flat, self._stage_mags, self.codebook_dim, drop_null=True, want_sum=want_sum, want_all=want_all)
        if s is not None:
            s = s.reshape(*lead, self.codebook_dim)
        if a is not None:
            a = a.reshape(self.num_quantizers, *lead, self.codebook_dim)
        return s, a

    def get_codes_from_indices(self, indices):
        """indices [b, ..., q] (q <= num_quantizers; -1 = dropped) -> codes [num_quantizers, b, ..., codebook_dim], the
        unnormalised codes (bits_to_codes) of each stage, zero where dropped.  Computed from the index bits."""
        quantize_dim = indices.shape[-1]
        decode = search.lfq_decode_backend(indices, self.num_quantizers)
        check_coarse(self, quantize_dim)
        if decode is not None:
            return self._decode(decode, indices, False, True)[1]
        lead = indices.shape[:-1]
        indices = indices.reshape(lead[0] if len(lead) else 1, -1, quantize_dim)
        if quantize_dim < self.num_quantizers:
            indices = F.pad(indices, (0, self.num_quantizers - quantize_dim), value=-1)
        dropped = indices == -1
        indices = indices.masked_fill(dropped, 0)
        codes = []
        for q, layer in enumerate(self.layers):
            bits = ((indices[..., q, None].int() & layer.mask) != 0).to(torch.float32)
            codes.append(layer.bits_to_codes(bits))
        all_codes = torch.stack(codes)  # [q, b, n, d]
        all_codes = all_codes.masked_fill(dropped.permute(2, 0, 1)[..., None], 0.0)
        return all_codes.reshape(self.num_quantizers, *lead, all_codes.shape[-1])

    def get_output_from_indices(self, indices):
        decode = search.lfq_decode_backend(indices, self.num_quantizers)
        if decode is not None:
            check_coarse(self, indices.shape[-1])
            return self.project_out(self._decode(decode, indices, True, False)[0])
        codes = self.get_codes_from_indices(indices)
        return self.project_out(codes.sum(dim=0))

    def _dropout_cut(self, seed):
        """The last active stage under quantize dropout (None: every stage runs), consuming `random` as the reference."""
        if not (self.training and self.quantize_dropout):
            return None
        return dropout_cut(self.quantize_dropout_cutoff_index, self.num_quantizers, self.quantize_dropout_multiple_of, seed)

    def forward(self, x, mask=None, return_all_codes=False, rand_quantize_dropout_fixed_seed=None):
        num_quant = self.num_quantizers
        x = self.project_in(x)
        cut = self._dropout_cut(rand_quantize_dropout_fixed_seed)
        stages = num_quant if cut is None else min(cut + 1, num_quant)

        if _fused_ok(self, x, stages):
            xf = x.float()
            assert xf.shape[-1] == self.codebook_dim
            xg = rows_contiguous(xf.reshape(1, -1, self.codebook_dim))
            with torch.autocast(device_type="cuda", enabled=False):
                out, idx, losses = _fused_forward([self], xg, mask, stages)
            quantized_out = self.project_out(out.reshape(xf.shape))
            all_indices, all_losses = pad_stages(idx.reshape(*xf.shape[:-1], stages), num_quant, losses[0].to(x.dtype))
        else:
            quantized_out, all_indices, all_losses = self._forward_stagewise(x, mask, cut)

        ret = (quantized_out, all_indices, all_losses)
        if not return_all_codes:
            return ret
        return (*ret, self.get_codes_from_indices(all_indices))

    def _forward_stagewise(self, x, mask, cut):
        """The fallback: the reference's loop over the LFQ layers (residual_lfq.py:128-197)."""
        quantized_out = 0.0
        residual = x
        all_losses = []
        all_indices = []
        if cut is not None:
            null_indices = torch.full(x.shape[:2], -1.0, device=x.device, dtype=torch.long)
            null_loss = torch.tensor(0.0, device=x.device, dtype=x.dtype)
        with torch.autocast(device_type="cuda", enabled=False):
            for quantizer_index, layer in enumerate(self.layers):
                if cut is not None and quantizer_index > cut:
                    all_indices.append(null_indices)
                    all_losses.append(null_loss)
                    continue
                quantized, indices, loss = layer(residual, mask=mask)
                residual = residual - quantized.detach()
                quantized_out = quantized_out + quantized
                all_indices.append(indices)
                all_losses.append(loss)
        quantized_out = self.project_out(quantized_out)
        return quantized_out, torch.stack(all_indices, dim=-1), torch.stack(all_losses, dim=-1)


class GroupedResidualLFQ(nn.Module):
    def __init__(self, *, dim, groups=1, accept_image_fmap=False, **kwargs):
        super().__init__()
        self.dim = dim
        self.groups = groups
        assert (dim % groups) == 0
        dim_per_group = dim // groups
        self.accept_image_fmap = accept_image_fmap
        self.rvqs = nn.ModuleList([])
        for _ in range(groups):
            self.rvqs.append(ResidualLFQ(dim=dim_per_group, **kwargs))
        # ONE decode launch serves every group when the stacks agree in depth, bits per index and stage scales (they do by
        # construction: every group gets the same arguments)
        rvq0 = self.rvqs[0]
        self._uniform_stacks = all(rvq.codebook_dim == rvq0.codebook_dim and rvq._stage_mags == rvq0._stage_mags
                                   for rvq in self.rvqs)

    @property
    def codebooks(self):
        return torch.stack(tuple(rvq.codebooks for rvq in self.rvqs))

    @property
    def split_dim(self):
        return 1 if self.accept_image_fmap else -1

    def _decode_backend(self, indices):
        """The fused decode when one launch serves every group: a stacked index tensor and uniform stacks."""
        if not (self._uniform_stacks and isinstance(indices, torch.Tensor) and indices.dim() >= 2
                and indices.shape[0] == self.groups):
            return None
        return search.lfq_decode_backend(indices, self.rvqs[0].num_quantizers)

    def get_codes_from_indices(self, indices):
        decode = self._decode_backend(indices)
        if decode is not None:
            rvq0 = self.rvqs[0]
            G, Q, d = self.groups, rvq0.num_quantizers, rvq0.codebook_dim
            check_coarse(rvq0, indices.shape[-1])
            flat, lead = grouped_decode_rows(indices)
            if _compiling():  # (the registered op returns fresh tensors)
                codes = decode(flat, rvq0._stage_mags, d, drop_null=True, want_sum=False, want_all=True)[1].transpose(0, 1)
                return codes.reshape(G, Q, *lead, d)
            codes, dest = grouped_decode_dest(flat, lead, d, Q)
            decode(flat, rvq0._stage_mags, d, drop_null=True, want_sum=False, want_all=True, all_out=dest)
            return codes
        codes = tuple(rvq.get_codes_from_indices(chunk_indices) for rvq, chunk_indices in zip(self.rvqs, indices))
        return torch.stack(codes)

    def get_output_from_indices(self, indices):
        decode = self._decode_backend(indices)
        if decode is not None:
            rvq0 = self.rvqs[0]
            d = rvq0.codebook_dim
            check_coarse(rvq0, indices.shape[-1])
            flat, lead = grouped_decode_rows(indices)
            mags = rvq0._stage_mags
            if self.split_dim == -1 and not rvq0.has_projections and not _compiling():
                # every group's sum lands in its columns of the concatenated result
                out, dest = grouped_decode_dest(flat, lead, d)
                decode(flat, mags, d, drop_null=True, sum_out=dest)
                return out
            sums, _ = decode(flat, mags, d, drop_null=True)
            outputs = tuple(rvq.project_out(sums[g].reshape(*lead, d)) for g, rvq in enumerate(self.rvqs))
            return torch.cat(outputs, dim=self.split_dim)
        outputs = tuple(rvq.get_output_from_indices(chunk_indices) for rvq, chunk_indices in zip(self.rvqs, indices))
        return torch.cat(outputs, dim=self.split_dim)

    def forward(self, x, mask=None, return_all_codes=False):
        shape, split_dim = x.shape, self.split_dim
        assert shape[split_dim] == self.dim
        seed = random.randint(0, int(1e7))  # drawn in eval too, as the reference does
        rvq0 = self.rvqs[0]
        cut = rvq0._dropout_cut(seed)  # every group gets the same seed, so the same cut
        Q = rvq0.num_quantizers
        stages = Q if cut is None else min(cut + 1, Q)
        if split_dim == -1 and _fused_ok(rvq0, x, stages):
            return self._forward_fused(x, mask, return_all_codes, stages)
        return grouped_fallback(self.rvqs, x, split_dim, seed, return_all_codes, tuple, mask=mask)

    def _forward_fused(self, x, mask, return_all_codes, stages):
        G = self.groups
        rvq0 = self.rvqs[0]
        Q = rvq0.num_quantizers
        lead = x.shape[:-1]
        d = rvq0.codebook_dim  # (= dim / G without projections)
        xg, loss_dtype = group_rows_in(x, self.rvqs, d, rvq0.has_projections)
        with torch.autocast(device_type="cuda", enabled=False):
            out, idx, losses = _fused_forward(list(self.rvqs), xg, mask, stages)
        quantized = group_rows_out(out, self.rvqs, lead, d, rvq0.has_projections)
        all_indices, commit_losses = pad_stages(idx.reshape(G, *lead, stages), Q, losses.to(loss_dtype))
        ret = (quantized, all_indices, commit_losses)
        if not return_all_codes:
            return ret
        return (*ret, tuple(rvq.get_codes_from_indices(all_indices[g]) for g, rvq in enumerate(self.rvqs)))
