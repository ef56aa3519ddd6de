"""``ResidualVQ`` / ``GroupedResidualVQ`` (reference: /root/reference/vector_quantization/residual_vq.py:26-357).

The reference walks its layers in Python, and every layer re-reads / re-writes the full residual and
rebuilds the ``[rows, K]`` similarity and one-hot tensors (residual_vq.py:212-243).  Here the whole stack
of stages is ONE native launch when the layers are homogeneous (the normal case): the residual rows stay
in registers across the Q codebook sweeps, the kernel writes ``indices[..., q]``, the accumulated
``quantized_out`` and the per-stage squared errors.  ``GroupedResidualVQ`` maps its groups onto the
kernel's head axis, so G groups x Q stages are still one launch.

A ``mask=`` keeps the one launch: the search runs on every row and one more native pass (the mask pass,
``search.quantize_rows_masked``) applies the reference's rule for masked-out rows to the output, the indices and
the per-stage squared errors.  Quantize dropout keeps it too: a stack cut after stage ``cut`` is the same launch
on ``cut + 1`` stages.  ``VQ_RVQ_NO_FUSED_MASK=1`` in the environment (read per call) sends both back to the loop.

Heterogeneous stacks (per-layer input normalisation, k-means seeding on the first batch, channel-first layers,
a mask together with device-side expiry) fall back to a per-layer loop in which each layer call is itself a
native launch.

The fused forward is written once: ``_fused_stack`` runs G homogeneous stacks on rows ``[G, rows, d]`` with the cached stage
codes (``_stage_codes``) -- search or masked search, EMA step, dead-code expiry -- and ``_stage_losses`` turns its squared
errors into the loss tensor.  ``ResidualVQ._forward_fused`` (one group, no destination view, one error sum per stage) and
``GroupedResidualVQ._forward_fused`` (G groups read and written in place, errors per group) are the layout around that call.
What the VQ, LFQ and FSQ stacks share beyond it -- the dropout draw, stage padding, the grouped loop over the stacks, the
grouped decode's buffers -- is ``residual_common.py``.
"""
from __future__ import annotations

import random
from typing import List

import torch
import torch.distributed as dist
from torch import nn

from . import search
from .quantizer import VectorQuantize, _cached_zeros
from .residual_common import check_coarse, dropout_cut, grouped_decode_dest, grouped_decode_rows, grouped_fallback, pad_stages


def _residual_chain(x: torch.Tensor, codes: torch.Tensor, idx: torch.Tensor, ste: bool) -> List[torch.Tensor]:
    """Per-stage residuals [r_1 .. r_Q] recomputed from the indices with the reference's fp32 operations
    (used only for training-state bookkeeping after the fused launch).  x [M, D], codes [Q, K, D], idx [M, Q]."""
    residuals = []
    r = x
    for q in range(idx.shape[-1]):
        residuals.append(r)
        c = codes[q][idx[:, q]]
        quant = r + (c - r) if ste else c
        r = r - quant
    return residuals


def _residual_chain_masked(x: torch.Tensor, codes: torch.Tensor, idx: torch.Tensor, mask: torch.Tensor) -> List[torch.Tensor]:
    """_residual_chain (train arithmetic) of a masked stack: a masked-out row's layer returns its input, so its residual is
    r_q - r_q from stage 1 on -- the rows the reference's layers hand to their dead-code re-seeding.  mask [M] bool."""
    residuals = []
    r = x
    kept = mask[:, None]
    for q in range(idx.shape[-1]):
        residuals.append(r)
        c = codes[q][idx[:, q]]
        r = r - torch.where(kept, r + (c - r), r)
    return residuals


def _zero_row_indices(owner, codes: torch.Tensor, packed, metric: int, Q: int) -> torch.Tensor:
    """[G, Q] int64: every stage codebook's answer to the all-zero row (search.zero_row_indices: one tiny launch of the real
    search), kept on ``owner`` beside its _stage_cache and rebuilt when that is."""
    key = None if torch.compiler.is_compiling() or owner._stage_cache is None else owner._stage_cache[0]
    cached = owner._zero_idx_cache
    if key is not None and cached is not None and cached[0] == key:
        return cached[1]
    with torch.no_grad():
        zero_idx = search.zero_row_indices(codes, metric=metric, packed=packed)
        if zero_idx.shape[1] != Q:  # one shared codebook: the same answer at every stage
            zero_idx = zero_idx.expand(-1, Q)
        zero_idx = zero_idx.contiguous()
    if key is not None:
        owner._zero_idx_cache = (key, zero_idx)
    return zero_idx


def _mask_fusable(layers, x, mask, groups: int = 1) -> bool:
    """A masked (or quantize-dropout) call may take the fused path: a backend with the mask pass, not switched off, and for
    a mask one flag per row and no device-side expiry (its kernel rebuilds r_q from the chain and does not know the mask)."""
    if search.masked_backend() is None:
        return False
    if mask is not None and any(layer.rotation_trick and layer.training for layer in layers):
        return False  # the rotation trick with a mask: the layer loop, each layer's one-stage backward is the fused kernel
    if mask is None:
        # quantize dropout on image / video input: the reference's own index shapes do not stack there
        # (residual_vq.py:198-208); the layer loop keeps that behaviour
        return x.ndim < 4
    d = x.shape[-1]
    # a [b, n] mask for [b, n, d] rows (anything else is the layer loop's to accept or refuse, as the reference does)
    if (x.ndim != 3 or mask.dtype != torch.bool or tuple(mask.shape) != tuple(x.shape[:2]) or d == 0 or d // groups > 512
            or mask.device != x.device):
        return False
    return not any(layer._codebook.expire_on_device for layer in layers)


def _stage_codes(owner, cbs, lead):
    """The natural codebooks of ``cbs`` stacked to [*lead, K, D] and their packed images for the fused launch, kept on
    ``owner._stage_cache`` and rebuilt only when some codes changed (Codebook.codes_state): an inference forward neither
    re-stacks nor re-packs."""
    backend = search.get_backend()
    if torch.compiler.is_compiling():  # traced: stack and pack are nodes of the graph (no identity-keyed cache in a trace)
        codes = torch.stack([cb.embeddings.detach()[0] for cb in cbs]).unflatten(0, lead)
        return codes, (backend.pack(codes, cbs[0].metric) if getattr(backend, "uses_packed", False) else None)
    key = (tuple(cb.codes_state() for cb in cbs), cbs[0].metric, getattr(backend, "name", None))
    if owner._stage_cache is None or owner._stage_cache[0] != key:
        with torch.no_grad():
            codes = torch.stack([cb.embeddings.detach()[0] for cb in cbs]).unflatten(0, lead)
            packed = None
            if getattr(backend, "uses_packed", False) and codes.is_cuda:
                packed = backend.pack(codes, cbs[0].metric)
        owner._stage_cache = (key, codes, packed)
    return owner._stage_cache[1], owner._stage_cache[2]


def _fused_stack(owner, stacks, flat, stage_codes, row_mask, run, share, freeze_codebook, out=None, idx=None, per_group=False):
    """The fused forward of ``stacks`` -- G homogeneous ResidualVQ, ``owner`` holding their caches -- on the fp32 rows ``flat``
    [G, rows, d] with ``stage_codes`` = owner._stage_codes() (fetched by the caller before it allocates its buffers): ONE launch
    for the stages 0 .. run - 1 of every group; with ``row_mask`` [rows] the search runs on every row and the mask pass
    (search.quantize_rows_masked) follows.  ``out`` / ``idx`` are destination views or None, ``per_group`` asks for the squared
    errors per group.  Nothing waits for the device.

    Returns (out [G, rows, d], idx [G, rows, run], sq_err [run] | [G, run] | None) and, in train mode, has done the EMA step of
    every layer that ran."""
    stack0 = stacks[0]
    first = stack0.layers[0]
    cb0 = first._codebook
    training = owner.training
    Q = stack0.num_quantizers
    codes, packed = stage_codes  # [G, Q, K, d] ([1, 1, K, d] when shared); fusable stacks are not learnable
    want_loss = training and first.has_commitment_loss
    zero_idx = None if row_mask is None else _zero_row_indices(owner, codes, packed, cb0.metric, Q)[:, :run]
    if run < Q and not share:  # quantize dropout: views of the first `run` codebooks and their images
        codes, packed = codes[:, :run], (packed[:run] if packed is not None else None)
    if row_mask is None:
        out, idx, sq_err = search.quantize_rows(flat, codes, metric=cb0.metric, ste=training, want_sq_err=want_loss, share=share,
                                                out=out, idx=idx, sq_err_per_head=per_group, packed=packed,
                                                rotate=training and first.rotation_trick)
    else:
        out, idx, sq_err = search.quantize_rows_masked(flat, codes, row_mask, zero_idx, metric=cb0.metric, ste=training,
                                                       want_sq_err=want_loss, share=share, out=out, idx=idx,
                                                       sq_err_per_head=per_group, packed=packed)
    if training and not freeze_codebook and cb0.ema_update:
        with torch.no_grad():
            chains = {}

            def residual_rows(g, q):
                if g not in chains:  # only needed when a code expired
                    stage_codes = (codes[g].expand(run, -1, -1) if share else codes[g]).detach()
                    if row_mask is None:
                        chains[g] = _residual_chain(flat[g].detach(), stage_codes, idx[g], ste=True)
                    else:
                        chains[g] = _residual_chain_masked(flat[g].detach(), stage_codes, idx[g], row_mask)
                return chains[g][q][None]

            idx_ema = idx
            if row_mask is not None:  # an index outside [0, K) ends a row's chain: masked-out rows contribute nothing
                idx_ema = idx.clone()
                idx_ema[:, :, 0].masked_fill_(~row_mask[None, :], -1)
            # one pass rebuilds the residual chain from the indices and scatter-adds every stage's statistics
            hits, sums = search.get_backend().ema_accumulate_residual(flat.detach(), codes.detach().contiguous(), idx_ema,
                                                                      ste=True, share=share)
            for g, stack in enumerate(stacks):
                for q, layer in zip(range(run), stack.layers):  # (a slice of a ModuleList would build a new module)
                    cbq = layer._codebook
                    if cbq.ema_update:
                        cbq.ema_apply(hits[g:g + 1, q], sums[g:g + 1, q])
                        if cbq.expire_on_device:  # the kernel rebuilds r_q for the rows it picks, from flat[g] in place: no chain
                            cbq.reseed_dead_codes((flat[g].detach(), codes[g].detach(), idx[g], q))
                        else:
                            cbq.reseed_dead_codes(lambda g=g, q=q: residual_rows(g, q))
    return out, idx, sq_err


def _stage_losses(owner, stacks, flat, row_mask, sq_err, run, shape):
    """The fp32 commitment losses, ``shape`` = [..., Q], of a fused forward from its squared errors: cached zeros in eval (no fill
    kernel per inference forward), fresh zeros in train mode without a commitment loss, zero columns for the stages dropout cut."""
    if not owner.training:
        return _cached_zeros(owner, "_zero_losses", shape, flat.device)
    lead, Q = shape[:-1], shape[-1]
    if sq_err is not None:
        rows, d = flat.shape[1:]
        # a mask: the kept rows are counted on the device; no kept row gives NaN, the reference's mean over nothing
        denom = rows * d if row_mask is None else row_mask.sum() * d
        losses = (sq_err / denom).to(torch.float32).reshape(*lead, run) * stacks[0].layers[0].commitment_weight
    else:
        losses = torch.zeros((*lead, run), dtype=torch.float32, device=flat.device)
    if run < Q:
        losses = torch.cat([losses, torch.zeros((*lead, Q - run), dtype=losses.dtype, device=flat.device)], dim=-1)
    return losses


class ResidualVQ(nn.Module):
    """Follows Algorithm 1 of https://arxiv.org/abs/2107.03312 (SoundStream), like the reference."""

    def __init__(
        self,
        *,
        dim,
        num_quantizers,
        codebook_dim=None,
        shared_codebook=False,
        heads=1,
        quantize_dropout=False,
        quantize_dropout_cutoff_index=0,
        quantize_dropout_multiple_of=1,
        **kwargs,
    ):
        super().__init__()
        assert heads == 1, "residual vq is not compatible with multi-headed codes"
        inner = dim if codebook_dim is None else codebook_dim
        self.has_projections = inner != dim
        self.project_in = nn.Linear(dim, inner) if self.has_projections else nn.Identity()
        self.project_out = nn.Linear(inner, dim) if self.has_projections else nn.Identity()
        self.num_quantizers = num_quantizers
        self.layers = nn.ModuleList(
            [VectorQuantize(dim=inner, codebook_dim=inner, **kwargs) for _ in range(num_quantizers)]
        )
        assert all(not layer.has_projections for layer in self.layers)

        self.quantize_dropout = quantize_dropout and num_quantizers > 1
        assert quantize_dropout_cutoff_index >= 0
        self.quantize_dropout_cutoff_index = quantize_dropout_cutoff_index
        self.quantize_dropout_multiple_of = quantize_dropout_multiple_of
        self.shared_codebook = shared_codebook
        if shared_codebook:
            first = self.layers[0]._codebook
            for layer in self.layers[1:]:
                layer._codebook = first
        self._stage_cache = None   # (key, stacked natural codebooks [1, Q|1, K, D], packed images) of the fused launch
        self._zero_idx_cache = None  # (the same key, [1, Q] indices of the all-zero row) of the fused masked launch
        self._zero_losses = None

    # ------------------------------------------------------------------ codes
    @property
    def codebooks(self):
        """[Q, K, D] stack of the per-layer codebooks."""
        return torch.stack([layer._codebook.embeddings[0] for layer in self.layers], dim=0)

    def _decode_tables(self):
        """The codebooks as the fused decode reads them, [1, Q | 1, K, D]: the learnable ones through the autograd graph,
        the others from the stack the fused forward keeps (_stage_codes)."""
        cbs = [self.layers[0]._codebook] if self.shared_codebook else [layer._codebook for layer in self.layers]
        if torch.is_grad_enabled() and any(cb.embeddings.requires_grad for cb in cbs):
            return torch.stack([cb.embeddings[0] for cb in cbs], dim=0)[None]
        return self._stage_codes()[0]

    def _decode_native(self, indices, want_sum):
        """(codes_sum [b, ..., D] | all_codes [Q, b, ..., D]) from one vq_decode_f32 call, or None when the call is not the
        fused decode's (search.decode_backend)."""
        first = self.layers[0]._codebook.embeddings
        decode = search.decode_backend(first, indices)
        if decode is None or indices.shape[-1] == 0:
            return None
        lead, Q = indices.shape[:-1], self.num_quantizers
        flat = indices.reshape(1, -1, indices.shape[-1])  # coarse indices: the missing stages are the call's Q_given
        codes_sum, all_codes = search.decode_rows(decode, self._decode_tables(), flat, num_stages=Q, drop_null=True,
                                                  want_sum=want_sum, want_all=not want_sum)
        if want_sum:
            return codes_sum.reshape(*lead, codes_sum.shape[-1])
        return all_codes.reshape(Q, *lead, all_codes.shape[-1])

    def get_codes_from_indices(self, indices):
        """indices [b, ..., q] (q may be < Q, -1 = dropped) -> [Q, b, ..., D]."""
        check_coarse(self, indices.shape[-1])
        codes = self._decode_native(indices, want_sum=False)
        if codes is not None:
            return codes
        indices, _ = pad_stages(indices, self.num_quantizers)
        dropped = indices < 0
        safe = indices.clamp(min=0)
        books = self.codebooks
        per_stage = [books[q][safe[..., q]] for q in range(self.num_quantizers)]
        codes = torch.stack(per_stage, dim=0)
        return codes.masked_fill(dropped.movedim(-1, 0)[..., None], 0.0)

    def get_output_from_indices(self, indices):
        check_coarse(self, indices.shape[-1])
        codes_sum = self._decode_native(indices, want_sum=True)  # nothing of [Q, N, D]: the stages are summed in registers
        if codes_sum is not None:
            return self.project_out(codes_sum)
        return self.project_out(self.get_codes_from_indices(indices).sum(dim=0))

    # ------------------------------------------------------------------ forward
    def _fusable(self, x, mask, drop_active: bool) -> bool:
        if (mask is not None or drop_active) and not _mask_fusable(self.layers, x, mask):
            return False
        first = self.layers[0]
        cb0 = first._codebook
        # the kernel keeps every stage's winners (and loss partials) in LDS: stacks beyond its budget (e.g. 32 stages of
        # dim 256 with the commitment loss) run layer by layer, one launch each, like the reference's loop
        limit = getattr(search.get_backend(), "max_fused_stages", None)
        if limit is not None and self.num_quantizers > limit(cb0.dim, self.training and first.has_commitment_loss):
            return False
        for layer in self.layers:
            cb = layer._codebook
            if (not layer.channel_last or not cb.is_initialized or cb._stochastic_requested()
                    or cb.transform_input is not cb0.transform_input
                    or cb.transform_input.__name__ != "_identity"
                    or cb.metric != cb0.metric or cb.embeddings.shape != cb0.embeddings.shape
                    or layer.commitment_weight != first.commitment_weight
                    or layer.rotation_trick != first.rotation_trick
                    or cb.learnable_codebook
                    # affine codebooks: every layer keeps its own running statistics of ITS residual rows
                    or cb.use_affine
                    # losses that look at the similarities go through VectorQuantize.forward layer by layer
                    or layer.commitment_use_cross_entropy_loss or layer.has_codebook_diversity_loss
                    or layer.has_codebook_orthogonal_loss):
                return False
        return True

    def forward(self, x, mask=None, indices=None, return_all_codes=False, freeze_codebook=False,
                rand_quantize_dropout_fixed_seed=None):
        assert indices is None, "cross-entropy to given indices is not supported (asserted in the reference as well)"
        x = self.project_in(x)
        drop_active = self.training and self.quantize_dropout
        # a SHARED codebook that is being updated must be searched stage by stage: in the reference every layer's forward
        # rewrites it (EMA) before the next layer looks at it (residual_vq.py:212-233, codebooks.py:399-426)
        shared_and_moving = (self.shared_codebook and self.training and not freeze_codebook
                             and self.layers[0]._codebook.ema_update)
        if not shared_and_moving and self._fusable(x, mask, drop_active):
            # quantize dropout: a stack cut after stage `cut` is the fused launch on cut + 1 stages
            cut = self._draw_cut(x, rand_quantize_dropout_fixed_seed) if drop_active else None
            quantized, all_indices, all_losses = self._forward_fused(x, freeze_codebook, mask=mask, cut=cut)
        else:
            quantized, all_indices, all_losses = self._forward_layers(x, mask, freeze_codebook, drop_active,
                                                                      rand_quantize_dropout_fixed_seed)
        quantized = self.project_out(quantized)
        ret = (quantized, all_indices, all_losses)
        if return_all_codes:
            ret = (*ret, self.get_codes_from_indices(all_indices))
        return ret

    def _stage_codes(self):
        """Stacked natural codebooks [1, Q, K, D] ([1, 1, K, D] when shared) and their packed images for the fused launch,
        rebuilt only when some layer's codes changed (Codebook.codes_state): an inference forward neither re-stacks nor
        re-packs."""
        if self.shared_codebook:
            return _stage_codes(self, [self.layers[0]._codebook], (1, 1))
        return _stage_codes(self, [layer._codebook for layer in self.layers], (1, self.num_quantizers))

    def _forward_fused(self, x, freeze_codebook, mask=None, cut=None):
        """One launch for the stages 0 .. cut (all of them without quantize dropout): the rows as one group of _fused_stack,
        which writes the indices of the stages that ran into their columns of the [..., Q] result."""
        lead, d = x.shape[:-1], x.shape[-1]
        flat = x.reshape(1, x.numel() // max(d, 1), d)
        wide_input = flat.dtype == torch.float64  # train mode: the reference's straight-through sums are in the input's width
        if flat.dtype != torch.float32:
            flat = flat.float()
        Q = self.num_quantizers
        run = Q if cut is None else cut + 1  # the stages that run; the dropped ones report index -1 and a zero loss
        rows = flat.shape[1]
        row_mask = None if mask is None else mask.reshape(rows)
        stage_codes = self._stage_codes()
        if run < Q:
            idx_buf = torch.full((1, rows, Q), -1, dtype=torch.int64, device=flat.device)
        else:
            idx_buf = torch.empty((1, rows, Q), dtype=torch.int64, device=flat.device)
        out, _, sq_err = _fused_stack(self, (self,), flat, stage_codes, row_mask, run, self.shared_codebook, freeze_codebook,
                                      idx=idx_buf[..., :run])
        losses = _stage_losses(self, (self,), flat, row_mask, sq_err, run, (1, Q))
        if self.training and wide_input:
            out = out.double()
        return out.reshape(*lead, d), idx_buf.reshape(*lead, Q), losses

    def _draw_cut(self, x, fixed_seed) -> int:
        """The last stage that runs under quantize dropout (residual_common.dropout_cut): one draw per forward, from the
        given seed, from a seed agreed between the replicas, or from the process-wide generator."""
        rng = fixed_seed
        if fixed_seed is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            seed = torch.tensor(random.randrange(10_000), device=x.device)
            dist.all_reduce(seed)
            rng = int(seed.item())
        return dropout_cut(self.quantize_dropout_cutoff_index, self.num_quantizers, self.quantize_dropout_multiple_of, rng)

    def _forward_layers(self, x, mask, freeze_codebook, drop_active, fixed_seed):
        Q = self.num_quantizers
        cut = self._draw_cut(x, fixed_seed) if drop_active else Q
        residual = x
        quantized_out = 0.0
        all_indices, all_losses = [], []
        for q, layer in enumerate(self.layers):
            if drop_active and q > cut:
                shape = (x.shape[0], *x.shape[-2:]) if x.ndim >= 4 else tuple(x.shape[:2])
                all_indices.append(torch.full(shape, -1, device=x.device, dtype=torch.long))
                all_losses.append(torch.zeros(1, device=x.device, dtype=x.dtype))
                continue
            quantized, layer_idx, layer_loss = layer(residual, mask=mask, freeze_codebook=freeze_codebook)
            residual = residual - quantized.detach()
            quantized_out = quantized_out + quantized
            all_indices.append(layer_idx)
            all_losses.append(layer_loss)
        return quantized_out, torch.stack(all_indices, dim=-1), torch.stack(all_losses, dim=-1)


class GroupedResidualVQ(nn.Module):
    def __init__(self, *, dim, groups=1, channel_last=True, **kwargs):
        super().__init__()
        assert dim % groups == 0
        self.dim = dim
        self.groups = groups
        self.channel_last = channel_last
        self.rvqs = nn.ModuleList([ResidualVQ(dim=dim // groups, **kwargs) for _ in range(groups)])
        self._stage_cache = None
        self._zero_idx_cache = None
        self._zero_losses = None

    @property
    def split_dim(self) -> int:
        return -1 if self.channel_last else 1

    @property
    def codebooks(self):
        return torch.stack(tuple(rvq.codebooks for rvq in self.rvqs))

    def _decode_uniform(self, indices):
        """(decode, tables [G, Q, K, d]) when ONE vq_decode_f32 call with the groups on its group axis decodes ``indices``
        [G, b, ..., q]: uniform groups (same Q, K, d, no projections, the condition _fusable checks for the shapes), else None."""
        r0 = self.rvqs[0]
        first = r0.layers[0]._codebook.embeddings
        if not isinstance(indices, torch.Tensor) or indices.dim() < 2 or indices.shape[0] != self.groups or indices.shape[-1] == 0:
            return None
        decode = search.decode_backend(first, indices)
        if decode is None:
            return None
        for rvq in self.rvqs:
            if rvq.has_projections or rvq.shared_codebook or rvq.num_quantizers != r0.num_quantizers:
                return None
            for layer in rvq.layers:
                e = layer._codebook.embeddings
                if e.shape != first.shape or e.dtype != first.dtype or e.device != first.device:
                    return None
        for rvq in self.rvqs:
            check_coarse(rvq, indices.shape[-1])
        cbs = [layer._codebook for rvq in self.rvqs for layer in rvq.layers]
        if torch.is_grad_enabled() and any(cb.embeddings.requires_grad for cb in cbs):
            return decode, self.codebooks
        return decode, self._stage_codes()[0]

    def get_codes_from_indices(self, indices):
        uniform = self._decode_uniform(indices)
        if uniform is not None:  # [G, Q, b, ..., d] written by one call
            decode, tables = uniform
            G, Q, d = self.groups, tables.shape[1], tables.shape[-1]
            flat, lead = grouped_decode_rows(indices)
            if search.decode_needs_grad(tables):
                _, codes = search.decode_rows(decode, tables, flat, drop_null=True, want_sum=False, want_all=True)
                return codes.transpose(0, 1).reshape(G, Q, *lead, d)
            codes, dest = grouped_decode_dest(flat, lead, d, Q)
            search.decode_rows(decode, tables, flat, drop_null=True, want_sum=False, want_all=True, all_out=dest)
            return codes
        return torch.stack(tuple(rvq.get_codes_from_indices(i) for rvq, i in zip(self.rvqs, indices)))

    def get_output_from_indices(self, indices):
        uniform = self._decode_uniform(indices) if self.channel_last else None
        if uniform is not None:  # the groups' sums written side by side on the feature axis by one call
            decode, tables = uniform
            G, d = self.groups, tables.shape[-1]
            flat, lead = grouped_decode_rows(indices)
            if search.decode_needs_grad(tables):
                out, _ = search.decode_rows(decode, tables, flat, drop_null=True)
                return out.transpose(0, 1).reshape(*lead, G * d)
            out, dest = grouped_decode_dest(flat, lead, d)
            search.decode_rows(decode, tables, flat, drop_null=True, sum_out=dest)
            return out
        outs = tuple(rvq.get_output_from_indices(i) for rvq, i in zip(self.rvqs, indices))
        return torch.cat(outs, dim=self.split_dim)

    def _fusable(self, x, mask) -> bool:
        if not self.channel_last:
            return False
        # one mask for all groups: one grouped launch and one mask pass (active quantize dropout keeps the loop over the
        # groups below, every group drawing its own cut and fusing on its own)
        if mask is not None and not _mask_fusable([layer for rvq in self.rvqs for layer in rvq.layers], x, mask, self.groups):
            return False
        r0 = self.rvqs[0]
        for rvq in self.rvqs:
            if rvq.has_projections or rvq.shared_codebook or rvq.num_quantizers != r0.num_quantizers:
                return False
            if (rvq.training and rvq.quantize_dropout) or not rvq._fusable(x, None, False):
                return False
            if rvq.layers[0]._codebook.embeddings.shape != r0.layers[0]._codebook.embeddings.shape:
                return False
            if rvq.layers[0]._codebook.metric != r0.layers[0]._codebook.metric:
                return False
        return True

    def forward(self, x, indices=None, return_all_codes=False, freeze_codebook=False, mask=None):
        assert x.shape[self.split_dim] == self.dim
        assert indices is None or len(indices) == 0, "cross-entropy to given indices is not supported"
        if self._fusable(x, mask):
            return self._forward_fused(x, return_all_codes, freeze_codebook, mask)
        seed = random.randint(0, int(1e7))  # (on this path only: the fused one consumes nothing of `random`)
        return grouped_fallback(self.rvqs, x, self.split_dim, seed, return_all_codes, torch.stack, mask=mask,
                                freeze_codebook=freeze_codebook)

    def _stage_codes(self):
        """[G, Q, K, d] natural codebooks + packed images of the one fused launch, rebuilt only when some codes changed."""
        cbs = [layer._codebook for rvq in self.rvqs for layer in rvq.layers]
        return _stage_codes(self, cbs, (self.groups, len(cbs) // self.groups))

    def _forward_fused(self, x, return_all_codes, freeze_codebook, mask=None):
        """Groups on the kernel's head axis: x [..., G*d] is searched in place as a [G, rows, d] view and the result written as
        its [rows, G, d] counterpart, both by _fused_stack; ``mask`` [b, n] is shared by the groups, and squared errors come back
        per group and stage."""
        G = self.groups
        rvqs = self.rvqs
        training = self.training
        lead = x.shape[:-1]
        d = self.dim // G
        xc = x if (x.is_contiguous() and x.dtype == torch.float32) else x.contiguous().float()
        rows = xc.numel() // self.dim
        flat = xc.view(rows, G, d).permute(1, 0, 2)
        stage_codes = self._stage_codes()  # [G, Q, K, d]
        Q = stage_codes[0].shape[1]
        q_buf = torch.empty((rows, G, d), dtype=torch.float32, device=xc.device)
        row_mask = None if mask is None else mask.reshape(rows)
        out, idx, sq_err = _fused_stack(self, rvqs, flat, stage_codes, row_mask, Q, False, freeze_codebook,
                                        out=q_buf.permute(1, 0, 2), per_group=True)
        losses = _stage_losses(self, rvqs, flat, row_mask, sq_err, Q, (G, 1, Q))
        quantized = out.permute(1, 0, 2).reshape(*lead, self.dim)  # q_buf's memory; keeps the autograd edge of `out`
        if training and x.dtype == torch.float64:
            quantized = quantized.double()
        all_indices = idx.reshape(G, *lead, Q)
        ret = (quantized, all_indices, losses)
        if return_all_codes:
            ret = (*ret, self.get_codes_from_indices(all_indices))
        return ret
