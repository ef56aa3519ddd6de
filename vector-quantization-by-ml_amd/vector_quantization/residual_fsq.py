"""Residual finite scalar quantization: the reference's ``ResidualFSQ`` and ``GroupedResidualFSQ``
(``vector_quantization/residual_fsq.py``), a stack of ``FSQ`` layers whose stage q quantizes what the stages before it
left over, scaled by (levels - 1)^-q.

Fused path (the hot path).  After ``project_in``, the first bound and every stage's bound / round / rescale / subtract /
accumulate chain, with the stages' indices, are one HIP pass (``vq_fsq_quantize_f32`` with ``prebound``: one thread per
row, its d <= 16 values held in registers across the stages), and dL/dx is one more (``vq_fsq_backward_f32``).
``GroupedResidualFSQ`` runs its G groups as the kernels' group axis, reading the ``x.chunk`` views in place when there are
no projections: G groups x Q stages are one launch.  ``get_codes_from_indices`` / ``get_output_from_indices`` on GPU
tensors run the decode kernel (``vq_fsq_decode_f32``).

Fallback path.  The reference's ``forward`` line by line over the module's own ``FSQ`` layers, in torch on the GPU: fp64
inputs, codebook dims above 16, layer options the kernel does not take (``channel_first``, several codebooks,
``keep_num_codebooks_dim``, ``return_indices=False``), ``accept_image_fmap`` groups.  It is the GPU oracle of the fused path.

CPU tensors raise ``native.NativeUnavailable`` in ``forward``; ``codebooks`` and the index helpers are torch on the CPU.
DESIGN.md section 12 states the accuracy contract.
"""
from __future__ import annotations

import random

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn import Module

from . import finite_scalar_quantization as _fsq
from .finite_scalar_quantization import FSQ
from .residual_common import (check_coarse, dropout_cut, group_rows_in, group_rows_out, grouped_fallback, pad_stages,
                              rows_contiguous)


def _fused_ok(rvq: "ResidualFSQ", x: torch.Tensor) -> bool:
    """x: the project_in output.  The first bound promotes it to fp32 (fp64 stays fp64: the fallback)."""
    l0 = rvq.layers[0]
    if x.dtype == torch.float64 or not x.is_floating_point():
        return False
    probe = x if x.dtype == torch.float32 else x.new_empty((0,), dtype=torch.float32)
    return (_fsq._fused_ok(probe, l0._level_values) and l0.num_codebooks == 1 and not l0.keep_num_codebooks_dim
            and not l0.channel_first and l0.return_indices and not l0.has_projections)


class ResidualFSQ(Module):
    """Follows Algorithm 1. in https://arxiv.org/pdf/2107.03312.pdf"""

    def __init__(
        self,
        *,
        dim,
        levels: list[int],
        num_quantizers,
        quantize_dropout=False,
        quantize_dropout_cutoff_index=0,
        quantize_dropout_multiple_of=1,
        **kwargs,
    ):
        super().__init__()
        codebook_dim = len(levels)

        requires_projection = codebook_dim != dim
        self.project_in = nn.Linear(dim, codebook_dim) if requires_projection else nn.Identity()
        self.project_out = nn.Linear(codebook_dim, dim) if requires_projection else nn.Identity()
        self.has_projections = requires_projection

        self.num_quantizers = num_quantizers

        self.levels = levels
        self.layers = nn.ModuleList([])

        levels_tensor = torch.Tensor(levels)

        scales = []

        for ind in range(num_quantizers):
            scales.append((levels_tensor - 1) ** -ind)

            fsq = FSQ(levels=levels, dim=codebook_dim, **kwargs)

            self.layers.append(fsq)

        assert all([not fsq.has_projections for fsq in self.layers])

        self.codebook_size = self.layers[0].codebook_size

        self.register_buffer("scales", torch.stack(scales), persistent=False)

        self.quantize_dropout = quantize_dropout and num_quantizers > 1

        assert quantize_dropout_cutoff_index >= 0

        self.quantize_dropout_cutoff_index = quantize_dropout_cutoff_index
        self.quantize_dropout_multiple_of = quantize_dropout_multiple_of  # encodec paper proposes structured dropout, believe this was set to 4

    @property
    def codebooks(self):
        codebooks = [layer.implicit_codebook for layer in self.layers]
        codebooks = torch.stack(codebooks, dim=0)
        return codebooks

    def _padded_indices(self, indices):
        """indices [b, ..., q] -> [b, n, num_quantizers] (pack "b * q", then the -1 padding of coarse indices)."""
        quantize_dim = indices.shape[-1]
        indices = indices.reshape(indices.shape[0], -1, quantize_dim)
        check_coarse(self, quantize_dim)
        if quantize_dim < self.num_quantizers:
            indices = F.pad(indices, (0, self.num_quantizers - quantize_dim), value=-1)
        return indices

    def _decode(self, indices, want_sum, want_all):
        Q = self.num_quantizers
        flat = self._padded_indices(indices).reshape(-1, Q)
        scales = self.scales.to(torch.float32).contiguous()
        return _fsq.native.fsq_decode(flat, self.layers[0]._level_values, scales, drop_null=True, want_sum=want_sum,
                                      want_all=want_all)

    def get_codes_from_indices(self, indices):
        """indices [b, ..., q] (q <= num_quantizers; -1 = dropped) -> codes [num_quantizers, b, ..., codebook_dim]."""
        lead = indices.shape[:-1]
        d = len(self.levels)
        if _fsq.decode_ok(indices, self.levels):
            _, all_codes = self._decode(indices, want_sum=False, want_all=True)
            return all_codes.reshape(self.num_quantizers, *lead, d)

        indices = self._padded_indices(indices)

        # take care of quantizer dropout

        mask = indices == -1
        indices = indices.masked_fill(mask, 0)  # have it fetch a dummy code to be masked out later

        codebooks = self.codebooks
        all_codes = torch.stack([codebooks[q][indices[..., q]] for q in range(self.num_quantizers)])  # q b n d

        # mask out any codes that were dropout-ed

        all_codes = all_codes.masked_fill(mask.permute(2, 0, 1)[..., None], 0.0)

        # scale the codes

        all_codes = all_codes * self.scales[:, None, None, :]

        return all_codes.reshape(self.num_quantizers, *lead, d)

    def get_output_from_indices(self, indices):
        if _fsq.decode_ok(indices, self.levels):
            codes_summed, _ = self._decode(indices, want_sum=True, want_all=False)
            codes_summed = codes_summed.reshape(*indices.shape[:-1], len(self.levels))
        else:
            codes_summed = self.get_codes_from_indices(indices).sum(dim=0)
        return self.project_out(codes_summed)

    def _dropout_cut(self, seed):
        """The last active stage under quantize dropout (None: every stage runs), consuming `random` as the reference."""
        if not (self.training and self.quantize_dropout):
            return None
        return dropout_cut(self.quantize_dropout_cutoff_index, self.num_quantizers, self.quantize_dropout_multiple_of, seed)

    def _kernel_consts(self, stages):
        consts = _fsq.cached_kernel_consts(self, self.layers[0]._levels, self.scales)
        return consts[: 3 + stages]

    def forward(self, x, return_all_codes=False, rand_quantize_dropout_fixed_seed=None):
        num_quant = self.num_quantizers

        x = self.project_in(x)

        cut = self._dropout_cut(rand_quantize_dropout_fixed_seed)
        stages = num_quant if cut is None else min(cut + 1, num_quant)

        if _fused_ok(self, x):
            d = len(self.levels)
            xg = rows_contiguous(x.float().reshape(1, -1, d))
            with torch.autocast(device_type="cuda", enabled=False):
                out, idx = _fsq.fused_quantize(xg, self.layers[0]._level_values, self._kernel_consts(stages), prebound=True)
            quantized_out = self.project_out(out.reshape(*x.shape[:-1], d))
            all_indices, _ = pad_stages(idx.reshape(*x.shape[:-1], stages), num_quant)
        else:
            if not (x.is_cuda or _fsq._compiling()):
                _fsq.native._require_gpu(x)
            quantized_out, all_indices = self._forward_stagewise(x, cut)

        ret = (quantized_out, all_indices)

        if not return_all_codes:
            return ret

        # whether to return all codes from all codebooks across layers

        all_codes = self.get_codes_from_indices(all_indices)

        # will return all codes in shape (quantizer, batch, sequence length, codebook dimension)

        return (*ret, all_codes)

    def _forward_stagewise(self, x, cut):
        """The fallback: the reference's loop over the FSQ layers (residual_fsq.py:128-197), each layer in torch."""
        quantized_out = 0.0
        residual = self.layers[0].bound(x)

        all_indices = []

        if cut is not None:
            null_indices = torch.full(x.shape[:2], -1.0, device=x.device, dtype=torch.long)

        with torch.autocast(device_type="cuda", enabled=False):
            for quantizer_index, (layer, scale) in enumerate(zip(self.layers, self.scales)):
                if cut is not None and quantizer_index > cut:
                    all_indices.append(null_indices)
                    continue

                quantized, indices = layer._forward(residual / scale, fused=False)
                quantized = quantized * scale

                residual = residual - quantized.detach()
                quantized_out = quantized_out + quantized

                all_indices.append(indices)

        quantized_out = self.project_out(quantized_out)

        all_indices = torch.stack(all_indices, dim=-1)

        return quantized_out, all_indices


# grouped residual fsq


class GroupedResidualFSQ(Module):
    def __init__(self, *, dim, groups=1, accept_image_fmap=False, **kwargs):
        super().__init__()
        self.dim = dim
        self.groups = groups
        assert (dim % groups) == 0
        dim_per_group = dim // groups

        self.accept_image_fmap = accept_image_fmap

        self.rvqs = nn.ModuleList([])

        for _ in range(groups):
            self.rvqs.append(ResidualFSQ(dim=dim_per_group, **kwargs))

        self.codebook_size = self.rvqs[0].codebook_size

    @property
    def codebooks(self):
        return torch.stack(tuple(rvq.codebooks for rvq in self.rvqs))

    @property
    def split_dim(self):
        return 1 if self.accept_image_fmap else -1

    def get_codes_from_indices(self, indices):
        codes = tuple(rvq.get_codes_from_indices(chunk_indices) for rvq, chunk_indices in zip(self.rvqs, indices))
        return torch.stack(codes)

    def get_output_from_indices(self, indices):
        outputs = tuple(rvq.get_output_from_indices(chunk_indices) for rvq, chunk_indices in zip(self.rvqs, indices))
        return torch.cat(outputs, dim=self.split_dim)

    def forward(self, x, return_all_codes=False):
        shape, split_dim = x.shape, self.split_dim
        assert shape[split_dim] == self.dim

        seed = random.randint(0, int(1e7))  # drawn in eval too, as the reference does

        if split_dim == -1 and self._fused_ok(x):
            return self._forward_fused(x, return_all_codes, seed)

        return grouped_fallback(self.rvqs, x, split_dim, seed, return_all_codes, tuple)

    def _fused_ok(self, x):
        rvq0 = self.rvqs[0]
        if rvq0.has_projections:
            w = rvq0.project_in.weight
            probe = x.new_empty((0, len(rvq0.levels)), dtype=torch.promote_types(x.dtype, w.dtype))
        else:
            probe = x
        return _fused_ok(rvq0, probe)

    def _forward_fused(self, x, return_all_codes, seed):
        G = self.groups
        rvq0 = self.rvqs[0]
        Q = rvq0.num_quantizers
        cut = rvq0._dropout_cut(seed)  # every group gets the same seed, so the same cut
        stages = Q if cut is None else min(cut + 1, Q)
        lead = x.shape[:-1]
        d = len(rvq0.levels)
        consts = rvq0._kernel_consts(stages)
        xg, _ = group_rows_in(x, self.rvqs, d, rvq0.has_projections)
        with torch.autocast(device_type="cuda", enabled=False):
            out, idx = _fsq.fused_quantize(xg, rvq0.layers[0]._level_values, consts, prebound=True,
                                           interleave=not rvq0.has_projections)
        quantized = group_rows_out(out, self.rvqs, lead, d, rvq0.has_projections)
        all_indices, _ = pad_stages(idx.reshape(G, *lead, stages), Q)
        ret = (quantized, all_indices)
        if not return_all_codes:
            return ret
        return (*ret, tuple(rvq.get_codes_from_indices(all_indices[g]) for g, rvq in enumerate(self.rvqs)))
