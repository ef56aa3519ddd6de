"""Finite scalar quantization: the reference's ``FSQ`` and ``round_ste`` (``vector_quantization/finite_scalar_quantization.py``).

Finite Scalar Quantization: VQ-VAE Made Simple - https://arxiv.org/abs/2309.15505

Fused path (the hot path).  After ``project_in``, bound, round, the division by the half width and the index of every
(row, codebook) sub-row are one HIP pass (``vq_fsq_quantize_f32``: one thread per sub-row, its d <= 16 values in
registers), and dL/dx one more (``vq_fsq_backward_f32``).  The bound constants are computed here in torch with the
reference's own expressions, once per device, and handed to the kernels.  ``indices_to_codes`` on GPU tensors runs the
decode kernel (``vq_fsq_decode_f32``), bitwise the reference's arithmetic.

Fallback path.  The reference's ``forward`` line by line in torch, on the GPU only: fp64 inputs, ``allowed_dtypes`` that
keep another dtype, more than 16 dims per codebook.  It is also the GPU oracle of the fused path.

CPU tensors raise ``native.NativeUnavailable`` in ``forward``; the index helpers are torch on any device.  One divergence
from the reference: a level below 2 raises ``ValueError`` (the reference computes NaN bounds there).  DESIGN.md section 12
states the accuracy contract.
"""
from __future__ import annotations

import torch
from torch import Tensor, int32, nn
from torch.nn import Module

from . import native
from .residual_common import rows_contiguous

MAX_FUSED_DIM = native.FSQ_MAX_DIM
_INT32_MAX = 2**31 - 1


def round_ste(features: Tensor) -> Tensor:
    """Round with straight through gradients."""
    zhat = features.round()
    return features + (zhat - features).detach()


def _compiling() -> bool:
    return torch.compiler.is_compiling()


def _fused_ok(x: Tensor, levels) -> bool:
    """Whether the kernels take a quantizer input x (its last dim = len(levels)): fp32, d <= 16, an int32 codebook."""
    size = 1
    for v in levels:
        size *= int(v)
    return ((x.is_cuda or _compiling()) and x.dtype == torch.float32 and 1 <= len(levels) <= MAX_FUSED_DIM
            and size <= _INT32_MAX)


def kernel_consts(levels: Tensor, scales: Tensor | None, eps: float = 1e-3) -> Tensor:
    """The kernels' float constants [3 + S, d]: half_l, offset, shift by ``FSQ.bound``'s own expressions (on the levels'
    device, so they are the fallback's values), then the stage scales (S = 1 of ones when None)."""
    half_l = (levels - 1) * (1 + eps) / 2
    offset = torch.where(levels % 2 == 0, 0.5, 0.0)
    shift = (offset / half_l).atanh()
    if scales is None:
        scales = torch.ones((1, levels.shape[0]), dtype=torch.float32, device=levels.device)
    return torch.cat([half_l[None], offset[None], shift[None], scales.to(torch.float32)]).contiguous()


def cached_kernel_consts(owner: Module, levels: Tensor, scales: Tensor | None) -> Tensor:
    """kernel_consts, kept on `owner` until its buffers move (traced afresh under torch.compile)."""
    if _compiling():
        return kernel_consts(levels, scales)
    key = (levels.device, levels.data_ptr(), None if scales is None else (scales.data_ptr(), scales._version))
    cache = owner.__dict__.get("_kernel_consts_cache")
    if cache is None or cache[0] != key:
        cache = (key, kernel_consts(levels, scales))
        owner.__dict__["_kernel_consts_cache"] = cache
    return cache[1]


def _quantize_call(x, levels, consts, prebound, want_idx, out=None):
    if _compiling():
        o, idx = torch.ops.vq_mi355x.fsq_quantize(x, list(levels), consts, prebound, want_idx)
        if out is not None:
            out.copy_(o)
            o = out
        return o, (idx if want_idx else None)
    return native.fsq_quantize(x, levels, consts, prebound=prebound, want_idx=want_idx, out=out)


class _FsqFn(torch.autograd.Function):
    """x [G, N, d] fp32 -> out [G, N, d] (the sum over the stages of code * scale), idx [G, N, S] int32 (or None).
    interleave: out is allocated as [N, G, d] and returned as its [G, N, d] view (the grouped layout)."""

    @staticmethod
    def forward(ctx, x, levels, consts, prebound, want_idx, interleave):
        G, N, d = x.shape
        out = None
        if interleave:
            out = torch.empty((N, G, d), dtype=torch.float32, device=x.device).transpose(0, 1)
        out, idx = _quantize_call(x.detach(), levels, consts, prebound, want_idx, out)
        ctx.save_for_backward(x, consts)
        ctx.meta = (levels, prebound)
        if idx is not None:
            ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, g_out, g_idx):
        x, consts = ctx.saved_tensors
        levels, prebound = ctx.meta
        if _compiling():
            gx = torch.ops.vq_mi355x.fsq_backward(x.detach(), list(levels), consts, prebound, g_out)
        else:
            gx = native.fsq_backward(x.detach(), levels, consts, g_out, prebound=prebound)
        return gx, None, None, None, None, None


def fused_quantize(x: Tensor, levels, consts: Tensor, *, prebound: bool, want_idx: bool = True, interleave: bool = False):
    """The fused chain over x [G, N, d] (rows contiguous): (out [G, N, d], idx [G, N, S] int32 or None)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _FsqFn.apply(x, tuple(levels), consts, prebound, want_idx, interleave)
    out = None
    if interleave:
        G, N, d = x.shape
        out = torch.empty((N, G, d), dtype=torch.float32, device=x.device).transpose(0, 1)
    return _quantize_call(x, levels, consts, prebound, want_idx, out)


def decode_ok(indices: Tensor, levels) -> bool:
    return (indices.is_cuda and not _compiling() and indices.dtype in (torch.int32, torch.int64)
            and 1 <= len(levels) <= MAX_FUSED_DIM)


class FSQ(Module):
    """Finite Scalar Quantization module (the reference's constructor arguments, attributes, methods and return tuple)."""

    def __init__(
        self,
        levels: list[int],
        dim: int | None = None,
        num_codebooks=1,
        keep_num_codebooks_dim: bool | None = None,
        allowed_dtypes: tuple[torch.dtype, ...] = (torch.float32, torch.float64),
        channel_first: bool = False,
        projection_has_bias: bool = True,
        return_indices=True,
    ):
        super().__init__()
        levels = [int(v) for v in levels]
        if len(levels) < 1 or min(levels) < 2:
            raise ValueError(f"FSQ: every level must be >= 2 (got {levels})")
        self._level_values = tuple(levels)
        _levels = torch.tensor(levels, dtype=int32)
        self.register_buffer("_levels", _levels, persistent=False)

        _basis = torch.cumprod(torch.tensor([1] + levels[:-1]), dim=0, dtype=int32)
        self.register_buffer("_basis", _basis, persistent=False)

        codebook_dim = len(levels)
        self.codebook_dim = codebook_dim

        effective_codebook_dim = codebook_dim * num_codebooks
        self.num_codebooks = num_codebooks
        self.effective_codebook_dim = effective_codebook_dim

        keep_num_codebooks_dim = keep_num_codebooks_dim if keep_num_codebooks_dim else num_codebooks > 1
        assert not (num_codebooks > 1 and not keep_num_codebooks_dim)
        self.keep_num_codebooks_dim = keep_num_codebooks_dim

        self.dim = dim if dim else len(_levels) * num_codebooks

        self.channel_first = channel_first

        has_projections = self.dim != effective_codebook_dim
        self.project_in = (nn.Linear(self.dim, effective_codebook_dim, bias=projection_has_bias) if has_projections
                           else nn.Identity())
        self.project_out = (nn.Linear(effective_codebook_dim, self.dim, bias=projection_has_bias) if has_projections
                            else nn.Identity())

        self.has_projections = has_projections

        self.return_indices = return_indices
        if return_indices:
            self.codebook_size = self._levels.prod().item()
            implicit_codebook = self._indices_to_codes(torch.arange(self.codebook_size))
            self.register_buffer("implicit_codebook", implicit_codebook, persistent=False)

        self.allowed_dtypes = allowed_dtypes

    def bound(self, features: Tensor, eps: float = 1e-3) -> Tensor:
        """Bound `features`, an array of shape (..., d)."""
        half_l = (self._levels - 1) * (1 + eps) / 2
        offset = torch.where(self._levels % 2 == 0, 0.5, 0.0)
        shift = (offset / half_l).atanh()
        return (features + shift).tanh() * half_l - offset

    def quantize(self, features: Tensor) -> Tensor:
        """Quantize features, returns quantized zhat, same shape as features."""
        quantized = round_ste(self.bound(features))
        half_width = self._levels // 2  # Renormalize to [-1, 1].
        return quantized / half_width

    def _scale_and_shift(self, zhat_normalized: Tensor) -> Tensor:
        half_width = self._levels // 2
        return (zhat_normalized * half_width) + half_width

    def _scale_and_shift_inverse(self, zhat: Tensor) -> Tensor:
        half_width = self._levels // 2
        return (zhat - half_width) / half_width

    def _indices_to_codes(self, indices: Tensor) -> Tensor:
        if decode_ok(indices, self._level_values):
            ones = torch.ones((1, self.codebook_dim), dtype=torch.float32, device=indices.device)
            codes, _ = native.fsq_decode(indices.reshape(-1, 1), self._level_values, ones)
            return codes.reshape(*indices.shape, self.codebook_dim)
        level_indices = self.indices_to_level_indices(indices)
        codes = self._scale_and_shift_inverse(level_indices)
        return codes

    def codes_to_indices(self, codes: Tensor) -> Tensor:
        """Convert a `code` to an index in the codebook."""
        assert codes.shape[-1] == self.codebook_dim
        codes = self._scale_and_shift(codes)
        index = (codes * self._basis).sum(dim=-1)
        # NaN -> INT32_MIN, what the reference's CPU cast gives (a GPU cast does not promise it)
        return torch.where(index.isnan(), torch.iinfo(int32).min, index.to(int32))

    def indices_to_level_indices(self, indices: Tensor) -> Tensor:
        """Convert indices to indices at each level, perhaps needed for a transformer with factorized embeddings."""
        indices = indices[..., None]
        codes_non_centered = (indices // self._basis) % self._levels
        return codes_non_centered

    def indices_to_codes(self, indices: Tensor) -> Tensor:
        """Inverse of `codes_to_indices`."""
        codes = self._indices_to_codes(indices)

        if self.keep_num_codebooks_dim:
            codes = codes.reshape(*codes.shape[:-2], codes.shape[-2] * codes.shape[-1])

        codes = self.project_out(codes)

        if self.channel_first:
            codes = codes.movedim(-1, 1)

        return codes

    def forward(self, features: Tensor) -> tuple[Tensor, Tensor]:
        """features (B, dim, *) if channel_first, else (B, *, dim) -> (out of the same shape, indices (B, *) int32, with a
        trailing codebook dim when keep_num_codebooks_dim; None when return_indices is False)."""
        with torch.autocast(device_type="cuda", enabled=False):
            return self._forward(features, fused=True)

    def _forward(self, features: Tensor, fused: bool):
        if not (features.is_cuda or _compiling()):
            native._require_gpu(features)
        orig_dtype = features.dtype

        if self.channel_first:
            features = features.movedim(1, -1)

        lead = features.shape[1:-1]
        features = features.reshape(features.shape[0], -1, features.shape[-1])  # pack "b * d"

        assert features.shape[-1] == self.dim, f"expected dimension of {self.dim} but found dimension of {features.shape[-1]}"

        features = self.project_in(features)

        b, n = features.shape[0], features.shape[1]
        features = features.reshape(b, n, self.num_codebooks, self.codebook_dim)

        # make sure allowed dtype before quantizing

        if features.dtype not in self.allowed_dtypes:
            features = features.float()

        if fused and _fused_ok(features, self._level_values):
            consts = cached_kernel_consts(self, self._levels, None)
            xg = rows_contiguous(features.reshape(1, -1, self.codebook_dim))
            codes, indices = fused_quantize(xg, self._level_values, consts, prebound=False, want_idx=self.return_indices)
            codes = codes.reshape(b, n, self.num_codebooks, self.codebook_dim)
            if indices is not None:
                indices = indices.reshape(b, n, self.num_codebooks)
        else:
            codes = self.quantize(features)
            indices = self.codes_to_indices(codes) if self.return_indices else None

        codes = codes.reshape(b, n, self.effective_codebook_dim)

        # cast codes back to original dtype

        if codes.dtype != orig_dtype:
            codes = codes.type(orig_dtype)

        out = self.project_out(codes)

        # reconstitute image or video dimensions
        out = out.reshape(b, *lead, out.shape[-1])
        if self.channel_first:
            out = out.movedim(-1, 1)

        if self.return_indices:
            indices = indices.reshape(b, *lead, self.num_codebooks)

        if not self.keep_num_codebooks_dim and self.return_indices:
            indices = indices.squeeze(-1)

        return out, indices
