"""Latent quantization: the reference's ``LatentQuantize`` (``vector_quantization/latent_quantization.py``).

Disentanglement via Latent Quantization - https://arxiv.org/abs/2305.18378

Each of the d latent dimensions is quantized on its own against a learnable table of L_i values: the nearest value (the
first minimum of |z_i - v_i[j]|), the straight-through value c_i = z_i + (q_i - z_i), and the index
(int32) sum_i ((c_i * 2) * hw_i + hw_i) * basis_i, which the reference evaluates from c_i in fp32 and truncates.

Fused path (the hot path).  Search, straight-through value and index of every (batch, position, codebook) sub-row are one
HIP pass (``vq_lq_quantize_f32``: one thread per sub-row, its d <= 16 values in registers, the tables in LDS).  Without
projections the kernel reads the caller's channel-first tensor as it lies and writes ``out`` channel-first, so the
reference's two layout copies disappear, and in training the same pass also sums the squared error (the loss is one more
tiny launch).  dL/dx is ``vq_lq_backward_f32``, or no launch at all when the two loss weights are equal (their gradients
cancel).  With projections ``nn.Linear`` and the loss stay in torch.  ``indices_to_codes`` on GPU indices runs the FSQ
decode kernel (``(k - hw) / hw / 2`` is bitwise ``(k - hw) / hw * 0.5``).

Fallback path.  The reference's ``forward`` line by line in torch, on the GPU only: inputs or tables that are not fp32,
more than 16 dims per codebook, tables above 4096 floats in all.  It is also the GPU oracle of the fused path.

CPU tensors raise ``native.NativeUnavailable`` in ``forward``; the index helpers are torch on any device.

Divergences from the reference: a level below 2 raises ``ValueError`` (the reference builds a NaN
codebook); ``num_codebooks > 1`` and ``keep_num_codebooks_dim=True`` construct (the reference's constructor raises while
building ``implicit_codebook``; here it is the [K, d] table that ``num_codebooks = 1`` gives); with
``optimize_values=False`` the tables stay a plain list of CPU tensors as in the reference, and the module keeps a device
copy so that a GPU forward works; with ``in_place_codebook_optimizer`` a training-mode forward raises
``NotImplementedError`` (the reference's reads an attribute that is never set).  As in the reference,
``values_per_latent`` never receives a gradient: the straight-through ``detach`` cuts it off.
"""
from __future__ import annotations

from typing import Callable

import torch
import torch.nn.functional as F
from torch import Tensor, int32, nn
from torch.nn import Module
from torch.optim import Optimizer

from . import native

MAX_FUSED_DIM = native.LQ_MAX_DIM
MAX_TABLE_FLOATS = native.LQ_MAX_TABLE_FLOATS
_INT32_MAX = 2**31 - 1


def _compiling() -> bool:
    return torch.compiler.is_compiling()


def _fused_ok(z: Tensor, levels, tables) -> bool:
    """Whether the kernel takes a quantizer input z: fp32 input and tables, d <= 16, tables within the LDS budget, an int32
    codebook."""
    size = 1
    for v in levels:
        size *= int(v)
    return ((z.is_cuda or _compiling()) and z.dtype == torch.float32 and 1 <= len(levels) <= MAX_FUSED_DIM
            and sum(levels) <= MAX_TABLE_FLOATS and size <= _INT32_MAX
            and all(t.dtype == torch.float32 and t.numel() == L for t, L in zip(tables, levels)))


def _quantize_call(z, levels, tables, C, weights, out):
    """z, out: [B, P, C * d] views -> (out, idx [B, P, C] int32, loss [2] or None)."""
    if _compiling():
        w_c, w_q = weights if weights is not None else (0.0, 0.0)
        o, idx, loss = torch.ops.vq_mi355x.lq_quantize(z, list(levels), tables, C, True, weights is not None, w_c, w_q)
        return o, idx, (loss if weights is not None else None)
    return native.lq_quantize(z, levels, tables, C, loss_weights=weights, out=out)


class _LqFn(torch.autograd.Function):
    """z [B, P, C * d] fp32 (any strides) -> codes laid out as z, idx [B, P, C] int32, and with weights the fused loss
    w_c * m + w_q * m, m = mean (codes - z)^2 (a 0-dim tensor; else None).  The straight-through value passes the upstream
    gradient on; the two loss terms add (g_loss * 2 / numel * (w_c - w_q)) * (codes - z)."""

    @staticmethod
    def forward(ctx, z, levels, tables, C, weights):
        zd = z.detach()
        out = torch.empty_like(zd)
        out, idx, loss = _quantize_call(zd, levels, tables, C, weights, out)
        ctx.weights = weights
        ctx.mark_non_differentiable(idx)
        if weights is None or weights[0] == weights[1]:
            return out, idx, (None if loss is None else loss[0])
        ctx.save_for_backward(z, out)
        return out, idx, loss[0]

    @staticmethod
    def backward(ctx, g_out, g_idx, g_loss):
        weights = ctx.weights
        if weights is None or weights[0] == weights[1]:
            return g_out, None, None, None, None
        z, out = ctx.saved_tensors
        coef = 2.0 / z.numel() * (weights[0] - weights[1])
        if _compiling():
            gz = torch.ops.vq_mi355x.lq_backward(z.detach(), out, g_out, g_loss, coef)
        else:
            gz = native.lq_backward(z.detach(), out, g_out, g_loss, coef)
        return gz, None, None, None, None


def fused_quantize(z: Tensor, levels, tables: Tensor, num_codebooks: int = 1, weights=None):
    """The fused pass over z [B, P, C * d]: (codes laid out as z, idx [B, P, C] int32, fused loss (0-dim) or None)."""
    if torch.is_grad_enabled() and z.requires_grad:
        return _LqFn.apply(z, tuple(levels), tables, num_codebooks, weights)
    out, idx, loss = _quantize_call(z, levels, tables, num_codebooks, weights, torch.empty_like(z))
    return out, idx, (None if loss is None else loss[0])


class LatentQuantize(Module):
    """Latent quantization module (the reference's constructor arguments, attributes, methods and return tuple)."""

    def __init__(
        self,
        levels: list[int] | int,
        dim: int,
        commitment_loss_weight: float | None = 0.1,
        quantization_loss_weight: float | None = 0.1,
        num_codebooks: int = 1,
        codebook_dim: int = -1,
        keep_num_codebooks_dim: bool | None = None,
        optimize_values: bool | None = True,
        in_place_codebook_optimizer: Callable[..., Optimizer] = None,
    ):
        """levels: the number of values per latent dimension (an int is repeated codebook_dim times); dim: the input's
        feature dimension, the input being [B, dim, ...]; optimize_values: keep the value tables as parameters."""
        super().__init__()

        self.dim = dim
        self.in_place_codebook_optimizer = in_place_codebook_optimizer
        _levels = torch.tensor(levels, dtype=int32)

        # if levels is an int, use it for all codebooks (codebook_dim = -1 raises RuntimeError, as the reference)
        if isinstance(levels, int):
            _levels = _levels.repeat(codebook_dim)
        if _levels.numel() < 1 or int(_levels.min()) < 2:
            raise ValueError(f"LatentQuantize: every level must be >= 2 (got {levels})")
        self._level_values = tuple(int(v) for v in _levels.tolist())

        self.register_buffer("commitment_loss_weight", torch.tensor(commitment_loss_weight, dtype=torch.float32),
                             persistent=False)
        self.register_buffer("quantization_loss_weight", torch.tensor(quantization_loss_weight, dtype=torch.float32),
                             persistent=False)
        self.register_buffer("_levels", _levels, persistent=False)

        _basis = torch.cumprod(torch.concat([torch.tensor([1], dtype=int32), _levels[:-1]], dim=0), dim=0)
        self.register_buffer("_basis", _basis, persistent=False)

        self.codebook_dim = codebook_dim if codebook_dim > 0 else len(_levels)

        effective_codebook_dim = self.codebook_dim * num_codebooks
        self.num_codebooks = num_codebooks
        self.effective_codebook_dim = effective_codebook_dim

        keep_num_codebooks_dim = keep_num_codebooks_dim if keep_num_codebooks_dim else num_codebooks > 1
        assert not (num_codebooks > 1 and not keep_num_codebooks_dim)
        self.keep_num_codebooks_dim = keep_num_codebooks_dim

        has_projections = self.dim != effective_codebook_dim
        self.project_in = nn.Linear(self.dim, effective_codebook_dim) if has_projections else nn.Identity()
        self.project_out = nn.Linear(effective_codebook_dim, self.dim) if has_projections else nn.Identity()
        self.has_projections = has_projections

        self.codebook_size = self._levels.prod().item()

        # [K, d], what the reference builds for num_codebooks = 1 (its constructor raises for the other settings)
        implicit_codebook = self._indices_to_codes(torch.arange(self.codebook_size))
        self.register_buffer("implicit_codebook", implicit_codebook, persistent=False)

        # ensure zero is in the middle and start is always -0.5
        values_per_latent = [
            torch.linspace(-0.5, 0.5, level) if level % 2 == 1 else torch.arange(level) / level - 0.5
            for level in _levels
        ]

        if optimize_values:
            self.values_per_latent = nn.ParameterList([nn.Parameter(values) for values in values_per_latent])
            if in_place_codebook_optimizer is not None:
                self.in_place_codebook_optimizer = in_place_codebook_optimizer(self.values_per_latent)
        else:
            self.values_per_latent = values_per_latent

    # ---------------------------------------------------------------------------------------------------------------
    # cached per-device constants
    # ---------------------------------------------------------------------------------------------------------------
    def _tables_on(self, device) -> list[Tensor]:
        """The value tables on `device` (the parameters themselves when they live there; for the plain-list mode a copy,
        refreshed when the list's tensors or the device change)."""
        tables = list(self.values_per_latent)
        if all(t.device == device for t in tables):
            return tables
        key = (device, tuple((id(t), t._version) for t in tables))
        cache = self.__dict__.get("_device_tables_cache")
        if cache is None or cache[0] != key:
            cache = (key, [t.detach().to(device) for t in tables])
            self.__dict__["_device_tables_cache"] = cache
        return cache[1]

    def _flat_tables(self, tables: list[Tensor]) -> Tensor:
        """The tables back to back as the kernel reads them, kept until one of them changes."""
        if _compiling():
            return torch.cat([t.detach() for t in tables])
        key = tuple((t.data_ptr(), t._version) for t in tables)
        cache = self.__dict__.get("_flat_tables_cache")
        if cache is None or cache[0] != key:
            cache = (key, torch.cat([t.detach() for t in tables]).contiguous())
            self.__dict__["_flat_tables_cache"] = cache
        return cache[1]

    def _host_weights(self) -> tuple[float, float]:
        """The two loss weights' fp32 values on the host (one read per change of the buffers)."""
        w_c, w_q = self.commitment_loss_weight, self.quantization_loss_weight
        if _compiling():
            return float(w_c), float(w_q)
        key = (w_c.data_ptr(), w_c._version, w_q.data_ptr(), w_q._version)
        cache = self.__dict__.get("_host_weights_cache")
        if cache is None or cache[0] != key:
            cache = (key, (float(w_c), float(w_q)))
            self.__dict__["_host_weights_cache"] = cache
        return cache[1]

    # ---------------------------------------------------------------------------------------------------------------
    # the reference's methods
    # ---------------------------------------------------------------------------------------------------------------
    def quantization_loss(self, z: Tensor, zhat: Tensor, reduce="mean") -> Tensor:
        """Computes the quantization loss."""
        return F.mse_loss(zhat.detach(), z, reduction=reduce)

    def commitment_loss(self, z: Tensor, zhat: Tensor, reduce="mean") -> Tensor:
        """Computes the commitment loss."""
        return F.mse_loss(z.detach(), zhat, reduction=reduce)

    def quantize(self, z: Tensor) -> Tensor:
        """Quantizes z (..., d) per latent dimension to the closest value of that dimension's table (the first one on a
        tie), with straight-through gradients; same shape as z."""
        tables = self._tables_on(z.device)
        index = torch.stack(
            [torch.argmin(torch.abs(z[..., i, None] - tables[i]), dim=-1) for i in range(self.codebook_dim)], dim=-1)
        quantize = torch.stack([tables[i][index[..., i]] for i in range(self.codebook_dim)], dim=-1)
        return z + (quantize - z).detach()

    def _scale_and_shift(self, zhat_normalized: Tensor) -> Tensor:
        """scale and shift zhat from [-0.5, 0.5] to [0, level_per_dim]"""
        half_width = self._levels // 2
        return (zhat_normalized * 2 * half_width) + half_width

    def _scale_and_shift_inverse(self, zhat: Tensor) -> Tensor:
        """normalize zhat to [-0.5, 0.5]"""
        half_width = self._levels // 2
        return (zhat - half_width) / half_width / 2

    def codes_to_indices(self, zhat: Tensor) -> Tensor:
        """Converts a `code` which contains the number per latent to an index in the codebook."""
        assert zhat.shape[-1] == self.codebook_dim
        zhat = self._scale_and_shift(zhat)
        terms = zhat * self._basis
        if terms.is_cuda and terms.dtype == torch.float32 and terms.shape[-1] <= 7:
            # torch's GPU sum chooses its order by shape and strides (d = 6 with three codebooks on channel-first rows
            # gave other indices than the same codes laid out otherwise); the reference's values are those of torch's
            # CPU order, which for fp32 and d <= 7 is term 0, terms 4 .. d - 1, then terms 1, 2, 3 (DESIGN.md section
            # 12).  Other dtypes keep torch.sum: it accumulates bf16 / fp16 in fp32 and rounds once, which a chain of
            # half-precision additions would not, and the CPU order was established for fp32 only
            t = terms.unbind(dim=-1)
            index = t[0]
            for i in range(4, len(t)):
                index = index + t[i]
            for i in range(1, min(len(t), 4)):
                index = index + t[i]
        else:
            index = terms.sum(dim=-1)
        # NaN -> INT32_MIN, what the reference's CPU cast gives (a GPU cast does not promise it)
        return torch.where(index.isnan(), torch.iinfo(int32).min, index.to(int32))

    def _indices_to_codes(self, indices: Tensor) -> Tensor:
        """indices (...) -> codes (..., d) on the uniform grid (k - hw) / hw / 2 (the learned tables are not used, as in
        the reference)."""
        levels = self._level_values
        if (indices.is_cuda and not _compiling() and indices.dtype in (torch.int32, torch.int64)
                and 1 <= len(levels) <= native.FSQ_MAX_DIM and indices.numel() > 0):
            halves = torch.full((1, len(levels)), 0.5, dtype=torch.float32, device=indices.device)
            codes, _ = native.fsq_decode(indices.reshape(-1, 1), levels, halves)
            return codes.reshape(*indices.shape, len(levels))
        indices = indices[..., None]
        codes_non_centered = (indices // self._basis) % self._levels
        return self._scale_and_shift_inverse(codes_non_centered)

    def indices_to_codes(self, indices: Tensor, project_out=True) -> Tensor:
        """Inverse of `codes_to_indices`."""
        codes = self._indices_to_codes(indices)

        if self.keep_num_codebooks_dim:
            codes = codes.reshape(*codes.shape[:-2], codes.shape[-2] * codes.shape[-1])

        if project_out:
            codes = self.project_out(codes)

        return codes.movedim(-1, 1)

    def quantize_and_project(self, z: Tensor, is_img_or_video, ps) -> Tensor:
        """z [b, n, c, d] -> (codes [b, n, c * d], out [b, dim, *ps], indices [b, *ps(, c)]); ps the packed spatial shape."""
        codes = self.quantize(z)
        indices = self.codes_to_indices(codes)
        b, n = codes.shape[0], codes.shape[1]
        codes = codes.reshape(b, n, self.effective_codebook_dim)
        out = self.project_out(codes)
        out = out.reshape(b, *ps, out.shape[-1]).movedim(-1, 1)
        indices = indices.reshape(b, *ps, self.num_codebooks)
        if not self.keep_num_codebooks_dim:
            indices = indices.squeeze(-1)
        return codes, out, indices

    def forward(self, z: Tensor) -> tuple[Tensor, Tensor, Tensor]:
        """z [b, dim, ...] -> (out of the same shape, indices [b, ...] int32 (a trailing codebook dim when
        keep_num_codebooks_dim), loss: 0-dim, in training commitment_loss_weight * mse(z.detach(), out) +
        quantization_loss_weight * mse(out.detach(), z), else 0)."""
        with torch.autocast(device_type="cuda", enabled=False):
            return self._forward(z, fused=True)

    def _loss(self, original_input: Tensor, out: Tensor) -> Tensor:
        """The reference's loss lines (torch)."""
        commitment_loss = (self.commitment_loss(original_input, out)
                           if self.training and self.commitment_loss_weight != 0 else torch.tensor(0.0))
        quantization_loss = (self.quantization_loss(original_input, out)
                             if self.training and self.quantization_loss_weight != 0 else torch.tensor(0.0))
        return self.commitment_loss_weight * commitment_loss + self.quantization_loss_weight * quantization_loss

    def _eval_loss(self, original_input: Tensor, out: Tensor) -> Tensor:
        """The reference's eval loss w_c * 0 + w_q * 0: a fresh zero unless a weight is not finite."""
        if _compiling() or not all(w == w and abs(w) != float("inf") for w in self._host_weights()):
            return self._loss(original_input, out)
        return self.commitment_loss_weight.new_zeros(())

    def _forward(self, z: Tensor, fused: bool):
        if self.in_place_codebook_optimizer is not None and self.training:
            raise NotImplementedError(
                "LatentQuantize: the in-place codebook optimizer step of a training forward is not implemented (the "
                "reference's reads self.optimize_values, which it never sets, and raises AttributeError)")
        if not (z.is_cuda or _compiling()):
            native._require_gpu(z)
        original_input = z
        b = z.shape[0]
        ps = tuple(z.shape[2:])
        assert z.dim() >= 2 and z.shape[1] == self.dim, f"expected dimension of {self.dim} but found dimension of {z.shape[1]}"

        tables = self._tables_on(z.device) if (z.is_cuda or not _compiling()) else list(self.values_per_latent)
        C, d = self.num_codebooks, self.codebook_dim
        if fused and not self.has_projections and _fused_ok(z, self._level_values, tables):
            # the caller's channel-first tensor as it lies: [b, dim, P] seen as [b, P, dim]
            z3 = z.reshape(b, self.dim, -1).transpose(1, 2)
            weights = self._host_weights() if self.training else None
            out3, indices, loss = fused_quantize(z3, self._level_values, self._flat_tables(tables), C, weights)
            out = out3.transpose(1, 2).reshape(z.shape)
            if loss is None:
                loss = self._eval_loss(original_input, out)
            indices = indices.reshape(b, *ps, C)
            if not self.keep_num_codebooks_dim:
                indices = indices.squeeze(-1)
            return out, indices, loss

        z = z.movedim(1, -1).reshape(b, -1, self.dim)  # "b d ... -> b ... d", pack "b * d"
        z = self.project_in(z)
        n = z.shape[1]

        if fused and _fused_ok(z, self._level_values, tables):
            codes, indices, _ = fused_quantize(z, self._level_values, self._flat_tables(tables), C, None)
        else:
            z = z.reshape(b, n, C, d)
            codes = self.quantize(z)
            indices = self.codes_to_indices(codes)
            codes = codes.reshape(b, n, C * d)

        out = self.project_out(codes)
        out = out.reshape(b, *ps, out.shape[-1]).movedim(-1, 1)

        indices = indices.reshape(b, *ps, C)
        if not self.keep_num_codebooks_dim:
            indices = indices.squeeze(-1)

        return out, indices, self._loss(original_input, out)
