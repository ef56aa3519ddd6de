"""Lookup-free quantization (LFQ, https://arxiv.org/abs/2310.05737), the reference's ``LFQ``
(``vector_quantization/lookup_free_quantization.py:31-397``) with its sweeps in HIP:

- the quantize step (signs -> +-a, int64 indices MSB first, straight-through value, commitment squared-error sum) is
  ``vq_lfq_quantize_f32``, one pass over the rows;
- the decode side, ``indices_to_codes``, is ``vq_lfq_decode_f32``: the codes of every codebook from the index bits in one
  pass, written side by side (device int32 / int64 indices; ``VQ_NO_FUSED_DECODE=1`` and CPU indices keep the tensor ops);
- the entropy aux loss is ``vq_lfq_entropy_fwd_f32`` / ``vq_lfq_entropy_bwd_f32``.  The reference builds the
  ``[rows, 2^d]`` softmax several times over; here the softmax over ``{+-a}^d`` is factorised per dim
  (``p_k = A_u * B_w``, two tables of at most 1024 entries per row), so no buffer grows with ``rows * 2^d``.

Everything that is not a sweep (projections, soft clamp, l2norm, packing, the scalar loss arithmetic, ``maybe_distributed_mean``)
composes in torch around the kernels.  There is no CPU fallback: CPU tensors raise ``native.NativeUnavailable``.
The product form rounds differently from the reference's fp32 softmax: losses and gradients agree to tolerance, indices
and quantized values bit for bit.
"""
from __future__ import annotations

from collections import namedtuple
from functools import partial
from math import ceil, log2, prod

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from . import native, search

Return = namedtuple("Return", ["quantized", "indices", "entropy_aux_loss"])

LossBreakdown = namedtuple("LossBreakdown", ["per_sample_entropy", "batch_entropy", "commitment"])

MAX_CODEBOOK_DIM = native.LFQ_MAX_DIM
_EPS = 1e-5  # the reference's log clamp (utils/general.py:25-26)


def _exists(v):
    return v is not None


def _l2norm(t):
    return F.normalize(t, p=2, dim=-1)


def _entropy(prob):
    return (-prob * prob.clamp(min=_EPS).log()).sum(dim=-1)


def _world_size() -> int:
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


def _maybe_distributed_mean(t):
    """utils/distributed.py:86-92: all_reduce, then divide by the world size (no autograd through the collective)."""
    world = _world_size()
    if world <= 1:
        return t, 1
    dist.all_reduce(t)
    return t / world, world


class CosineSimLinear(nn.Module):
    def __init__(self, dim_in, dim_out, scale=1.0):
        super().__init__()
        self.scale = scale
        self.weight = nn.Parameter(torch.randn(dim_in, dim_out))

    def forward(self, x):
        x = F.normalize(x, dim=-1)
        w = F.normalize(self.weight, dim=0)
        return (x @ w) * self.scale


class _LfqQuantize(torch.autograd.Function):
    """(v, xa) -> straight-through out = xa + (q - xa), q, idx, commitment squared-error sum (float64).
    Gradients: out -> xa unchanged; the sum -> v as 2 (v - q) on the rows the mask keeps (q is detached)."""

    @staticmethod
    def forward(ctx, v, xa, qmag, mask, want_commit):
        q, out, idx, commit = native.lfq_quantize(v.detach(), qmag, xa=xa.detach(), mask=mask, want_commit=want_commit)
        if commit is None:
            commit = torch.zeros((), dtype=torch.float64, device=v.device)
        ctx.save_for_backward(v, q, mask)
        ctx.mark_non_differentiable(q, idx)
        return out, q, idx, commit

    @staticmethod
    def backward(ctx, g_out, g_q, g_idx, g_commit):
        v, q, mask = ctx.saved_tensors
        g_v = None
        if ctx.needs_input_grad[0] and g_commit is not None:
            g_v = (v.detach() - q) * (2.0 * g_commit.to(torch.float32))
            if mask is not None:
                g_v = g_v * mask.reshape(-1, 1, 1).to(g_v.dtype)
        return g_v, g_out, None, None, None


class _LfqEntropy(torch.autograd.Function):
    """v [N, C, d] (+ the selected rows) -> (per-sample entropy, codebook entropy), both fp32 scalars
    (lookup_free_quantization.py:294-331 of the reference)."""

    @staticmethod
    def forward(ctx, v, rows, code_scale, inv_temperature):
        N, C, d = v.shape
        R = N if rows is None else int(rows.numel())
        ps_sum, avg_prob = native.lfq_entropy_forward(v.detach(), rows, code_scale, inv_temperature)
        avg_prob, world = _maybe_distributed_mean(avg_prob)
        per_sample = (ps_sum / (R * C)).to(torch.float32)
        codebook = _entropy(avg_prob).mean()
        ctx.save_for_backward(v, rows if rows is not None else torch.empty(0), avg_prob)
        ctx.meta = (rows is not None, R, C, world, code_scale, inv_temperature)
        return per_sample, codebook

    @staticmethod
    def backward(ctx, g_ps, g_cb):
        v, rows, avg_prob = ctx.saved_tensors
        has_rows, R, C, world, code_scale, inv_temperature = ctx.meta
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        dev = v.device
        if g_ps is None:
            g_ps = torch.zeros((), dtype=torch.float32, device=dev)
        if g_cb is None:
            g_cb = torch.zeros((), dtype=torch.float32, device=dev)
        w_ps = g_ps.to(torch.float32) / (R * C)
        # d/dx of -x log(max(x, eps)): -(log x + 1) above the clamp, -log eps below it
        dh = -(avg_prob.clamp(min=_EPS).log() + (avg_prob >= _EPS).to(avg_prob.dtype))
        w_cb = dh * (g_cb.to(torch.float32) / (C * R * world))
        g_v = native.lfq_entropy_backward(v.detach(), rows if has_rows else None, code_scale, inv_temperature, w_ps, w_cb)
        return g_v, None, None, None


def _rows_view(x: torch.Tensor, C: int, d: int) -> torch.Tensor:
    """[..., C * d] -> [N, C, d] whose rows keep their C * d values contiguous (copy only when they do not)."""
    v = x.reshape(-1, C, d)
    if v.shape[0] > 1 and not (v.stride(2) == 1 and v.stride(1) == d):
        v = v.contiguous()
    return v


class LFQ(nn.Module):
    def __init__(
        self,
        *,
        dim=None,
        codebook_size=None,
        entropy_loss_weight=0.1,
        commitment_loss_weight=0.25,
        diversity_gamma=1.0,
        straight_through_activation=nn.Identity(),
        num_codebooks=1,
        keep_num_codebooks_dim=None,
        codebook_scale=1.0,
        frac_per_sample_entropy=1.0,
        has_projections=None,
        projection_has_bias=True,
        soft_clamp_input_value=None,
        cosine_sim_project_in=False,
        cosine_sim_project_in_scale=None,
        channel_first=False,
        experimental_softplus_entropy_loss=False,
        entropy_loss_offset=5.0,
        spherical=False,
    ):
        super().__init__()
        assert _exists(dim) or _exists(codebook_size), "either dim or codebook_size must be specified for LFQ"
        assert (
            not _exists(codebook_size) or log2(codebook_size).is_integer()
        ), f"your codebook size must be a power of 2 for lookup free quantization (suggested {2 ** ceil(log2(codebook_size))})"

        codebook_size = codebook_size if codebook_size is not None else 2**dim
        self.codebook_size = codebook_size
        codebook_dim = int(log2(codebook_size))
        if codebook_dim > MAX_CODEBOOK_DIM:
            raise ValueError(
                f"LFQ: codebook_dim {codebook_dim} (codebook_size 2^{codebook_dim}) exceeds the native limit of "
                f"{MAX_CODEBOOK_DIM} bits per codebook"
            )
        codebook_dims = codebook_dim * num_codebooks
        dim = dim if dim is not None else codebook_dims

        has_projections = has_projections if has_projections is not None else (dim != codebook_dims)
        if cosine_sim_project_in:
            # (the reference's expression: the flag itself, True, becomes the scale)
            cosine_sim_project_in = cosine_sim_project_in if cosine_sim_project_in is not None else codebook_scale
            project_in_klass = partial(CosineSimLinear, scale=cosine_sim_project_in)
        else:
            project_in_klass = partial(nn.Linear, bias=projection_has_bias)

        self.project_in = project_in_klass(dim, codebook_dims) if has_projections else nn.Identity()
        self.project_out = nn.Linear(codebook_dims, dim, bias=projection_has_bias) if has_projections else nn.Identity()
        self.has_projections = has_projections

        self.dim = dim
        self.codebook_dim = codebook_dim
        self.num_codebooks = num_codebooks

        keep_num_codebooks_dim = keep_num_codebooks_dim if keep_num_codebooks_dim is not None else (num_codebooks > 1)
        assert not (num_codebooks > 1 and not keep_num_codebooks_dim)
        self.keep_num_codebooks_dim = keep_num_codebooks_dim

        self.channel_first = channel_first
        self.activation = straight_through_activation
        self.spherical = spherical

        assert 0 < frac_per_sample_entropy <= 1.0
        self.frac_per_sample_entropy = frac_per_sample_entropy
        self.diversity_gamma = diversity_gamma
        self.entropy_loss_weight = entropy_loss_weight
        self.codebook_scale = codebook_scale
        self.commitment_loss_weight = commitment_loss_weight

        self.soft_clamp_input_value = soft_clamp_input_value
        assert not _exists(soft_clamp_input_value) or soft_clamp_input_value >= codebook_scale

        self.entropy_loss_offset = entropy_loss_offset
        self.experimental_softplus_entropy_loss = experimental_softplus_entropy_loss

        self.register_buffer("mask", 2 ** torch.arange(codebook_dim - 1, -1, -1))
        self.register_buffer("zero", torch.tensor(0.0), persistent=False)

        # Magnitude of every entry of a code: +-scale, or for spherical codes l2norm(+-scale) * scale (all |entries| equal,
        # so one fp32 value).  The reference's codebook buffer [2^d, d] is not materialised (see `codebook`).
        ones = torch.full((1, codebook_dim), float(codebook_scale), dtype=torch.float32)
        self._code_mag = float(self.maybe_l2norm(ones)[0, 0]) if spherical else float(ones[0, 0])

    def maybe_l2norm(self, t):
        return _l2norm(t) * self.codebook_scale if self.spherical else t

    def bits_to_codes(self, bits):
        return bits * self.codebook_scale * 2 - self.codebook_scale

    @property
    def codebook(self):
        """The reference's codebook buffer, [2^d, d] (built on demand: it is 80 MB at d = 20)."""
        all_codes = torch.arange(self.codebook_size, device=self.mask.device)
        bits = ((all_codes[..., None].int() & self.mask) != 0).to(self.dtype)
        return self.bits_to_codes(bits)

    @property
    def dtype(self):
        return self.zero.dtype

    def indices_to_codes(self, indices, project_out=True):
        should_transpose = self.channel_first
        if not self.keep_num_codebooks_dim:
            indices = indices[..., None]
        decode = search.lfq_decode_backend(indices) if self.dtype == torch.float32 else None
        if decode is not None:
            # one pass (vq_lfq_decode_f32): the codebooks are the kernel's group axis, their codes land side by side
            C, d = self.num_codebooks, self.codebook_dim
            lead = indices.shape[:-1]
            flat = indices.reshape(prod(lead), C)
            if torch.compiler.is_compiling():  # (the registered op returns fresh tensors)
                codes = decode(flat.t()[..., None], (self._code_mag,), d, drop_null=False)[0].transpose(0, 1)
            else:
                codes = torch.empty((flat.shape[0], C * d), dtype=torch.float32, device=indices.device)
                decode(flat.t()[..., None], (self._code_mag,), d, drop_null=False,
                       sum_out=codes.view(flat.shape[0], C, d).transpose(0, 1))
            codes = codes.reshape(*lead, C * d)
        else:
            bits = ((indices[..., None].int() & self.mask) != 0).to(self.dtype)
            codes = self.maybe_l2norm(self.bits_to_codes(bits))
            codes = codes.reshape(*codes.shape[:-2], -1)
        if project_out:
            codes = self.project_out(codes)
        if should_transpose:
            codes = codes.movedim(-1, 1)
        return codes

    def _entropy_rows(self, N: int, mask, device):
        """Row selection of the entropy terms: prob[mask] first, then the reference's CPU-generator draw for
        frac_per_sample_entropy < 1 (lookup_free_quantization.py:304-318).  None = all rows."""
        rows = None
        if mask is not None:
            rows = mask.reshape(-1).to(device).nonzero().squeeze(1)
        if self.frac_per_sample_entropy < 1.0:
            num_tokens = N if rows is None else int(rows.numel())
            num_sampled_tokens = int(num_tokens * self.frac_per_sample_entropy)
            rand_mask = torch.randn(num_tokens).argsort(dim=-1) < num_sampled_tokens
            picked = rand_mask.nonzero().squeeze(1).to(device)
            rows = picked if rows is None else rows[picked]
        return rows

    @torch.autocast(device_type="cuda", enabled=False)
    def forward(self, x, inv_temperature=100.0, return_loss_breakdown=False, mask=None):
        x = x.float()
        is_img_or_video = x.ndim >= 4

        if self.channel_first:
            x = x.movedim(1, -1)
        if is_img_or_video:
            spatial = x.shape[1:-1]
            x = x.reshape(x.shape[0], -1, x.shape[-1])

        assert x.shape[-1] == self.dim, f"expected dimension of {self.dim} but received {x.shape[-1]}"

        x = self.project_in(x)
        if _exists(self.soft_clamp_input_value):
            clamp_value = self.soft_clamp_input_value
            x = (x / clamp_value).tanh() * clamp_value

        b, n = x.shape[0], x.shape[1]
        C, d = self.num_codebooks, self.codebook_dim
        x = x.reshape(b, n, C, d)
        x = self.maybe_l2norm(x)
        v = _rows_view(x, C, d)  # original_input, [b * n, C, d]
        native._require_gpu(v)

        want_commit = self.training and self.commitment_loss_weight > 0.0
        if self.training:
            xa = _rows_view(self.activation(v), C, d)
            out, _, indices, commit_sum = _LfqQuantize.apply(v, xa, self._code_mag, mask, want_commit)
        else:
            out, _, indices, _ = native.lfq_quantize(v.detach(), self._code_mag)  # eval: out is q itself

        if self.training:
            rows = self._entropy_rows(v.shape[0], mask, v.device)
            per_sample_entropy, codebook_entropy = _LfqEntropy.apply(v, rows, self._code_mag, float(inv_temperature))
            entropy_aux_loss = per_sample_entropy - self.diversity_gamma * codebook_entropy
        else:
            entropy_aux_loss = per_sample_entropy = codebook_entropy = self.zero

        if self.training and self.experimental_softplus_entropy_loss:
            entropy_aux_loss = F.softplus(entropy_aux_loss + self.entropy_loss_offset)

        if want_commit:
            kept = b * n if mask is None else mask.sum()
            commit_loss = (commit_sum / (kept * C * d)).to(torch.float32)
        else:
            commit_loss = self.zero

        x = out.reshape(b, n, C * d)
        x = self.project_out(x)
        indices = indices.reshape(b, n, C)

        if is_img_or_video:
            x = x.reshape(b, *spatial, x.shape[-1])
            indices = indices.reshape(b, *spatial, C)
        if self.channel_first:
            x = x.movedim(-1, 1)
        if not self.keep_num_codebooks_dim:
            indices = indices[..., 0]

        aux_loss = entropy_aux_loss * self.entropy_loss_weight + commit_loss * self.commitment_loss_weight
        ret = Return(x, indices, aux_loss)
        if not return_loss_breakdown:
            return ret
        return ret, LossBreakdown(per_sample_entropy, codebook_entropy, commit_loss)
