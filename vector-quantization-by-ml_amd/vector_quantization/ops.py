"""``torch.library`` registration of the native op ("registered to PyTorch as ``torch.ops.<ns>.vq_nearest``").

The transport stays the C ABI over ctypes (``native.py``); these are the *same* calls given a dispatcher identity and a
fake (meta) implementation, so that ``torch.compile`` / ``torch.export`` can trace a module forward THROUGH the search
instead of breaking the graph at an opaque Python call:

    torch.ops.vq_mi355x.pack(cb, metric) -> packed images
    torch.ops.vq_mi355x.quantize_into(x, cb, packed, out, idx, metric, ste, want_sq_err, share, per_head) -> sq_err
        (writes the quantized rows and the indices into the caller's -- possibly strided -- ``out`` / ``idx`` views)
    torch.ops.vq_mi355x.gumbel_sample(x, cb, packed, seed, metric, tau) -> idx [H, M]   (Gumbel-max sampling, native.sample_codes)
    torch.ops.vq_mi355x.expire_codes(cluster_size, embed_avg, embeddings, pool, chain_x, chain_codes, chain_idx, stage,
        threshold, reset_cluster_size, l2norm, seed) -> picked [H, K]   (dead-code expiry on the device, native.expire_codes;
        mutates the three buffers)
    torch.ops.vq_mi355x.residual_mask(x, cb, idx, mask, zero_idx, out, train, want_sq_err, per_group) -> sq_err
        (the mask pass of a residual stack, native.residual_mask; rewrites ``idx`` on masked-out rows and writes ``out``)
    torch.ops.vq_mi355x.lfq_quantize / lfq_entropy_fwd / lfq_entropy_bwd   (lookup-free quantization, native.lfq_*)
    torch.ops.vq_mi355x.rlfq_quantize / rlfq_backward / lfq_entropy_staged_fwd / lfq_entropy_staged_bwd
        (residual LFQ, native.rlfq_* and native.lfq_entropy_staged_*)
    torch.ops.vq_mi355x.fsq_quantize / fsq_backward / fsq_decode   (finite scalar quantization, native.fsq_*)
    torch.ops.vq_mi355x.lfq_decode(indices, mag, d, drop_null, want_sum, want_all) -> (codes_sum, all_codes)
        (indices -> code vectors of the lookup-free family, native.lfq_decode)
    torch.ops.vq_mi355x.lq_quantize / lq_backward   (latent quantization, native.lq_*)
    torch.ops.vq_mi355x.decode_codes(cb, indices, num_stages, drop_null, want_sum, want_all) -> (codes_sum, all_codes)
        (indices -> code vectors, native.decode_codes; differentiable with respect to cb)

Eager forwards keep calling ``native.quantize`` directly (a custom-op dispatch costs tens of microseconds of host time,
which is most of a small launch); the modules switch to these ops only while being compiled
(``torch.compiler.is_compiling()``).  There is still no CPU implementation: the real kernels raise on CPU tensors.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import native

_LIB_NS = "vq_mi355x"


@torch.library.custom_op(f"{_LIB_NS}::pack", mutates_args=())
def pack(cb: torch.Tensor, metric: int) -> torch.Tensor:
    return native.pack_codebooks(cb.contiguous(), metric)


@pack.register_fake
def _(cb, metric):
    k, d = cb.shape[-2], cb.shape[-1]
    n = cb.numel() // max(1, k * d)
    return cb.new_empty((n, native.packed_floats(int(k), int(d))))


@torch.library.custom_op(f"{_LIB_NS}::quantize_into", mutates_args=("out", "idx"))
def quantize_into(x: torch.Tensor, cb: torch.Tensor, packed: Optional[torch.Tensor], out: torch.Tensor, idx: torch.Tensor,
                  metric: int, ste: bool, want_sq_err: bool, share: bool, per_head: bool) -> torch.Tensor:
    """x [H, M, D], cb [H, Q|1, K, D], out [H, M, D] / idx [H, M, Q] destination views -> sq_err ([Q] or [H, Q] float64;
    zeros when not requested)."""
    r = native.quantize(x, cb, metric=metric, ste=ste, want_sq_err=want_sq_err, want_best=False, packed=packed,
                        stages_share_codebook=share, out=out, idx=idx, sq_err_per_head=per_head)
    if r["sq_err"] is not None:
        return r["sq_err"]
    q = idx.shape[-1]
    return torch.zeros((x.shape[0], q) if per_head else (q,), dtype=torch.float64, device=x.device)


@quantize_into.register_fake
def _(x, cb, packed, out, idx, metric, ste, want_sq_err, share, per_head):
    q = idx.shape[-1]
    return x.new_empty((x.shape[0], q) if per_head else (q,), dtype=torch.float64)


@torch.library.custom_op(f"{_LIB_NS}::gumbel_sample", mutates_args=())
def gumbel_sample(x: torch.Tensor, cb: torch.Tensor, packed: Optional[torch.Tensor], seed: torch.Tensor, metric: int,
                  tau: float) -> torch.Tensor:
    """x [H, M, D] (D <= 512), cb [H, K, D], seed [2] int64 -> idx [H, M] int64: argmax_k of similarity * tau + Gumbel noise."""
    idx = native.sample_codes(x, cb, metric=metric, tau=tau, seed=seed, packed=packed)
    if idx is None:
        raise RuntimeError("vq_gumbel_sample_f32: rows wider than 512 dims are not supported")
    return idx


@gumbel_sample.register_fake
def _(x, cb, packed, seed, metric, tau):
    return x.new_empty((x.shape[0], x.shape[1]), dtype=torch.int64)


@torch.library.custom_op(f"{_LIB_NS}::expire_codes", mutates_args=("cluster_size", "embed_avg", "embeddings"))
def expire_codes(cluster_size: torch.Tensor, embed_avg: torch.Tensor, embeddings: torch.Tensor, pool: Optional[torch.Tensor],
                 chain_x: Optional[torch.Tensor], chain_codes: Optional[torch.Tensor], chain_idx: Optional[torch.Tensor],
                 stage: int, threshold: float, reset_cluster_size: float, l2norm: bool, seed: torch.Tensor) -> torch.Tensor:
    """Dead-code expiry on the device, in place on the three buffers (native.expire_codes); the pool is ``pool`` [H | 1, N, D]
    or the stage-``stage`` residual of the chain (x [M, D], codes [Q | 1, K, D], idx [M, Q]) -> picked [H, K] int64."""
    chain = None if chain_x is None else (chain_x, chain_codes, chain_idx)
    return native.expire_codes(cluster_size, embed_avg, embeddings, pool, chain=chain, stage=stage, threshold=threshold,
                               reset_cluster_size=reset_cluster_size, l2norm=l2norm, seed=seed, want_picked=True)[1]


@expire_codes.register_fake
def _(cluster_size, embed_avg, embeddings, pool, chain_x, chain_codes, chain_idx, stage, threshold, reset_cluster_size, l2norm, seed):
    return cluster_size.new_empty(cluster_size.shape, dtype=torch.int64)


@torch.library.custom_op(f"{_LIB_NS}::residual_mask", mutates_args=("idx", "out"))
def residual_mask(x: torch.Tensor, cb: torch.Tensor, idx: torch.Tensor, mask: torch.Tensor, zero_idx: torch.Tensor,
                  out: torch.Tensor, train: bool, want_sq_err: bool, per_group: bool) -> torch.Tensor:
    """The mask pass of a residual stack (native.residual_mask): x [G, M, D], cb [G, Q | 1, K, D], idx [G, M, Q] as the search
    wrote it (rewritten on masked-out rows), mask [M] | [G, M], zero_idx [G, Q]; writes ``out`` [G, M, D] -> sq_err over the
    kept rows ([Q] or [G, Q] float64; zeros when not requested)."""
    _, sq_err = native.residual_mask(x, cb, idx, mask, zero_idx, train=train, want_sq_err=want_sq_err,
                                     sq_err_per_group=per_group, out=out)
    if sq_err is not None:
        return sq_err
    q = idx.shape[-1]
    return torch.zeros((x.shape[0], q) if per_group else (q,), dtype=torch.float64, device=x.device)


@residual_mask.register_fake
def _(x, cb, idx, mask, zero_idx, out, train, want_sq_err, per_group):
    q = idx.shape[-1]
    return x.new_empty((x.shape[0], q) if per_group else (q,), dtype=torch.float64)


# lookup-free quantization (native.lfq_*): the same calls with a dispatcher identity and fake implementations
@torch.library.custom_op(f"{_LIB_NS}::lfq_quantize", mutates_args=())
def lfq_quantize(v: torch.Tensor, xa: Optional[torch.Tensor], qmag: float, mask: Optional[torch.Tensor],
                 want_commit: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """v [N, C, d] -> (q, out, idx [N, C] int64, commitment squared-error sum (float64 scalar; 0 when not requested))."""
    q, out, idx, commit = native.lfq_quantize(v, qmag, xa=xa, mask=mask, want_commit=want_commit)
    if commit is None:
        commit = torch.zeros((), dtype=torch.float64, device=v.device)
    return q, out.clone() if out is q else out, idx, commit


@lfq_quantize.register_fake
def _(v, xa, qmag, mask, want_commit):
    n, c, _ = v.shape
    return (v.new_empty(v.shape), v.new_empty(v.shape), v.new_empty((n, c), dtype=torch.int64),
            v.new_empty((), dtype=torch.float64))


@torch.library.custom_op(f"{_LIB_NS}::lfq_entropy_fwd", mutates_args=())
def lfq_entropy_fwd(v: torch.Tensor, rows: Optional[torch.Tensor], code_scale: float,
                    inv_temperature: float) -> tuple[torch.Tensor, torch.Tensor]:
    """v [N, C, d] -> (sum of the per-sample entropies (float64 scalar), avg_prob [C, 2^d])."""
    return native.lfq_entropy_forward(v, rows, code_scale, inv_temperature)


@lfq_entropy_fwd.register_fake
def _(v, rows, code_scale, inv_temperature):
    return v.new_empty((), dtype=torch.float64), v.new_empty((v.shape[1], 1 << v.shape[2]))


@torch.library.custom_op(f"{_LIB_NS}::lfq_entropy_bwd", mutates_args=())
def lfq_entropy_bwd(v: torch.Tensor, rows: Optional[torch.Tensor], code_scale: float, inv_temperature: float,
                    w_ps: torch.Tensor, w_cb: torch.Tensor) -> torch.Tensor:
    """dL/dv [N, C, d] for L = w_ps * sum of the per-sample entropies + sum_(row, c, k) w_cb[c, k] * p_k."""
    return native.lfq_entropy_backward(v, rows, code_scale, inv_temperature, w_ps, w_cb)


@lfq_entropy_bwd.register_fake
def _(v, rows, code_scale, inv_temperature, w_ps, w_cb):
    return v.new_empty(v.shape)


# residual LFQ (native.rlfq_*, native.lfq_entropy_staged_*).  clamp entries of 0 mean no clamp; outputs that were not
# requested come back as empty tensors (a custom op returns no None).
@torch.library.custom_op(f"{_LIB_NS}::rlfq_quantize", mutates_args=())
def rlfq_quantize(x: torch.Tensor, qmag: list[float], clamp: list[float], scale: list[float], spherical: bool, ste: bool,
                  mask: Optional[torch.Tensor], want_v: bool,
                  want_commit: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """x [G, N, d] -> (out [G, N, d], idx [G, N, S] int64, v_all [G, S, N, d] (or empty), commit sums [G, S] float64 (or empty))."""
    out, idx, v_all, commit = native.rlfq_quantize(x, qmag, clamp, scale, spherical=spherical, ste=ste, mask=mask,
                                                   want_v=want_v, want_commit=want_commit)
    if v_all is None:
        v_all = x.new_empty((0,))
    if commit is None:
        commit = x.new_empty((0,), dtype=torch.float64)
    return out, idx, v_all, commit


@rlfq_quantize.register_fake
def _(x, qmag, clamp, scale, spherical, ste, mask, want_v, want_commit):
    G, N, d = x.shape
    S = len(qmag)
    return (x.new_empty((G, N, d)), x.new_empty((G, N, S), dtype=torch.int64),
            x.new_empty((G, S, N, d) if want_v else (0,)), x.new_empty((G, S) if want_commit else (0,), dtype=torch.float64))


@torch.library.custom_op(f"{_LIB_NS}::rlfq_backward", mutates_args=())
def rlfq_backward(x: torch.Tensor, qmag: list[float], clamp: list[float], scale: list[float], spherical: bool,
                  mask: Optional[torch.Tensor], g_out: Optional[torch.Tensor], w_commit: Optional[torch.Tensor],
                  g_ent: Optional[torch.Tensor]) -> torch.Tensor:
    """dL/dx [G, N, d] of the residual LFQ chain (native.rlfq_backward)."""
    return native.rlfq_backward(x, qmag, clamp, scale, spherical=spherical, mask=mask, g_out=g_out, w_commit=w_commit,
                                g_ent=g_ent)


@rlfq_backward.register_fake
def _(x, qmag, clamp, scale, spherical, mask, g_out, w_commit, g_ent):
    return x.new_empty(x.shape)


@torch.library.custom_op(f"{_LIB_NS}::lfq_entropy_staged_fwd", mutates_args=())
def lfq_entropy_staged_fwd(v: torch.Tensor, rows: Optional[torch.Tensor], code_scale: list[float],
                           inv_temperature: float) -> tuple[torch.Tensor, torch.Tensor]:
    """v [T, N, d] -> (per-sample entropy sums float64 [T], avg_prob [T, 2^d])."""
    return native.lfq_entropy_staged_forward(v, rows, code_scale, inv_temperature)


@lfq_entropy_staged_fwd.register_fake
def _(v, rows, code_scale, inv_temperature):
    T = v.shape[0]
    return v.new_empty((T,), dtype=torch.float64), v.new_empty((T, 1 << v.shape[2]))


@torch.library.custom_op(f"{_LIB_NS}::lfq_entropy_staged_bwd", mutates_args=())
def lfq_entropy_staged_bwd(v: torch.Tensor, rows: Optional[torch.Tensor], code_scale: list[float], inv_temperature: float,
                           w_ps: torch.Tensor, w_cb: torch.Tensor) -> torch.Tensor:
    """dL/dv [T, N, d] of the staged entropy terms (native.lfq_entropy_staged_backward)."""
    return native.lfq_entropy_staged_backward(v, rows, code_scale, inv_temperature, w_ps, w_cb)


@lfq_entropy_staged_bwd.register_fake
def _(v, rows, code_scale, inv_temperature, w_ps, w_cb):
    return v.new_empty(v.shape)


# finite scalar quantization (native.fsq_*).  consts [3 + S, d] as the kernels read them; indices that were not requested
# come back as an empty tensor (a custom op returns no None).
@torch.library.custom_op(f"{_LIB_NS}::fsq_quantize", mutates_args=())
def fsq_quantize(x: torch.Tensor, levels: list[int], consts: torch.Tensor, prebound: bool,
                 want_idx: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """x [G, N, d] -> (out [G, N, d], idx [G, N, S] int32 (or empty))."""
    out, idx = native.fsq_quantize(x, levels, consts, prebound=prebound, want_idx=want_idx)
    if idx is None:
        idx = x.new_empty((0,), dtype=torch.int32)
    return out, idx


@fsq_quantize.register_fake
def _(x, levels, consts, prebound, want_idx):
    G, N, d = x.shape
    S = consts.shape[0] - 3
    return x.new_empty((G, N, d)), x.new_empty((G, N, S) if want_idx else (0,), dtype=torch.int32)


@torch.library.custom_op(f"{_LIB_NS}::fsq_backward", mutates_args=())
def fsq_backward(x: torch.Tensor, levels: list[int], consts: torch.Tensor, prebound: bool, g_out: torch.Tensor) -> torch.Tensor:
    """dL/dx [G, N, d] of fsq_quantize's out (native.fsq_backward)."""
    return native.fsq_backward(x, levels, consts, g_out, prebound=prebound)


@fsq_backward.register_fake
def _(x, levels, consts, prebound, g_out):
    return x.new_empty(x.shape)


@torch.library.custom_op(f"{_LIB_NS}::fsq_decode", mutates_args=())
def fsq_decode(indices: torch.Tensor, levels: list[int], scales: torch.Tensor, drop_null: bool, want_sum: bool,
               want_all: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """indices [N, Q] -> (codes summed over q [N, d] (or empty), all codes [Q, N, d] (or empty))."""
    codes_sum, all_codes = native.fsq_decode(indices, levels, scales, drop_null=drop_null, want_sum=want_sum,
                                             want_all=want_all)
    if codes_sum is None:
        codes_sum = scales.new_empty((0,))
    if all_codes is None:
        all_codes = scales.new_empty((0,))
    return codes_sum, all_codes


@fsq_decode.register_fake
def _(indices, levels, scales, drop_null, want_sum, want_all):
    N, Q = indices.shape
    d = len(levels)
    return scales.new_empty((N, d) if want_sum else (0,)), scales.new_empty((Q, N, d) if want_all else (0,))


# indices -> code vectors of the lookup-free family (native.lfq_decode): the codes are a function of the index bits, so the
# op has no differentiable input.  An output that was not requested comes back as an empty tensor.
@torch.library.custom_op(f"{_LIB_NS}::lfq_decode", mutates_args=())
def lfq_decode(indices: torch.Tensor, mag: list[float], d: int, drop_null: bool, want_sum: bool,
               want_all: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """indices [G, N, Qg], one magnitude per stage -> (codes summed over the stages [G, N, d] (or empty), all codes
    [Q, G, N, d] (or empty))."""
    codes_sum, all_codes = native.lfq_decode(indices, mag, d, drop_null=drop_null, want_sum=want_sum, want_all=want_all)
    if codes_sum is None:
        codes_sum = indices.new_empty((0,), dtype=torch.float32)
    if all_codes is None:
        all_codes = indices.new_empty((0,), dtype=torch.float32)
    return codes_sum, all_codes


@lfq_decode.register_fake
def _(indices, mag, d, drop_null, want_sum, want_all):
    G, N, _ = indices.shape
    return (indices.new_empty((G, N, d) if want_sum else (0,), dtype=torch.float32),
            indices.new_empty((len(mag), G, N, d) if want_all else (0,), dtype=torch.float32))


# indices -> code vectors (native.decode_codes).  An output that was not requested comes back as an empty tensor.
@torch.library.custom_op(f"{_LIB_NS}::decode_codes", mutates_args=())
def decode_codes(cb: torch.Tensor, indices: torch.Tensor, num_stages: int, drop_null: bool, want_sum: bool,
                 want_all: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """cb [G | 1, Q | 1, K, D], indices [G, N, Qg] -> (codes summed over the stages [G, N, D] (or empty), all codes
    [Q, G, N, D] (or empty))."""
    codes_sum, all_codes = native.decode_codes(cb, indices, num_stages=num_stages, drop_null=drop_null, want_sum=want_sum,
                                               want_all=want_all)
    if codes_sum is None:
        codes_sum = cb.new_empty((0,))
    if all_codes is None:
        all_codes = cb.new_empty((0,))
    return codes_sum, all_codes


@decode_codes.register_fake
def _(cb, indices, num_stages, drop_null, want_sum, want_all):
    G, N, _ = indices.shape
    D = cb.shape[-1]
    return cb.new_empty((G, N, D) if want_sum else (0,)), cb.new_empty((num_stages, G, N, D) if want_all else (0,))


def _decode_setup(ctx, inputs, output):
    cb, indices, _num_stages, drop_null, want_sum, want_all = inputs
    ctx.save_for_backward(indices)
    ctx.cb_shape, ctx.drop_null, ctx.want = tuple(cb.shape), drop_null, (want_sum, want_all)


def _decode_backward(ctx, g_sum, g_all):
    from .search import decode_grad_codes  # (search imports this module lazily as well)

    (indices,) = ctx.saved_tensors
    want_sum, want_all = ctx.want
    return (decode_grad_codes(ctx.cb_shape, indices, ctx.drop_null, g_sum if want_sum else None, g_all if want_all else None),
            None, None, None, None, None)


decode_codes.register_autograd(_decode_backward, setup_context=_decode_setup)


# latent quantization (native.lq_*).  z [B, P, C * d] of any strides; the codes come back laid out as z; indices or a loss
# that were not requested come back as empty tensors.
@torch.library.custom_op(f"{_LIB_NS}::lq_quantize", mutates_args=())
def lq_quantize(z: torch.Tensor, levels: list[int], tables: torch.Tensor, num_codebooks: int, want_idx: bool, want_loss: bool,
                w_c: float, w_q: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """z [B, P, C * d] -> (codes [B, P, C * d], idx [B, P, C] int32 (or empty), loss [2] = (weighted, mean) (or empty))."""
    out = torch.empty_like(z)
    _, idx, loss = native.lq_quantize(z, levels, tables, num_codebooks, want_idx=want_idx,
                                      loss_weights=(w_c, w_q) if want_loss else None, out=out)
    if idx is None:
        idx = z.new_empty((0,), dtype=torch.int32)
    if loss is None:
        loss = z.new_empty((0,))
    return out, idx, loss


@lq_quantize.register_fake
def _(z, levels, tables, num_codebooks, want_idx, want_loss, w_c, w_q):
    B, P, _ = z.shape
    return (torch.empty_like(z), z.new_empty((B, P, num_codebooks) if want_idx else (0,), dtype=torch.int32),
            z.new_empty((2,) if want_loss else (0,)))


@torch.library.custom_op(f"{_LIB_NS}::lq_backward", mutates_args=())
def lq_backward(x: torch.Tensor, out: torch.Tensor, g_out: torch.Tensor, g_loss: torch.Tensor, coef: float) -> torch.Tensor:
    """g_out + (g_loss * coef) * (out - x) (native.lq_backward), laid out as x."""
    grad_x = torch.empty_like(x)
    return native.lq_backward(x, out, g_out, g_loss, coef, grad_x=grad_x)


@lq_backward.register_fake
def _(x, out, g_out, g_loss, coef):
    return torch.empty_like(x)
