"""Shared by the host and the GPU test of the cross-entropy loss's gradient with respect to a learnable codebook
(vq_ce_backward_codes_f32, the kCeC role of the sweep): the dense closed form of the loss and both gradients, the reference's
own op sequence with autograd, and the tests/golden/data/ce_codes_<case>.npz fixtures run through this package.

Per head, with s = similarities(x, c) [M, K] (x c^T, or -cdist(x, c)), t the targets and coef = g / (number of valid rows):
    valid_m = 0 <= t_m < K
    w_mk    = coef * (softmax_k(s_m)_k - [k == t_m])     for valid rows, 0 otherwise
    dot     gx = w c                       gc_k = sum_m w_mk x_m
    Euclid  r = w / s (0 where s == 0)     gx = x rowsum(r) - r c      gc_k = c_k sum_m r_mk - sum_m r_mk x_m
An ignored row is never read: whatever its x holds (NaN, inf), it adds nothing to the loss or to either gradient."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from ce_codes_cases import CE_CODES_CASES
from helpers import load_golden


EXACT = "donot_use_mm_for_euclid_dist"  # cdist from the differences: a row bit-equal to a code is at distance exactly 0


def similarities(x, c, metric_dot):
    return x @ c.transpose(-1, -2) if metric_dot else -torch.cdist(x, c, compute_mode=EXACT)


def _valid_rows(x, c, target):
    """(valid [H, M], x with the ignored rows replaced by zeros, the targets with -1 in every ignored row)"""
    valid = (target >= 0) & (target < c.shape[1])
    return valid, torch.where(valid[..., None], x, torch.zeros_like(x)), torch.where(valid, target, torch.full_like(target, -1))


def closed_form(x, c, target, metric_dot, coef=None, g_loss=1.0, dtype=torch.float64):
    """x [H, M, D], c [H, K, D], target [H, M] int64 -> dict(loss, gx [H, M, D], gc [H, K, D], count) in ``dtype``, dense, no
    autograd.  ``coef``: the factor of the gradients (default g_loss / count, count = the valid rows of all heads)."""
    valid, xs, t = _valid_rows(x, c, target)
    xs, c = xs.to(dtype), c.to(dtype)
    count = int(valid.sum())
    if coef is None:
        coef = g_loss / max(count, 1)
    s = similarities(xs, c, metric_dot)
    lse = s.logsumexp(-1)
    hot = F.one_hot(t.clamp(min=0), c.shape[1]).to(dtype)
    picked = (s * hot).sum(-1)
    zero = torch.zeros((), dtype=dtype)
    loss = torch.where(valid, lse - picked, zero).sum() / max(count, 1)
    w = torch.where(valid[..., None], coef * (s.softmax(-1) - hot), zero)
    if metric_dot:
        gx, gc = w @ c, w.transpose(-1, -2) @ xs
    else:
        r = torch.where(s == 0, torch.zeros_like(w), w / s)
        gx = xs * r.sum(-1, keepdim=True) - r @ c
        gc = c * r.sum(-2).unsqueeze(-1) - r.transpose(-1, -2) @ xs
    return dict(loss=loss, gx=gx, gc=gc, count=count)


def reference_sequence(x, c, target, metric_dot, coef=None, g_loss=1.0, dtype=torch.float32, compute_mode=None):
    """The reference's own op sequence in ``dtype`` with autograd (vector_quantize_pytorch.py:287-297 on codebooks.py's
    similarities): F.cross_entropy(similarities, target, ignore_index=-1, reduction="sum") / count through -cdist / einsum,
    over the valid rows -> dict(loss, gx, gc, count).  ``compute_mode``: cdist's (None: the reference's default)."""
    valid, xs, t = _valid_rows(x, c, target)
    count = int(valid.sum())
    if coef is None:
        coef = g_loss / max(count, 1)
    xs = xs.to(dtype).clone().requires_grad_(True)
    c = c.to(dtype).clone().requires_grad_(True)
    s = torch.einsum("hmd,hkd->hmk", xs, c) if metric_dot else -torch.cdist(xs, c, **(dict(compute_mode=compute_mode) if compute_mode else {}))
    total = F.cross_entropy(s.reshape(-1, s.shape[-1]), t.reshape(-1), ignore_index=-1, reduction="sum")
    (total * coef).backward()
    return dict(loss=total.detach() / max(count, 1), gx=xs.grad, gc=c.grad, count=count)


# ------------------------------------------------------------------------------------------------ the fixtures
def _layout(c):
    vq = c["vq"]
    heads = vq.get("heads", 1)
    return heads, vq.get("separate_codebook_per_head", False), vq.get("codebook_dim", c["dim"])


def fixture_closed_form(name, dtype=torch.float64):
    """The closed form on a fixture's inputs, carried back to the module's arguments with autograd of the layout ops (head
    split, l2norm of the rows under the cosine metric) -> (arrays, dict(loss, gx like x, gcb [h, K, d]))."""
    c = CE_CODES_CASES[name]
    arrays, _meta = load_golden("ce_codes_" + name)
    heads, separate, d = _layout(c)
    cos = c.get("cosine", False)
    x = torch.from_numpy(arrays["x"]).to(dtype).requires_grad_(True)
    cb = torch.from_numpy(arrays["cb"]).to(dtype)
    b, n, _ = x.shape
    ind = torch.from_numpy(arrays["embed_ind"]).to(torch.int64).reshape(b, n, heads)
    if heads == 1:
        rows, target = x.reshape(1, b * n, d), ind.reshape(1, b * n)
    elif separate:  # b n (h d) -> h (b n) d
        rows, target = x.reshape(b * n, heads, d).permute(1, 0, 2), ind.reshape(b * n, heads).permute(1, 0)
    else:  # b n (h d) -> 1 (b h n) d
        rows = x.reshape(b, n, heads, d).permute(0, 2, 1, 3).reshape(1, b * heads * n, d)
        target = ind.permute(0, 2, 1).reshape(1, b * heads * n)
    if cos:
        rows = F.normalize(rows, p=2, dim=-1)
    res = closed_form(rows.detach(), cb, target, cos, dtype=dtype)
    rows.backward(res["gx"])
    return arrays, dict(loss=res["loss"].reshape(1), gx=x.grad, gcb=res["gc"])


def run_fixture(name, device="cpu"):
    """A fixture through this package's VectorQuantize -> (arrays, dict(quantize, embed_ind, loss, gx, gcb, module))."""
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    c = CE_CODES_CASES[name]
    arrays, _meta = load_golden("ce_codes_" + name)
    heads, separate, d = _layout(c)
    cos = c.get("cosine", False)
    norm = "l2norm" if cos else "identity"
    params = CodebookParams(dim=d, codebook_size=c["K"], learnable_codebook=True, ema_update=False, use_cosine_sim=cos,
                            transform_input=norm, weights_regularization=norm)
    mod = vq.VectorQuantize(dim=c["dim"], codebook_params=params, **c["vq"])
    with torch.no_grad():
        mod._codebook.embeddings.copy_(torch.from_numpy(arrays["cb"]))
    mod = mod.to(device).train()
    x = torch.from_numpy(arrays["x"]).to(device).requires_grad_(True)
    kwargs = {}
    if "mask" in arrays:
        kwargs["mask"] = torch.from_numpy(arrays["mask"]).to(device)
    if "indices" in arrays:
        indices = torch.from_numpy(arrays["indices"]).to(torch.int64).to(device)
        q, loss = mod(x, indices=indices, **kwargs)
        ind = indices
    else:
        q, ind, loss = mod(x, **kwargs)
    loss.sum().backward()
    return arrays, dict(quantize=q, embed_ind=ind, loss=loss.detach().reshape(-1), gx=x.grad, gcb=mod._codebook.embeddings.grad,
                        module=mod)


def check_fixture(name, device="cpu"):
    from gumbel_run import assert_grad_close

    arrays, res = run_fixture(name, device)
    assert np.array_equal(res["embed_ind"].cpu().numpy(), arrays["embed_ind"]), "indices differ from the reference"
    np.testing.assert_allclose(res["quantize"].detach().cpu().numpy(), arrays["quantize"], rtol=1e-6, atol=1e-6)
    assert_grad_close(res["loss"], arrays["loss"], f"{name} loss")
    assert_grad_close(res["gx"], arrays["gx"], f"{name} dL/dx")
    assert_grad_close(res["gcb"], arrays["gcb"], f"{name} dL/dcodebook")
    return arrays, res
