"""Generate the ResidualLFQ / GroupedResidualLFQ golden fixtures by IMPORTING THE REFERENCE (this container only; never
runs on the GPU box).

    python tests/golden/make_golden_rlfq.py        # writes tests/golden/data/rlfq_<case>.npz

Each fixture is data only: the config (JSON), the state_dict (its key list and every tensor as sd_<key>), the input x, any
mask, the upstream weight r, and the reference's outputs -- quantized output, indices, stacked losses, dL/dx of
losses.sum() + (out * r).sum(), all_codes when requested, get_output_from_indices of the indices (and of the first two
stages, padded, under quantize dropout).  grad64 is the fp64 restatement of dL/dx (tests/rlfq_dense.py) and grad_ref_dev
the largest distance of the reference's fp32 dL/dx from it.  The reference runs on torch's CPU path in fp32.
"""
from __future__ import annotations

import json
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from rlfq_cases import RLFQ_CASES  # noqa: E402
from rlfq_dense import restate, stage_rows  # noqa: E402


def _get_at(pattern, codebooks, indices):
    """einx.get_at for the one pattern the residual quantizers use: codebooks [q, c, d], indices [b, n, q] -> [q, b, n, d]."""
    assert pattern == "q [c] d, b n q -> q b n d", pattern
    q = codebooks.shape[0]
    return torch.stack([codebooks[i][indices[..., i]] for i in range(q)])


def _import_reference():
    einx = types.ModuleType("einx")
    einx.get_at = _get_at
    sys.modules["einx"] = einx
    sys.path.insert(0, "/root/reference")
    from vector_quantization.residual_lfq import GroupedResidualLFQ, ResidualLFQ  # noqa

    return ResidualLFQ, GroupedResidualLFQ


def _mask(shape):
    b, n = shape[0], shape[1]
    mask = torch.zeros(b, n, dtype=torch.bool)
    for i in range(b):
        mask[i, : max(1, n // (i + 2))] = True
    return mask


def run_case(classes, name, c):
    ResidualLFQ, GroupedResidualLFQ = classes
    kw = dict(c["kwargs"])
    torch.manual_seed(c.get("init_seed", 0))
    grouped = c["kind"] == "grlfq"
    mod = (GroupedResidualLFQ if grouped else ResidualLFQ)(**kw)
    mod.train(c.get("train", True))
    g = torch.Generator().manual_seed(2000 + len(name))
    x = torch.randn(*c["shape"], generator=g) * c.get("x_scale", 1.0)
    if c.get("zeros"):
        x.view(-1)[:: c["zeros"]] = 0.0
    mask = _mask(c["shape"]) if c.get("mask") else None
    x = x.requires_grad_(True)
    codes = c.get("codes", False)
    random.seed(c.get("py_seed", 0))
    torch.manual_seed(c.get("draw_seed", 5))  # the frac_per_sample_entropy draws use the global CPU generator
    if grouped:
        res = mod(x, mask=mask, return_all_codes=codes)
    else:
        res = mod(x, mask=mask, return_all_codes=codes, rand_quantize_dropout_fixed_seed=c.get("seed"))
    out, idx, losses = res[:3]
    r = torch.randn(out.shape, generator=g)
    data = dict(x=x.detach().numpy(), r=r.numpy(), out=out.detach().numpy(), idx=idx.numpy(),
                losses=losses.detach().numpy())
    if codes:
        all_codes = res[3]
        data["all_codes"] = (torch.stack(all_codes) if isinstance(all_codes, tuple) else all_codes).detach().numpy()
    if mod.training:
        (losses.sum() + (out * r).sum()).backward()
        data["grad"] = x.grad.numpy()
    if mask is not None:
        data["mask"] = mask.numpy()
    sd = mod.state_dict()
    data["sd_keys"] = np.array(json.dumps([[k, list(t.shape), str(t.dtype)] for k, t in sd.items()]))
    for k, t in sd.items():
        data["sd_" + k] = t.numpy()
    with torch.no_grad():
        data["from_idx"] = mod.get_output_from_indices(idx).numpy()
        if not grouped and kw.get("quantize_dropout") and idx.shape[-1] > 2:
            data["from_idx_pad"] = mod.get_output_from_indices(idx[..., :2]).numpy()
    if mod.training:
        # fp64 restatement of dL/dx, with the same draws
        torch.manual_seed(c.get("draw_seed", 5))
        rvqs = list(mod.rvqs) if grouped else [mod]
        G = len(rvqs)
        xs = x.detach().chunk(G, dim=-1)
        rs = r.chunk(G, dim=-1)
        idx_g = idx if grouped else idx[None]
        grads = []
        for gi, rvq in enumerate(rvqs):
            stages = int((idx_g[gi].reshape(-1, idx_g.shape[-1]) != -1).any(0).sum())
            inner = dict(kw)
            inner.pop("groups", None)
            inner.pop("dim")
            N = xs[gi].numel() // xs[gi].shape[-1]
            rows = stage_rows(N, mask, inner.get("frac_per_sample_entropy", 1.0), stages)
            sdg = {k: t.detach() for k, t in rvq.state_dict().items()}
            st = restate(inner, sdg, xs[gi], mask, rs[gi], stages, rows)
            lg = losses[gi] if grouped else losses
            np.testing.assert_allclose(st["losses"].numpy(), lg.detach().double().numpy()[:stages], rtol=1e-4, atol=1e-6)
            grads.append(st["grad"])
        grad64 = torch.cat(grads, dim=-1)
        data["grad64"] = grad64.numpy()
        data["grad_ref_dev"] = np.float64((grad64 - x.grad.double()).abs().max())
    data["config"] = np.array(json.dumps(c))
    np.savez_compressed(os.path.join(HERE, "data", f"rlfq_{name}.npz"), **data)
    return data


def main():
    classes = _import_reference()
    torch.set_num_threads(4)
    only = sys.argv[1:]
    for name, c in RLFQ_CASES.items():
        if only and name not in only:
            continue
        d = run_case(classes, name, c)
        print(f"{name:16s} losses {np.array2string(np.asarray(d['losses']).reshape(-1)[:4], precision=5)} "
              f"ref_dev {float(d.get('grad_ref_dev', 0.0)):.2e}")


if __name__ == "__main__":
    main()
