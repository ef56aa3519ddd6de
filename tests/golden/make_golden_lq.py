"""Generate the LatentQuantize golden fixtures by IMPORTING THE REFERENCE (the development container only; never runs on
the GPU box).

    python tests/golden/make_golden_lq.py        # writes tests/golden/data/lq_<case>.npz

Each fixture is data only: the config (JSON), the state_dict (its key list and every tensor as sd_<key>), the value
tables the forward used (tab_<i>), the input x, the upstream weight r, and the reference's outputs -- out, the indices
(with their dtype), the loss, dL/dx of (out * r).sum() + loss, indices_to_codes of the (valid) indices, whether any
values_per_latent[i].grad was set -- plus the fp64 restatement's loss and gradient (tests/lq_dense.py) and the
reference's own distance from them, and the smallest gap between the two smallest distances of any quantizer input
(margin; cases with projections are drawn until it is at least MARGIN).  The reference runs on torch's CPU path.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from lq_cases import LQ_CASES  # noqa: E402
from lq_dense import levels_of, restate64, smallest_gap  # noqa: E402

MARGIN = 1e-4


def _import_reference():
    einx = types.ModuleType("einx")  # the reference's package imports it for the residual quantizers only
    einx.get_at = None
    sys.modules["einx"] = einx
    sys.path.insert(0, os.environ.get("VQ_REFERENCE_ROOT", "/root/reference"))
    from vector_quantization.latent_quantization import LatentQuantize  # noqa

    return LatentQuantize


def _overwrite_tables(mod, how, g):
    sd = mod.state_dict()
    for i, L in enumerate(mod._levels.tolist()):
        t = sd[f"values_per_latent.{i}"].clone()
        if how == "unsorted":
            t = t[torch.randperm(L, generator=g)] + 0.01 * torch.randn(L, generator=g)
        elif how == "dup":
            t[1] = t[0]
            t[L - 1] = t[L // 2]
        elif how == "nan" and i == 1:
            t[2] = float("nan")
        sd[f"values_per_latent.{i}"] = t
    mod.load_state_dict(sd)


def _projected(mod, x):
    with torch.no_grad():
        z = mod.project_in(x.movedim(1, -1).reshape(x.shape[0], -1, x.shape[1]))
    return z.reshape(z.shape[0], z.shape[1], mod.num_codebooks, mod.codebook_dim)


def run_case(cls, name, c):
    kw = dict(c["kwargs"])
    torch.manual_seed(c.get("init_seed", 0))
    mod = cls(**kw)
    g = torch.Generator().manual_seed(5000 + sum(map(ord, name)))
    if c.get("tables"):
        _overwrite_tables(mod, c["tables"], g)
    mod.train(c.get("train", True))
    tables = [t.detach().numpy().copy() for t in mod.values_per_latent]
    shape = c["shape"]
    scale = c.get("x_scale", 1.0)
    x = torch.randn(*shape, generator=g) * scale
    if mod.has_projections:
        for _ in range(200):
            gap = torch.from_numpy(smallest_gap(_projected(mod, x).numpy(), tables)).amin(-1).reshape(shape[0], -1)
            bad = (gap < MARGIN).reshape(shape[0], 1, *shape[2:])
            if not bool(bad.any()):
                break
            x = torch.where(bad, torch.randn(*shape, generator=g) * scale, x)
        else:
            raise RuntimeError("could not clear the near ties")
    if c.get("on_values"):
        for i, tab in enumerate(tables):
            for p in range(max(len(t) for t in tables)):
                x[(0, i, p) if x.dim() == 3 else (0, i)] = float(tab[p % len(tab)])
    if c.get("nonfinite"):
        x[0, 1, 0] = float("nan")
        x[0, 2, 1] = float("inf")
        x[0, 0, 2] = float("-inf")
    x = x.clone().requires_grad_(True)
    out, idx, loss = mod(x)
    r = torch.randn(out.shape, generator=g)
    ((out * r).sum() + loss).backward()
    table_grads = [getattr(t, "grad", None) is not None for t in mod.values_per_latent]
    sd = {k: t.detach() for k, t in mod.state_dict().items()}
    data = dict(x=x.detach().numpy(), r=r.numpy(), out=out.detach().numpy(), idx=idx.numpy(),
                loss=np.asarray(loss.detach().numpy()), grad=x.grad.numpy(), table_grad_set=np.array(any(table_grads)))
    for i, t in enumerate(tables):
        data[f"tab_{i}"] = t
    data["sd_keys"] = np.array(json.dumps([[k, list(t.shape), str(t.dtype)] for k, t in sd.items()]))
    for k, t in sd.items():
        data["sd_" + k] = t.numpy()
    data["buffers"] = np.array(json.dumps(sorted(k for k, _ in mod.named_buffers())))
    data["attrs"] = np.array(json.dumps(dict(
        dim=mod.dim, codebook_dim=mod.codebook_dim, num_codebooks=mod.num_codebooks,
        effective_codebook_dim=mod.effective_codebook_dim, keep_num_codebooks_dim=mod.keep_num_codebooks_dim,
        has_projections=mod.has_projections, codebook_size=mod.codebook_size, levels=mod._levels.tolist(),
        basis=mod._basis.tolist(), implicit_codebook_shape=list(mod.implicit_codebook.shape),
        values_type=type(mod.values_per_latent).__name__)))
    with torch.no_grad():
        valid = idx.clone()
        valid[valid < 0] = 0  # the NaN rows' INT32_MIN
        data["idx_valid"] = valid.numpy()
        data["codes_from_idx"] = mod.indices_to_codes(valid).numpy()
        z = _projected(mod, x.detach())
    data["margin"] = np.float64(np.nanmin(smallest_gap(z.numpy(), tables)))
    st = restate64(kw, {k: t.numpy() for k, t in sd.items()}, x.detach(), r, c.get("train", True), tables)
    data["loss64"] = np.float64(st["loss"])
    data["grad64"] = st["grad"].numpy()
    data["loss_ref_dev"] = np.float64(abs(float(st["loss"]) - float(loss.detach())))
    fin = np.isfinite(data["grad64"]) & np.isfinite(data["grad"])
    dev = np.abs(data["grad64"] - data["grad"].astype(np.float64))[fin]
    data["grad_ref_dev"] = np.float64(dev.max()) if dev.size else np.float64(0.0)
    data["config"] = np.array(json.dumps(c))
    np.savez_compressed(os.path.join(HERE, "data", f"lq_{name}.npz"), **data)
    return data


def main():
    cls = _import_reference()
    torch.set_num_threads(4)
    only = sys.argv[1:]
    for name, c in LQ_CASES.items():
        if only and name not in only:
            continue
        d = run_case(cls, name, c)
        print(f"lq_{name:12s} idx {d['idx'].dtype} {d['idx'].shape} loss {float(d['loss']):.6g} margin {float(d['margin']):.2e} "
              f"loss_dev {float(d['loss_ref_dev']):.2e} grad_dev {float(d['grad_ref_dev']):.2e}")


if __name__ == "__main__":
    main()
