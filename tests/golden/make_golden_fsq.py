"""Generate the FSQ / ResidualFSQ / GroupedResidualFSQ golden fixtures by IMPORTING THE REFERENCE (this container only;
never runs on the GPU box).

    python tests/golden/make_golden_fsq.py        # writes tests/golden/data/fsq_<case>.npz and rfsq_<case>.npz

Each fixture is data only: the config (JSON), the state_dict (its key list and every tensor as sd_<key>), the input x, the
upstream weight r, and the reference's outputs -- out, the indices (with their dtype), all_codes when requested, dL/dx of
(out * r).sum(), get_output_from_indices (of the indices, and of the first two stages under quantize dropout) or
indices_to_codes / indices_to_level_indices for FSQ.  grad64 is the fp64 restatement of dL/dx (tests/fsq_dense.py) and
grad_ref_dev the largest distance of the reference's dL/dx from it.  Any input row whose fp64 bound value at any stage
lies within MARGIN of a rounding boundary is drawn again; margin is the smallest distance left.  The reference runs on
torch's CPU path.
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

from fsq_cases import FSQ_CASES, RFSQ_CASES  # noqa: E402
from fsq_dense import forward64, restate  # noqa: E402

MARGIN = 1e-4


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
    from vector_quantization.finite_scalar_quantization import FSQ  # noqa
    from vector_quantization.residual_fsq import GroupedResidualFSQ, ResidualFSQ  # noqa

    return dict(fsq=FSQ, rfsq=ResidualFSQ, grfsq=GroupedResidualFSQ)


def _collide_rows(levels):
    """Level-index rows [k_0 .. k_{d-1}] that put every code whose index term is not an integer into some row."""
    rows = []
    for i, L in enumerate(levels):
        hw = np.float32(L // 2)
        for k in range(L):
            c = np.float32(np.float32(k - L // 2) / hw)
            t = np.float32(np.float32(c * hw) + hw)
            if t != k:
                row = [0] * len(levels)  # the other terms exactly 0, so a term below its integer moves the index
                row[i] = k
                rows.append(row)
    return rows


def _x_for_level_indices(rows, levels):
    """Inputs whose bound lands exactly on the given level indices (margin 0.5)."""
    L = torch.tensor(levels, dtype=torch.float64)
    half_l = (L - 1) * 1.001 / 2
    offset = torch.tensor([0.5 if v % 2 == 0 else 0.0 for v in levels], dtype=torch.float64)
    shift = torch.atanh(offset / half_l)
    b = torch.tensor(rows, dtype=torch.float64) - torch.tensor([v // 2 for v in levels], dtype=torch.float64)
    return torch.atanh((b + offset) / half_l) - shift


def _draw(kind, kw, sd, c, g):
    """The input, drawn until every row clears MARGIN (non-finite and collision rows are placed, not drawn)."""
    shape = c["shape"]
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * c.get("x_scale", 1.0)
    cf = c.get("kwargs", {}).get("channel_first", False)
    dtype = getattr(torch, c.get("dtype", "float32"))
    for _ in range(200):
        x = x.to(dtype).double()  # the margin of the values the module sees
        _, margin = forward64(kind, kw, sd, x)
        bad = margin < MARGIN
        if c.get("nonfinite"):
            bad[0, :3] = False
        if not bool(bad.any()):
            break
        fresh = torch.randn(*shape, generator=g, dtype=torch.float64)
        if cf:
            x = torch.where(bad[:, None], fresh, x)
        else:
            x = torch.where(bad[..., None], fresh, x)
    else:
        raise RuntimeError("could not clear the rounding boundaries")
    if c.get("collide"):
        rows = _collide_rows(kw["levels"])
        assert 0 < len(rows) <= shape[1], rows
        x[0, : len(rows)] = _x_for_level_indices(rows, kw["levels"])
    if c.get("nonfinite"):
        x[0, 0, 1] = float("nan")
        x[0, 1, 2] = float("inf")
        x[0, 2, 0] = float("-inf")
    _, margin = forward64(kind, kw, sd, x)
    finite = torch.isfinite(margin)
    return x, float(margin[finite].min())


def run_case(classes, name, c, prefix):
    kind = c["kind"]
    kw = dict(c["kwargs"])
    torch.manual_seed(c.get("init_seed", 0))
    mod = classes[kind](**kw)
    mod.train(c.get("train", True))
    sd = {k: t.detach() for k, t in mod.state_dict().items()}
    g = torch.Generator().manual_seed(3000 + len(name) + 7 * len(prefix))
    x64, margin = _draw(kind, kw, sd, c, g)
    dtype = getattr(torch, c.get("dtype", "float32"))
    x = x64.to(dtype).requires_grad_(True)
    codes = c.get("codes", False)
    random.seed(c.get("py_seed", 0))
    if kind == "fsq":
        res = mod(x)
    elif kind == "rfsq":
        res = mod(x, return_all_codes=codes, rand_quantize_dropout_fixed_seed=c.get("seed"))
    else:
        res = mod(x, return_all_codes=codes)
    out, idx = res[:2]
    r = torch.randn(out.shape, generator=g)
    data = dict(x=x.detach().float().numpy() if dtype == torch.bfloat16 else x.detach().numpy(), r=r.numpy(),
                out=out.detach().float().numpy() if out.dtype == torch.bfloat16 else out.detach().numpy(),
                margin=np.float64(margin))
    if idx is not None:
        data["idx"] = idx.numpy()
    if codes:
        all_codes = res[2]
        data["all_codes"] = (torch.stack(all_codes) if isinstance(all_codes, tuple) else all_codes).detach().numpy()
    (out.float() * r).sum().backward()
    data["grad"] = x.grad.float().numpy() if dtype == torch.bfloat16 else x.grad.numpy()
    data["sd_keys"] = np.array(json.dumps([[k, list(t.shape), str(t.dtype)] for k, t in sd.items()]))
    for k, t in sd.items():
        data["sd_" + k] = t.numpy()
    with torch.no_grad():
        if kind == "fsq":
            if idx is not None:
                valid = idx.clone()
                valid[valid < 0] = 0  # the NaN rows' INT32_MIN
                data["idx_valid"] = valid.numpy()
                data["codes_from_idx"] = mod.indices_to_codes(valid).float().numpy()
                data["level_idx"] = mod.indices_to_level_indices(valid).numpy()
        else:
            data["from_idx"] = mod.get_output_from_indices(idx).numpy()
            if kind == "rfsq" and kw.get("quantize_dropout") and idx.shape[-1] > 2:
                data["from_idx_pad"] = mod.get_output_from_indices(idx[..., :2]).numpy()
    # fp64 restatement of dL/dx over the stages that ran
    stages = None
    if kind != "fsq":
        stages = int((idx.reshape(-1, idx.shape[-1]) != -1).any(0).sum())
    finite_rows = torch.isfinite(x64).all(dim=-1)
    st = restate(kind, kw, sd, x.detach().double(), r, stages)
    grad64 = st["grad"]
    data["grad64"] = grad64.numpy()
    fin = torch.isfinite(grad64) & finite_rows[..., None] if not kw.get("channel_first") else torch.isfinite(grad64)
    dev = (grad64 - x.grad.double()).abs()[fin]
    data["grad_ref_dev"] = np.float64(dev.max()) if dev.numel() else np.float64(0.0)
    data["config"] = np.array(json.dumps(c))
    np.savez_compressed(os.path.join(HERE, "data", f"{prefix}_{name}.npz"), **data)
    return data


def main():
    classes = _import_reference()
    torch.set_num_threads(4)
    only = sys.argv[1:]
    for prefix, cases in (("fsq", FSQ_CASES), ("rfsq", RFSQ_CASES)):
        for name, c in cases.items():
            if only and name not in only:
                continue
            d = run_case(classes, name, c, prefix)
            idx = d.get("idx")
            print(f"{prefix}_{name:10s} idx {None if idx is None else (idx.dtype, idx.shape)} margin {float(d['margin']):.2e} "
                  f"ref_dev {float(d['grad_ref_dev']):.2e}")


if __name__ == "__main__":
    main()
