"""Generate the LFQ golden fixtures by IMPORTING THE REFERENCE (this container only; never runs on the GPU box).

    python tests/golden/make_golden_lfq.py        # writes tests/golden/data/lfq_<case>.npz

Each fixture is data only: the config (JSON), the input x, any mask / upstream weight r / projection weights, and the
reference's outputs -- quantized output, indices, aux loss, the three LossBreakdown terms and dL/dx of
aux_loss.sum() + (out * r).sum().  The reference runs on torch's CPU path in fp32.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from lfq_cases import LFQ_CASES  # noqa: E402


def _import_reference():
    # the reference package's __init__ imports einx (not installed) for its residual quantizers; LFQ never calls it
    import types

    einx = types.ModuleType("einx")
    einx.get_at = None
    sys.modules.setdefault("einx", einx)
    sys.path.insert(0, "/root/reference")
    from vector_quantization.lookup_free_quantization import LFQ  # noqa

    return LFQ


def run_case(LFQ, name, c):
    kw = dict(c["kwargs"])
    torch.manual_seed(c.get("seed", 0))
    mod = LFQ(**kw)
    mod.train(c.get("train", True))
    g = torch.Generator().manual_seed(1000 + c.get("seed", 0))
    x = torch.randn(*c["shape"], generator=g) * c.get("x_scale", 1.0)
    if c.get("zeros"):
        x.view(-1)[:: c["zeros"]] = 0.0
    mask = None
    if c.get("mask"):
        b, n = c["shape"][0], c["shape"][1]
        mask = torch.zeros(b, n, dtype=torch.bool)
        for i in range(b):
            mask[i, : max(1, n // (i + 2))] = True
    x = x.requires_grad_(True)
    torch.manual_seed(c.get("draw_seed", 5))  # the frac_per_sample_entropy draw uses the global CPU generator
    (out, idx, aux), bd = mod(x, inv_temperature=c.get("tau", 100.0), return_loss_breakdown=True, mask=mask)
    r = torch.randn(out.shape, generator=g)
    data = dict(x=x.detach().numpy(), r=r.numpy(), out=out.detach().numpy(), idx=idx.numpy(),
                aux=np.float32(aux.detach()), ps=np.float32(bd.per_sample_entropy.detach()),
                cb=np.float32(bd.batch_entropy.detach()), commit=np.float32(bd.commitment.detach()))
    if mod.training:
        (aux.sum() + (out * r).sum()).backward()
        data["grad"] = x.grad.numpy()
    if mask is not None:
        data["mask"] = mask.numpy()
    for k, t in mod.state_dict().items():
        if k.startswith("project_"):
            data["w_" + k] = t.numpy()
    data["config"] = np.array(json.dumps(c))
    np.savez_compressed(os.path.join(HERE, "data", f"lfq_{name}.npz"), **data)
    return data


def main():
    LFQ = _import_reference()
    torch.set_num_threads(4)
    for name, c in LFQ_CASES.items():
        d = run_case(LFQ, name, c)
        print(f"{name:18s} aux {float(d['aux']):+.6f} ps {float(d['ps']):.6f} cb {float(d['cb']):.6f} commit {float(d['commit']):.6f}")


if __name__ == "__main__":
    main()
