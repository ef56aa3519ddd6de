"""Generate the Gumbel straight-through / reinmax fixtures by IMPORTING THE REFERENCE (the development container only;
never runs on the GPU box).

    python tests/golden/make_golden_gumbel.py        # writes tests/golden/data/gumbel_<case>.npz

Each fixture is data only: the config (JSON), the input x, the codebook cb, the fixed random tensor r, the mask (if any)
and the reference's quantize, embed_ind, loss, dL/dx and -- where the codebook is learnable -- dL/dcodebook for
L = (quantize * r).sum() + loss.  The in-place-optimizer case also holds the codebook after the step and the step's loss;
the EMA case the buffers after the update.  The reference runs on torch's CPU path.
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

from gen import l2norm, make_codebook, make_x  # noqa: E402
from gumbel_cases import DIM, GUMBEL_CASES, K, X_SHAPE  # noqa: E402
from make_golden import make_mask  # noqa: E402


def _import_reference():
    einx = types.ModuleType("einx")  # the reference's package imports it for the residual quantizers only
    einx.get_at = None
    sys.modules["einx"] = einx
    sys.path.insert(0, os.environ.get("VQ_REFERENCE_ROOT", "/root/reference"))
    import vector_quantization as ref  # noqa
    from vector_quantization import codebooks as ref_cb  # noqa

    return ref, ref_cb


def run_vq(ref, ref_cb, c):
    vq_kw = dict(c.get("vq", {}))
    d = vq_kw.get("codebook_dim", DIM)
    h = vq_kw.get("heads", 1) if vq_kw.get("separate_codebook_per_head", False) else 1
    cos = c.get("cosine", False)
    norm = "l2norm" if cos else "identity"
    params = ref_cb.CodebookParams(dim=d, codebook_size=K, learnable_codebook=True, ema_update=False, use_cosine_sim=cos,
                                   transform_input=norm, weights_regularization=norm,
                                   gumbel_params=ref_cb.GumbelParams(**c["gumbel"]))
    if "sgd_lr" in c:
        vq_kw["in_place_codebook_optimizer"] = lambda p: torch.optim.SGD(p, lr=c["sgd_lr"])
    torch.manual_seed(777)
    mod = ref.VectorQuantize(dim=DIM, codebook_params=params, **vq_kw).train()
    cb = make_codebook(h, K, d, "S")
    if cos:
        cb = l2norm(cb)
    with torch.no_grad():
        mod._codebook.embeddings.copy_(cb)
    x = make_x(X_SHAPE, "S").requires_grad_(True)
    r = torch.randn(X_SHAPE, generator=torch.Generator().manual_seed(99))
    kwargs = {}
    data = {}
    if c.get("mask", False):
        kwargs["mask"] = make_mask(X_SHAPE[0], X_SHAPE[1])
        data["mask"] = kwargs["mask"].numpy()
    q, ind, loss, parts = mod(x, return_loss_breakdown=True, **kwargs)
    ((q * r).sum() + loss.sum()).backward()
    data.update(x=x.detach().numpy(), cb=cb.numpy(), r=r.numpy(), quantize=q.detach().numpy(),
                embed_ind=ind.numpy().astype(np.int32), loss=loss.detach().numpy(), gx=x.grad.numpy(),
                gcb=mod._codebook.embeddings.grad.numpy())
    if "sgd_lr" in c:
        data["cb_after"] = mod._codebook.embeddings.detach().numpy().copy()
        data["inplace_loss"] = np.asarray(parts.inplace_optimize.detach().numpy())
    return data


def run_codebook(ref, ref_cb, c):
    mod = ref_cb.Codebook(dim=DIM, codebook_size=K, ema_update=True, threshold_ema_dead_code=0,
                          gumbel_params=ref_cb.GumbelParams(**c["gumbel"])).train()
    cb = make_codebook(1, K, DIM, "S")
    with torch.no_grad():  # warm statistics consistent with the codes: the update stays on scale
        mod.embeddings.copy_(cb)
        mod.embed_avg.copy_(cb * 10.0)
        mod.cluster_size.fill_(10.0)
    x = make_x(X_SHAPE, "S").requires_grad_(True)
    r = torch.randn(X_SHAPE, generator=torch.Generator().manual_seed(99))
    q, ind, _sims = mod(x)
    (q * r).sum().backward()
    return dict(x=x.detach().numpy(), cb=cb.numpy(), r=r.numpy(), quantize=q.detach().numpy(),
                embed_ind=ind.numpy().astype(np.int32), loss=np.zeros(1, np.float32), gx=x.grad.numpy(),
                cb_after=mod.embeddings.detach().numpy().copy(), embed_avg_after=mod.embed_avg.numpy().copy(),
                cluster_size_after=mod.cluster_size.numpy().copy())


def main():
    ref, ref_cb = _import_reference()
    torch.set_num_threads(4)
    only = sys.argv[1:]
    for name, c in GUMBEL_CASES.items():
        if only and name not in only:
            continue
        data = (run_vq if c["kind"] == "vq" else run_codebook)(ref, ref_cb, c)
        meta = dict(case=c, torch=torch.__version__, threads=torch.get_num_threads())
        data["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, "data", f"gumbel_{name}.npz"), **data)
        print(f"gumbel_{name:14s} loss {float(data['loss'].sum()):.6g} |gx| {np.abs(data['gx']).max():.4g}"
              + (f" |gcb| {np.abs(data['gcb']).max():.4g}" if "gcb" in data else ""))


if __name__ == "__main__":
    main()
