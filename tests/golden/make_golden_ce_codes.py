"""Generate the cross-entropy fixtures of a learnable codebook by IMPORTING THE REFERENCE (the development container only;
never runs on the GPU box).

    python tests/golden/make_golden_ce_codes.py        # writes tests/golden/data/ce_codes_<case>.npz

Each fixture is data only: the config (JSON), the input x, the initial codebook cb, the mask or the given indices (if any) and
the reference's quantize, embed_ind (the given indices where the module returns none), loss, dL/dx and dL/dcodebook for
L = loss.sum().  The reference runs on torch's CPU path.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from ce_codes_cases import CE_CODES_CASES  # noqa: E402
from gen import l2norm, make_codebook, make_x  # noqa: E402
from make_golden import given_indices, make_mask  # noqa: E402
from make_golden_gumbel import _import_reference  # noqa: E402


def run_case(ref, ref_cb, c):
    vq_kw = dict(c["vq"])
    dim, K = c["dim"], c["K"]
    heads = vq_kw.get("heads", 1)
    d = vq_kw.get("codebook_dim", dim)
    h = heads if vq_kw.get("separate_codebook_per_head", False) else 1
    cos = c.get("cosine", False)
    norm = "l2norm" if cos else "identity"
    params = ref_cb.CodebookParams(dim=d, codebook_size=K, learnable_codebook=True, ema_update=False, use_cosine_sim=cos,
                                   transform_input=norm, weights_regularization=norm)
    torch.manual_seed(777)
    mod = ref.VectorQuantize(dim=dim, codebook_params=params, **vq_kw).train()
    assert not mod.has_projections
    cb = make_codebook(h, K, d, "S")
    if cos:
        cb = l2norm(cb)
    with torch.no_grad():
        mod._codebook.embeddings.copy_(cb)
    x = make_x(c["x_shape"], "S").requires_grad_(True)
    kwargs, data = {}, {}
    if c.get("mask", False):
        kwargs["mask"] = make_mask(x.shape[0], x.shape[1])
        data["mask"] = kwargs["mask"].numpy()
    if c.get("given_indices", False):
        b, n = x.shape[:2]
        kwargs["indices"] = given_indices(c, (b, n, heads) if heads > 1 else (b, n), K)
        data["indices"] = kwargs["indices"].numpy().astype(np.int32)
        q, loss = mod(x, **kwargs)
        ind = kwargs["indices"]
    else:
        q, ind, loss, _parts = mod(x, return_loss_breakdown=True, **kwargs)
    loss.sum().backward()
    data.update(x=x.detach().numpy(), cb=cb.numpy(), quantize=q.detach().numpy(), embed_ind=ind.numpy().astype(np.int32),
                loss=loss.detach().numpy().reshape(-1), gx=x.grad.numpy(), gcb=mod._codebook.embeddings.grad.numpy())
    return data


def main():
    ref, ref_cb = _import_reference()
    torch.set_num_threads(4)
    only = sys.argv[1:]
    for name, c in CE_CODES_CASES.items():
        if only and name not in only:
            continue
        data = run_case(ref, ref_cb, c)
        meta = dict(case=c, torch=torch.__version__, threads=torch.get_num_threads())
        data["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, "data", f"ce_codes_{name}.npz"), **data)
        print(f"ce_codes_{name:16s} loss {float(data['loss'].sum()):.6g} |gx| {np.abs(data['gx']).max():.4g} "
              f"|gcb| {np.abs(data['gcb']).max():.4g} ignored {int((data['embed_ind'] < 0).sum())}")


if __name__ == "__main__":
    main()
