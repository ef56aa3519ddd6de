"""Generate the masked residual-stack fixtures by IMPORTING THE REFERENCE (CPU only, like make_golden.py, whose einx stand-in
and seeded inputs it shares):

    python tests/golden/make_golden_rvq_mask.py            # writes tests/golden/data/rvq_mask_*.npz

Fixtures are data only: the expected indices, outputs, losses, d loss / d x and EMA buffers of the cases in
rvq_mask_cases.py.  The inputs are regenerated from seeds by the tests (gen.py); the fixtures carry their checksums.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen import CB_SEED, checksum, make_rvq_codebooks, make_x, poison_  # noqa: E402
from make_golden import _import_reference, q_weights  # noqa: E402
from rvq_mask_cases import CASES, DIM, GROUPS, K, Q, X_SHAPE, make_mask  # noqa: E402


def build(ref, ref_cb, c):
    """-> (module, x, the codebooks [G, Q, K, D] it was given)."""
    params = ref_cb.CodebookParams(dim=DIM, codebook_size=K, **c["cb_extra"])
    grouped = c["kind"] == "grvq"
    if grouped:
        mod = ref.GroupedResidualVQ(dim=GROUPS * DIM, groups=GROUPS, num_quantizers=Q, codebook_params=params, **c["rvq_extra"])
        rvqs = list(mod.rvqs)
    else:
        mod = ref.ResidualVQ(dim=DIM, num_quantizers=Q, codebook_params=params, shared_codebook=c["shared_codebook"],
                             **c["rvq_extra"])
        rvqs = [mod]
    all_cbs = []
    with torch.no_grad():
        for g, rvq in enumerate(rvqs):
            cbs = make_rvq_codebooks(Q, K, DIM, "S", seed=CB_SEED + 100 * g)
            all_cbs.append(cbs)
            for i, layer in enumerate(rvq.layers):
                layer._codebook.embeddings.copy_(cbs[0 if c["shared_codebook"] else i][None])
                layer._codebook.embed_avg.copy_(cbs[0 if c["shared_codebook"] else i][None])
    shape = (*X_SHAPE[:-1], (GROUPS if grouped else 1) * DIM)
    x = make_x(shape, "S")
    poison_(x, all_cbs[0], c["nonfinite"])
    return mod, x, torch.stack(all_cbs)


def run(ref, ref_cb, c):
    mod, x, cbs = build(ref, ref_cb, c)
    mask = make_mask()
    kwargs = dict(mask=mask, **c["fwd_extra"])
    if c["training"]:
        mod.train()
        kwargs["freeze_codebook"] = c["freeze_codebook"]
    else:
        mod.eval()
    x = x.requires_grad_(c["grad"])
    with torch.set_grad_enabled(c["grad"]):
        q, idx, losses = mod(x, **kwargs)[:3]
    arrays = dict(idx=idx.numpy().astype(np.int32), loss=losses.detach().numpy().astype(np.float32),
                  q_full=q.detach().numpy().copy())
    if c["grad"]:
        (losses.sum() + (q * q_weights(q.shape)).sum()).backward()
        arrays["g_full"] = x.grad.numpy().copy()
    if c["training"] and not c["freeze_codebook"]:
        layers = [l for rvq in (mod.rvqs if c["kind"] == "grvq" else [mod]) for l in rvq.layers]
        arrays["ema_embeddings"] = torch.stack([l._codebook.embeddings for l in layers]).detach().numpy().copy()
        arrays["ema_embed_avg"] = torch.stack([l._codebook.embed_avg for l in layers]).detach().numpy().copy()
        arrays["ema_cluster_size"] = torch.stack([l._codebook.cluster_size for l in layers]).detach().numpy().copy()
    meta = dict(x_checksum=checksum(x.detach().nan_to_num(0.0, 0.0, 0.0)), cb_checksum=checksum(cbs),
                q_shape=list(q.shape), idx_shape=list(idx.shape))
    return arrays, meta


def main():
    ref, ref_cb = _import_reference()
    out_dir = os.path.join(HERE, "data")
    only = set(sys.argv[1:])
    for c in CASES:
        if only and c["name"] not in only:
            continue
        arrays, meta = run(ref, ref_cb, c)
        meta.update(case=c, torch_version=torch.__version__, num_threads=torch.get_num_threads(),
                    generator="tests/golden/make_golden_rvq_mask.py importing the reference @ 2024_10_08")
        arrays["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(out_dir, c["name"] + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{c['name']:>26s}  idx{tuple(arrays['idx'].shape)}  loss={arrays['loss'].ravel()[:4]}  "
              f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
