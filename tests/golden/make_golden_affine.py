"""Generate the use_affine fixtures by IMPORTING THE REFERENCE (the development container only; never runs on the GPU box).

    python tests/golden/make_golden_affine.py        # writes tests/golden/data/affine_<case>.npz

Each fixture is data only: the config (JSON), the start codebook and, per step s of the case, the input ``x{s}``, the mask (if
any), the fixed random tensor ``r{s}``, the reference's ``quantize{s}`` / ``embed_ind{s}`` (/ ``loss{s}``, ``gx{s}``,
``gcb{s}``) and every buffer of the codebook after the step (``<buffer>{s}``), plus the key list of its state dict after the
first step.  The reference runs on torch's CPU path.

The generator ASSERTS, for every row of every step, that the reference's best similarity leads the second best by at least
1e-4 * max|s| -- about 100 times the fp32 difference a reordered transform can cause -- so the tests may demand every index
equal.  A seed that violates it is replaced by the next one (recorded in the fixture's meta); rows are never dropped.
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

from affine_cases import AFFINE, AFFINE_CASES, DIM, EMA_BUFFERS, K, STAT_BUFFERS, X_SHAPE  # noqa: E402
from gen import l2norm, make_codebook, make_x  # noqa: E402
from make_golden import make_mask  # noqa: E402

MARGIN = 1e-4


def _import_reference():
    einx = types.ModuleType("einx")  # the reference's package imports it for the residual quantizers only
    einx.get_at = None
    sys.modules["einx"] = einx
    sys.path.insert(0, os.environ.get("VQ_REFERENCE_ROOT", "/root/reference"))
    import vector_quantization as ref  # noqa
    from vector_quantization import codebooks as ref_cb  # noqa

    return ref, ref_cb


def build(ref, ref_cb, c):
    """-> (module, codebook module, start codes)"""
    h = c.get("heads", 1)
    cos = c.get("cosine", False)
    learnable = c.get("learnable", False)
    book = ref_cb.Codebook(dim=DIM, codebook_size=K, num_codebooks=h, threshold_ema_dead_code=0, learnable_codebook=learnable,
                           ema_update=not learnable, use_affine=True, affine_params=ref_cb.AffineParameters(**AFFINE),
                           use_cosine_sim=cos, weights_regularization="l2norm" if cos else "identity")
    cb = make_codebook(h, K, DIM, "S")
    if cos:
        cb = l2norm(cb)
    with torch.no_grad():  # warm statistics consistent with the codes: the update stays on scale
        book.embeddings.copy_(cb)
        book.embed_avg.copy_(cb * 10.0)
        book.cluster_size.fill_(10.0)
    if c["kind"] == "codebook":
        return book, book, cb
    params = ref_cb.CodebookParams(dim=DIM, codebook_size=K, threshold_ema_dead_code=0)
    mod = ref.VectorQuantize(dim=DIM, codebook_params=params, **c.get("vq", {}))
    mod._codebook = book  # (VectorQuantize(use_affine=True) itself crashes: asdict() turns affine_params into a dict)
    return mod, book, cb


def step_input(c, step, seed):
    shape = (c["heads"], *X_SHAPE) if c.get("heads", 1) > 1 else X_SHAPE
    x = make_x(shape, "S", seed=seed) + step["offset"]
    return l2norm(x) if c.get("cosine", False) else x


def run_case(ref, ref_cb, c, seeds):
    """Runs the case with the given seeds -> (data, index of the first step whose margin fails | None)"""
    mod, book, cb = build(ref, ref_cb, c)
    data = dict(cb=cb.numpy())
    seen = {}
    inner = book.forward

    def spy(*a, **k):
        out = inner(*a, **k)
        seen["sims"] = out[2].detach()
        return out

    book.forward = spy
    for s, (step, seed) in enumerate(zip(c["steps"], seeds)):
        mod.train(step["train"])
        x = step_input(c, step, seed).requires_grad_(True)
        r = torch.randn(x.shape, generator=torch.Generator().manual_seed(99 + s))
        kwargs = {}
        if step["mask"]:
            kwargs["mask"] = make_mask(X_SHAPE[0], X_SHAPE[1])
            data[f"mask{s}"] = kwargs["mask"].numpy()
        if c["kind"] == "vq":
            q, ind, loss = mod(x, **kwargs)
            objective = (q * r).sum() + loss.sum()
            data[f"loss{s}"] = loss.detach().numpy()
        else:
            q, ind, _ = mod(x, **kwargs)
            objective = (q * r).sum()
        top2 = seen["sims"].reshape(-1, K).topk(2, dim=-1).values
        if bool(((top2[:, 0] - top2[:, 1]) < MARGIN * seen["sims"].abs().max()).any()):
            return None, s
        if objective.requires_grad:
            book.embeddings.grad = None
            objective.backward()
        data[f"x{s}"] = x.detach().numpy()
        data[f"r{s}"] = r.numpy()
        data[f"quantize{s}"] = q.detach().numpy()
        data[f"embed_ind{s}"] = ind.numpy().astype(np.int32)
        data[f"gx{s}"] = (x.grad if x.grad is not None else torch.zeros_like(x)).numpy().copy()
        if c.get("learnable", False):
            data[f"gcb{s}"] = book.embeddings.grad.numpy().copy()
        for name in (*STAT_BUFFERS, *EMA_BUFFERS):
            data[f"{name}{s}"] = getattr(book, name).detach().numpy().copy()
        if s == 0:
            data["state_keys_json"] = np.frombuffer(json.dumps(list(book.state_dict().keys())).encode(), dtype=np.uint8)
    return data, None


def main():
    ref, ref_cb = _import_reference()
    torch.set_num_threads(4)
    only = sys.argv[1:]
    for name, c in AFFINE_CASES.items():
        if only and name not in only:
            continue
        seeds = [step["seed"] for step in c["steps"]]
        for _attempt in range(50):
            torch.manual_seed(777)
            data, failed = run_case(ref, ref_cb, c, seeds)
            if failed is None:
                break
            seeds[failed] += 1000  # reseed the step whose margin failed
        assert failed is None, f"{name}: no seed gives every row a margin of {MARGIN} * max|s|"
        meta = dict(case=c, seeds=seeds, affine=AFFINE, margin=MARGIN, torch=torch.__version__, threads=torch.get_num_threads())
        data["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, "data", f"affine_{name}.npz"), **data)
        print(f"affine_{name:18s} seeds {seeds} |batch_mean| {np.abs(data['batch_mean0']).max():.4g}")


if __name__ == "__main__":
    main()
