"""Conditioning of the affine EMA step's sum identity r * sum(x) + hits * (cm - bm * r): worst deviation of
``embed_avg`` after the first step of the +3.0 offset fixture (and of the plain one) from an fp64 model of the reference's
formula, for this package's tensor-op path (CPU, checker backend) and for the reference's own recorded fp32 run.

    python tools/affine_conditioning.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-quantization-by-ml_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
from helpers import OracleBackend
from vector_quantization import search
from affine_run import build_module, run_step
search.set_backend(OracleBackend)
for name in ("offset", "first"):
    mod, book, arrays, c = build_module(name)
    run_step(mod, book, arrays, c, 0)
    x = torch.from_numpy(arrays["x0"]).double().reshape(1, -1, 32); cb = torch.from_numpy(arrays["cb"]).double()
    idx = torch.from_numpy(arrays["embed_ind0"]).long().reshape(1, -1)
    bm, bv = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    cm, cv = cb.mean(1, keepdim=True), cb.var(1, unbiased=False, keepdim=True)
    r = cv.clamp(min=1e-5).sqrt() / bv.clamp(min=1e-5).sqrt()
    moved = (x - bm) * r + cm
    onehot = torch.nn.functional.one_hot(idx, 64).double()
    avg64 = cb * 10 * 0.8 + 0.2 * (onehot.transpose(1, 2) @ moved)
    ref = torch.from_numpy(arrays["embed_avg0"]).double(); mine = book.embed_avg.double()
    print(name, "reference fp32 vs fp64: %.3e   identity (this package) vs fp64: %.3e   |embed_avg| max %.3f" % (
        float((ref - avg64).abs().max()), float((mine - avg64).abs().max()), float(avg64.abs().max())))
