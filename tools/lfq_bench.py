#!/usr/bin/env python3
"""Time the LFQ entropy aux loss (forward + backward) on one GPU: the native kernels against a dense torch
restatement that builds the [rows, 2^d] softmax the way the reference does (lookup_free_quantization.py:294-331),
capped at rows * 2^d <= 2^30 elements.  HIP events around each step; peak device memory above the inputs.

    python tools/lfq_bench.py [--steps 20] [--warmup 5]      # prints one JSON line per (path, d, rows) and a table
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vector-quantization-by-ml_amd"))

import torch  # noqa: E402

from vector_quantization.lookup_free_quantization import _LfqEntropy  # noqa: E402


def native_step(v, tau):
    ps, cb = _LfqEntropy.apply(v, None, 1.0, tau)
    (ps - cb).backward()


def dense_step(v, tau, codes):
    def entropy(p):
        return (-p * p.clamp(min=1e-5).log()).sum(-1)

    prob = (2.0 * tau * torch.einsum("ncd,kd->nck", v, codes)).softmax(dim=-1)
    ps = entropy(prob).mean()
    avg = prob.mean(dim=0)
    cb = entropy(avg).mean()
    (ps - cb).backward()


def measure(fn, v, steps, warmup):
    for _ in range(warmup):
        v.grad = None
        fn()
    torch.cuda.synchronize()
    v.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = []
    for _ in range(steps):
        v.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dims", default="10,14,16")
    ap.add_argument("--rows", default="8192,32768")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tau = 1.0
    table = []
    for d in (int(s) for s in args.dims.split(",")):
        bits = (torch.arange(1 << d, device=dev)[:, None] >> torch.arange(d - 1, -1, -1, device=dev)) & 1
        codes = (2.0 * bits - 1.0).float()
        for rows in (int(s) for s in args.rows.split(",")):
            g = torch.Generator(device=dev).manual_seed(d * 100003 + rows)
            v = (torch.randn(rows, 1, d, device=dev, generator=g) * 0.5).requires_grad_(True)
            ms, mib = measure(lambda: native_step(v, tau), v, args.steps, args.warmup)
            bound = (rows * 2 * 2 ** ((d + 1) // 2) + (1 << d)) * 4 / 2**20
            rec = dict(path="native", d=d, rows=rows, ms=round(ms, 4), peak_mib=round(mib, 1), bound_units_mib=round(bound, 1))
            print(json.dumps(rec), flush=True)
            dense = None
            if rows * (1 << d) <= 2**30:
                dms, dmib = measure(lambda: dense_step(v, tau, codes), v, max(3, args.steps // 4), 2)
                dense = dict(path="dense", d=d, rows=rows, ms=round(dms, 3), peak_mib=round(dmib, 1))
                print(json.dumps(dense), flush=True)
            table.append((d, rows, rec, dense))
            del v
            torch.cuda.empty_cache()
    print("\n| d | rows | native fwd+bwd (ms) | native peak (MiB) | dense fwd+bwd (ms) | dense peak (MiB) |")
    print("|---|---|---|---|---|---|")
    for d, rows, rec, dense in table:
        dm = f"{dense['ms']:.3f}" if dense else "not run (> 2^30 elements)"
        dp = f"{dense['peak_mib']:.0f}" if dense else "-"
        print(f"| {d} | {rows} | {rec['ms']:.3f} | {rec['peak_mib']:.1f} | {dm} | {dp} |")


if __name__ == "__main__":
    main()
