"""One training step of a learnable codebook with the cross-entropy commitment loss, timed for ONE build of the package per
process (profiles/ce_codes_bench.md keeps the table; the method is that of profiles/diversity_codes_bench.md):

    VectorQuantize(dim=D, CodebookParams(dim=D, codebook_size=K, learnable_codebook=True, ema_update=False),
                   commitment_use_cross_entropy_loss=True), train mode, x [B, N, D] with x.requires_grad;
    one step = forward + loss.sum().backward()

HIP events around each step, the median after the warm-up, torch.cuda.max_memory_allocated over the timed steps.  Run it
once per build and alternate the builds in one session:

    python tools/ce_codes_bench.py --label fused             # --set scan: the row scan [rows, 1024, D]
    VQ_CE_CODES_NO_FUSED=1 python tools/ce_codes_bench.py --label chunked
    python tools/ce_codes_bench.py --pkg /path/to/parent/checkout/vector-quantization-by-ml_amd --label parent

Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, N, D, K, timed steps)
SHAPES = {
    "main": [(256, 1024, 256, 1024, 5), (64, 1024, 64, 8192, 5)],
    # the row scan: M = rows * 1024 rows of one head, per padded row width
    "scan": [(b, 1024, d, k, 10) for d in (32, 64, 128, 256) for k in (1024, 8192) for b in (1, 4, 16)],
    # below one sequence: where a cut could lie
    "few": [(1, n, d, k, 20) for d in (32, 64, 128, 256) for k in (1024, 8192) for n in (32, 256)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "vector-quantization-by-ml_amd"), help="directory that holds the package to time")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--set", default="main", choices=sorted(SHAPES))
    ap.add_argument("--codes-min-rows", type=int, default=None,
                    help="lower every cut of losses.CE_CODES_FUSED_MIN_ROWS to this, so that the fused path is measured below the cut")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    assert os.path.abspath(vq.__file__).startswith(os.path.abspath(args.pkg)), vq.__file__
    if args.codes_min_rows is not None:
        from vector_quantization import losses

        losses.CE_CODES_FUSED_MIN_ROWS = {dp: args.codes_min_rows for dp in losses.CE_CODES_FUSED_MIN_ROWS}
    for b, n, d, k, steps in SHAPES[args.set]:
        torch.manual_seed(7)
        params = CodebookParams(dim=d, codebook_size=k, learnable_codebook=True, ema_update=False)
        mod = vq.VectorQuantize(dim=d, codebook_params=params, commitment_use_cross_entropy_loss=True).cuda().train()
        x = torch.randn((b, n, d), device="cuda", requires_grad=True)

        def step():
            mod.zero_grad(set_to_none=True)
            x.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, _, loss = mod(x)
            loss.sum().backward()
            e1.record()
            return e0, e1

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        events = [step() for _ in range(steps)]
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in events]
        grad = mod._codebook.embeddings.grad
        print(json.dumps(dict(label=args.label, x=[b, n, d], K=k, rows=b * n, ms_median=round(statistics.median(ms), 3),
                              ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), steps=steps,
                              peak_mib=round(torch.cuda.max_memory_allocated() / 2**20),
                              sum_abs_codes_grad=float(grad.abs().sum()), sum_abs_x_grad=float(x.grad.abs().sum()))), flush=True)
        del mod, x, events
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
