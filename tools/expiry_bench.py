"""What the dead-code expiry's host synchronisation costs a training step, and what expire_on_device does about it: train-mode
forwards queued back to back without a synchronise in between, with the expiry on the host path (the default: ``.any()`` makes
the host wait for the GPU once per codebook and step) and on the device (``set_expire_on_device``), alternating round by round
in one process on twins of one module.  The shapes are BASELINE.md's cfg2 (VectorQuantize, 256 x 1024 rows of dim 256,
K = 1024) and cfg4 (ResidualVQ, Q = 8, 16 x 1024 rows), with ``threshold_ema_dead_code=2``; a third line runs cfg2's module on
16 x 1024 rows, where the step is short enough for the host to be what limits it.  DESIGN.md section 23 quotes these; the raw
lines are kept in profiles/device_expiry.md.

    python tools/expiry_bench.py [--rounds 7] [--steps 20] [--out FILE]     # on the GPU box
"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vector-quantization-by-ml_amd"))

import vector_quantization as vq  # noqa: E402
from vector_quantization.codebooks import CodebookParams  # noqa: E402

DEV = "cuda:0"
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def steps_ms(mod, xs, steps):
    """wall milliseconds per step of ``steps`` training forwards queued without a synchronise in between (host clock around work
    that ends in a device synchronise), and the same span by device events"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    with torch.no_grad():
        for i in range(steps):
            mod(xs[i % len(xs)])
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps, e0.elapsed_time(e1) / steps


def books(mod):
    return [m for m in mod.modules() if isinstance(m, vq.Codebook)]


def compare(title, make, shape, rounds, steps):
    torch.manual_seed(0)
    host = make().to(DEV).train()
    device = vq.set_expire_on_device(copy.deepcopy(host))
    xs = [torch.randn(shape, device=DEV) for _ in range(4)]
    variants = {"host expiry (default)": host, "expire_on_device": device}
    for mod in variants.values():  # warm-up of every shape and launch path; the first steps also expire the untrained codes
        steps_ms(mod, xs, 6)
    wall = {name: [] for name in variants}
    dev = {name: [] for name in variants}
    for _ in range(rounds):
        for name, mod in variants.items():
            w, d = steps_ms(mod, xs, steps)
            wall[name].append(w)
            dev[name].append(d)
    say(f"{title}: input {list(shape)}, {len(books(host))} codebook(s), {rounds} rounds x {steps} steps, alternating")
    for name in variants:
        w, d = wall[name], dev[name]
        say(f"  {name:22s} wall {statistics.median(w):8.3f} ms/step (min {min(w):.3f}, max {max(w):.3f}; spread "
            f"{(max(w) - min(w)) / statistics.median(w) * 100:.1f} %)   device events {statistics.median(d):8.3f} ms/step")
        say(f"  {'':22s} rounds: " + " ".join(f"{v:.3f}" for v in w))
    base, new = statistics.median(wall["host expiry (default)"]), statistics.median(wall["expire_on_device"])
    spread = max(wall["host expiry (default)"]) - min(wall["host expiry (default)"])
    say(f"  expire_on_device / default = {new / base:.3f} (difference {new - base:+.3f} ms; the default's own min-max spread "
        f"{spread:.3f} ms)")
    dead = [int((b.cluster_size < b.threshold_ema_dead_code).sum()) for b in books(device)]
    say(f"  codes below the threshold after the last step (expire_on_device twin): {dead}")
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("expiry_bench.py measures on the GPU: no device is visible")
    params = CodebookParams(dim=256, codebook_size=1024, threshold_ema_dead_code=2)
    say(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    compare("cfg2 VectorQuantize dim=256 K=1024", lambda: vq.VectorQuantize(dim=256, codebook_params=params), (256, 1024, 256),
            a.rounds, a.steps)
    compare("cfg4 ResidualVQ Q=8 K=1024 dim=256", lambda: vq.ResidualVQ(dim=256, num_quantizers=8, codebook_params=params),
            (16, 1024, 256), a.rounds, a.steps)
    compare("cfg2 module on 16 x 1024 rows", lambda: vq.VectorQuantize(dim=256, codebook_params=params), (16, 1024, 256),
            a.rounds, a.steps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
