"""Timings beyond the bench of record: similarity-consuming entry points, training-mode forwards / full steps at cfg2 and
cfg4, cfg1 latency with and without hipGraph replay (diagnostic; DESIGN.md quotes these).

    python tools/loss_bench.py            # on the GPU box
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vector-quantization-by-ml_amd"))

import vector_quantization as vq  # noqa: E402
from vector_quantization import native  # noqa: E402
from vector_quantization.codebooks import CodebookParams  # noqa: E402


def timed(fn, n=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    dev = "cuda:0"
    M, K, D = 262144, 1024, 256
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((1, M, D), device=dev, generator=g)
    cb = torch.randn((1, K, D), device=dev, generator=g)
    tgt = torch.randint(0, K, (1, M), device=dev, generator=g)
    packed = native.pack_codebooks(cb, 0)
    flops = 2.0 * M * K * D
    t = timed(lambda: native.quantize(x, cb[:, None], packed=packed, want_best=False))
    print(f"search (reference point)        {t:8.3f} ms  {flops / t / 1e9:7.1f} TFLOP/s")
    t = timed(lambda: native.softmax_stats(x, cb, target=tgt, packed=packed))
    print(f"softmax stats (CE forward)      {t:8.3f} ms  {flops / t / 1e9:7.1f} TFLOP/s")
    lse, tl = native.softmax_stats(x, cb, target=tgt, packed=packed)
    coef = torch.tensor([1.0 / M], device=dev)
    for env in ("", "1"):
        if env:
            os.environ["VQ_CE_NO_ROLES"] = env
        t = timed(lambda: native.ce_backward(x, cb, lse, tl, tgt, coef, packed=packed))
        os.environ.pop("VQ_CE_NO_ROLES", None)
        print(f"CE backward ({'one-wave kernel' if env else 'wave-pair roles'})  {t:8.3f} ms  {2 * flops / t / 1e9:7.1f} TFLOP/s "
              f"({2 * flops / t / 1e9 / 157.3:.3f} of peak)")
    # the same kernels on a long sweep (K = 8192): the per-block costs amortised
    M8, K8 = 65536, 8192
    x8 = x[:, :M8].contiguous()
    cb8 = torch.randn((1, K8, D), device=dev, generator=g)
    tgt8 = torch.randint(0, K8, (1, M8), device=dev, generator=g)
    pk8 = native.pack_codebooks(cb8, 0)
    lse8, tl8 = native.softmax_stats(x8, cb8, target=tgt8, packed=pk8)
    f8 = 4.0 * M8 * K8 * D
    t = timed(lambda: native.ce_backward(x8, cb8, lse8, tl8, tgt8, coef, packed=pk8), n=5, warm=2)
    print(f"CE backward D=256 K=8192 M=65536 (wave-pair roles)  {t:8.3f} ms  {f8 / t / 1e9:7.1f} TFLOP/s ({f8 / t / 1e9 / 157.3:.3f} of peak)")
    t = timed(lambda: native.softmax_stats(x8, cb8, target=tgt8, packed=pk8), n=5, warm=2)
    print(f"softmax stats D=256 K=8192 M=65536  {t:8.3f} ms  {f8 / 2 / t / 1e9:7.1f} TFLOP/s ({f8 / 2 / t / 1e9 / 157.3:.3f} of peak)")
    # D = 512 (cfg3b's per-head shape): four roles per row block against the one-wave kernel (two workgroups per row block)
    M5, K5, D5 = 65536, 8192, 512
    x5 = torch.randn((1, M5, D5), device=dev, generator=g)
    cb5 = torch.randn((1, K5, D5), device=dev, generator=g)
    tgt5 = torch.randint(0, K5, (1, M5), device=dev, generator=g)
    pk5 = native.pack_codebooks(cb5, 0)
    lse5, tl5 = native.softmax_stats(x5, cb5, target=tgt5, packed=pk5)
    f5 = 4.0 * M5 * K5 * D5
    for env in ("", "1"):
        if env:
            os.environ["VQ_CE_NO_ROLES"] = env
        t = timed(lambda: native.ce_backward(x5, cb5, lse5, tl5, tgt5, coef, packed=pk5), n=5, warm=2)
        os.environ.pop("VQ_CE_NO_ROLES", None)
        print(f"CE backward D=512 K=8192 M=65536 ({'one-wave kernel' if env else 'four roles'})  {t:8.3f} ms  {f5 / t / 1e9:7.1f} TFLOP/s "
              f"({f5 / t / 1e9 / 157.3:.3f} of peak, algorithmic 4MKD)")
    out = torch.empty((1, 65536, K), device=dev)
    t = timed(lambda: native.similarities(x[:, :65536], cb, packed=packed, out=out))
    print(f"similarities, 65536-row chunk   {t:8.3f} ms  {flops / 4 / t / 1e9:7.1f} TFLOP/s  {out.numel() * 4 / t / 1e6:7.1f} GB/s written")

    mod = vq.VectorQuantize(dim=D, codebook_params=CodebookParams(dim=D, codebook_size=K),
                            commitment_use_cross_entropy_loss=True).to(dev).train()
    xs = torch.randn(256, 1024, D, device=dev, requires_grad=True)

    def step():
        xs.grad = None
        q, i, loss = mod(xs, freeze_codebook=True)
        loss.sum().backward()

    t = timed(step, n=3, warm=1)
    print(f"VectorQuantize CE commitment, forward + backward (train, frozen codebook)  {t:8.2f} ms")

    def fwd():
        with torch.no_grad():
            mod(xs, freeze_codebook=True)

    t = timed(fwd, n=5, warm=2)
    print(f"VectorQuantize CE commitment, forward only                                 {t:8.2f} ms")


def train_steps():
    """Training-mode module forwards at cfg2 (no autograd): search + straight-through + loss (+ EMA codebook update)."""
    dev = "cuda:0"
    D, K = 256, 1024
    xs = torch.randn(256, 1024, D, device=dev)
    for name, kw, fkw in (
        ("train, MSE commitment, codebook frozen", {}, dict(freeze_codebook=True)),
        ("train, MSE commitment, EMA codebook update", {}, {}),
        ("train, cross-entropy commitment, EMA codebook update", dict(commitment_use_cross_entropy_loss=True), {}),
    ):
        mod = vq.VectorQuantize(dim=D, codebook_params=CodebookParams(dim=D, codebook_size=K, threshold_ema_dead_code=0),
                                **kw).to(dev).train()

        def fwd():
            with torch.no_grad():
                mod(xs, **fkw)

        t = timed(fwd, n=10, warm=3)
        print(f"VectorQuantize forward, {name:55s} {t:8.3f} ms  {xs.shape[0] * xs.shape[1] / t / 1e3:8.1f} M rows/s")


def train_backward():
    """Standard training step at cfg2: forward (search + STE + MSE commitment + EMA) and backward to x."""
    dev = "cuda:0"
    D, K = 256, 1024
    mod = vq.VectorQuantize(dim=D, codebook_params=CodebookParams(dim=D, codebook_size=K, threshold_ema_dead_code=0)).to(dev).train()
    xs = torch.randn(256, 1024, D, device=dev, requires_grad=True)
    w = torch.randn(256, 1024, D, device=dev)

    def step():
        xs.grad = None
        q, i, loss = mod(xs)
        ((q * w).sum() + loss.sum()).backward()

    def fwd_only():
        q, i, loss = mod(xs)

    t_full = timed(step, n=5, warm=2)
    t_fwd = timed(fwd_only, n=5, warm=2)
    print(f"VectorQuantize train step (MSE commitment, EMA): forward {t_fwd:.2f} ms, forward + backward {t_full:.2f} ms "
          f"(includes the (q*w).sum() objective: 2 passes)")


def rvq_train():
    """cfg4 ResidualVQ (Q = 8, K = 1024, D = 256, 65536 tokens): eval forward, train forward with EMA, full step."""
    dev = "cuda:0"
    mod = vq.ResidualVQ(dim=256, num_quantizers=8,
                        codebook_params=CodebookParams(dim=256, codebook_size=1024, threshold_ema_dead_code=0)).to(dev)
    with torch.no_grad():
        for i, layer in enumerate(mod.layers):
            layer._codebook.embeddings.mul_(2.0 ** (-i / 2))
            layer._codebook.embed_avg.copy_(layer._codebook.embeddings)
    xs = torch.randn(64, 1024, 256, device=dev, requires_grad=True)
    w = torch.randn(64, 1024, 256, device=dev)

    def ev():
        with torch.no_grad():
            mod(xs)

    def tr():
        with torch.no_grad():
            mod(xs)

    def step():
        xs.grad = None
        q, i, loss = mod(xs)
        ((q * w).sum() + loss.sum()).backward()

    mod.eval()
    t_eval = timed(ev, n=5, warm=2)
    mod.train()
    t_train = timed(tr, n=5, warm=2)
    t_step = timed(step, n=5, warm=2)
    print(f"ResidualVQ cfg4: eval forward {t_eval:.2f} ms, train forward with EMA {t_train:.2f} ms, forward + backward {t_step:.2f} ms")




def cfg1_latency():
    """cfg1 (the reference's CPU-sized case): eager module forward vs hipGraph replay."""
    dev = "cuda:0"
    mod = vq.VectorQuantize(dim=64, codebook_params=CodebookParams(dim=64, codebook_size=256)).to(dev).eval()
    x = torch.randn(32, 256, 64, device=dev)

    def eager():
        with torch.no_grad():
            mod(x)

    fast = vq.GraphedForward(mod, x)
    t_e = timed(eager, n=200, warm=20)
    t_g = timed(lambda: fast(x), n=200, warm=20)
    print(f"cfg1 VectorQuantize [32,256,64] K=256: eager forward {t_e * 1e3:.1f} us, GraphedForward {t_g * 1e3:.1f} us "
          f"({8192 / t_g / 1e3:.1f} M rows/s)")


def half_inference():
    """cfg2 eval forward on bf16 activations: rows widened inside the search kernel vs a .float() pass in front of it."""
    dev = "cuda:0"
    mod = vq.VectorQuantize(dim=256, codebook_params=CodebookParams(dim=256, codebook_size=1024)).to(dev).eval()
    xb = torch.randn(256, 1024, 256, device=dev).to(torch.bfloat16)
    xf = xb.float()

    def native_half():
        with torch.no_grad():
            mod(xb)

    def cast_first():
        with torch.no_grad():
            mod(xb.float())

    def fp32():
        with torch.no_grad():
            mod(xf)

    t32, tc, th = timed(fp32, n=20, warm=10), timed(cast_first, n=20, warm=10), timed(native_half, n=20, warm=10)
    print(f"cfg2 eval forward: fp32 rows {t32:.3f} ms | bf16 rows, .float() first {tc:.3f} ms | bf16 rows widened in the kernel "
          f"{th:.3f} ms ({262144 / th / 1e3:.1f} M rows/s)")


def _rounds(variants, rounds=7, n=3, warm=2):
    """variants {name: fn}: the variants alternate in this process, `rounds` rounds of `n` calls each between HIP events after
    `warm` untimed calls -> {name: (median ms, min, max)}."""
    times = {name: [] for name in variants}
    for name, fn in variants.items():
        for _ in range(warm):
            fn()
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, n=n, warm=0))
    return {name: (sorted(t)[len(t) // 2], min(t), max(t)) for name, t in times.items()}


def _with_env(name, fn):
    def run():
        os.environ[name] = "1"
        try:
            fn()
        finally:
            os.environ.pop(name, None)
    return run


def ce_live():
    """The cross-entropy commitment step with the EMA update RUNNING (not frozen): backward through vq_ce_backward_live_f32
    against the chunked path (VQ_CE_NO_LIVE=1), module forward + backward; then the live kernel alone against
    vq_ce_backward_f32 on the same inputs.  `python tools/loss_bench.py ce_live`"""
    dev = "cuda:0"
    for shape, K in (((256, 1024, 256), 1024), ((64, 1024, 64), 8192), ((64, 1024, 128), 1024), ((64, 1024, 32), 1024)):
        D = shape[-1]
        mod = vq.VectorQuantize(dim=D, codebook_params=CodebookParams(dim=D, codebook_size=K, threshold_ema_dead_code=0),
                                commitment_use_cross_entropy_loss=True).to(dev).train()
        xs = torch.randn(*shape, device=dev, requires_grad=True)

        def step():
            xs.grad = None
            q, i, loss = mod(xs)
            loss.sum().backward()

        def step_frozen():
            xs.grad = None
            q, i, loss = mod(xs, freeze_codebook=True)
            loss.sum().backward()

        res = _rounds({"fused live": step, "chunked (VQ_CE_NO_LIVE=1)": _with_env("VQ_CE_NO_LIVE", step), "frozen codebook": step_frozen})
        for name, (med, lo, hi) in res.items():
            print(f"CE commitment step, EMA update, x {list(shape)} K={K}: {name:27s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})")
        del mod, xs
    g = torch.Generator(device=dev).manual_seed(0)
    for M, K, D in ((262144, 1024, 256), (65536, 8192, 64), (65536, 1024, 128), (65536, 1024, 32)):
        x = torch.randn((1, M, D), device=dev, generator=g)
        cb = torch.randn((1, K, D), device=dev, generator=g)
        live = 0.8 * cb + 0.2 * torch.randn((1, K, D), device=dev, generator=g)
        tgt = torch.randint(0, K, (1, M), device=dev, generator=g)
        pk, lpk = native.pack_codebooks(cb, 0), native.pack_codebooks(live, 0)
        lse, tl = native.softmax_stats(x, cb, target=tgt, packed=pk)
        coef = torch.tensor([1.0 / M], device=dev)
        variants = {
            "live": lambda: native.ce_backward(x, cb, lse, tl, tgt, coef, packed=pk, live=live, live_packed=lpk),
            "not live": lambda: native.ce_backward(x, cb, lse, tl, tgt, coef, packed=pk),
        }
        if D > 128:
            variants["not live, VQ_CE_NO_ROLES=1"] = _with_env("VQ_CE_NO_ROLES", variants["not live"])
        f = 4.0 * M * K * D
        for name, (med, lo, hi) in _rounds(variants, n=5).items():
            print(f"CE backward kernel M={M} K={K} D={D}: {name:27s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {f / med / 1e9:6.1f} TFLOP/s "
                  f"({f / med / 1e9 / 157.3:.3f} of peak)")


if __name__ == "__main__":
    if sys.argv[1:] == ["ce_live"]:
        ce_live()
        sys.exit(0)
    half_inference()
    main()
    train_steps()
    train_backward()
    rvq_train()
    cfg1_latency()
    ce_live()
