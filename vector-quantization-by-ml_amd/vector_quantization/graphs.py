"""hipGraph replay of an eval-mode forward for latency-bound shapes (serving).

At the reference's CPU-sized configuration (cfg1: 8192 rows, K = 256, D = 64) the search kernel runs ~10 us but an eager
module forward costs several times that in Python / launch overhead.  The native launch functions allocate nothing and
never synchronise, so the whole forward -- codebook pack, search + gather, layout views -- can be captured once into a
hipGraph and replayed with one launch.

    fast = GraphedForward(vq_module.eval(), example_input)
    quantized, indices, loss = fast(x)          # x: same shape / dtype as the example; outputs are static buffers

The outputs are the graph's own static tensors: copy them if they must outlive the next call.  The codebook is read at
replay time (its buffer address is captured, not its values), so loading new weights in place needs no re-capture.

``GraphedTrainForward`` does the same for a train-mode forward without gradients -- search, EMA update and dead-code expiry in
one graph -- for modules whose codebooks expire their dead codes on the device (``set_expire_on_device``).
"""
from __future__ import annotations

import torch
from torch import nn


class GraphedForward:
    def __init__(self, module: nn.Module, example: torch.Tensor, warmup: int = 2, **forward_kwargs):
        if module.training:
            raise ValueError("GraphedForward captures inference: call module.eval() first (a training forward updates the "
                             "codebook, and its default dead-code expiry synchronises; GraphedTrainForward captures one "
                             "whose codebooks expire on the device)")
        if not example.is_cuda:
            raise ValueError("GraphedForward needs a ROCm device tensor")
        self._capture(module, example, warmup, forward_kwargs)

    def _capture(self, module, example, warmup, forward_kwargs):
        """Warm up on a side stream, then record one no-grad forward of ``module`` (in the mode it is in) on ``example``."""
        self.module = module
        self.static_in = example.clone()
        self._kwargs = forward_kwargs
        side = torch.cuda.Stream(device=example.device)
        side.wait_stream(torch.cuda.current_stream(example.device))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(max(1, warmup)):  # first calls set kernel attributes and query the device
                module(self.static_in, **forward_kwargs)
        torch.cuda.current_stream(example.device).wait_stream(side)
        torch.cuda.synchronize(example.device)
        # the modules cache the packed image of an unchanged codebook; the graph must contain the pack itself, so that a
        # replay reads the weights of its own time (in-place updates need no re-capture): drop the caches before capturing
        self._drop_packed_caches()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.static_out = module(self.static_in, **forward_kwargs)
        # the capturing forward refilled those caches with tensors from the graph's private pool whose pack kernels were only
        # RECORDED: until the first replay they hold uninitialised memory.  Drop them again, so that an eager module(x)
        # (e.g. the fallback for a batch shape the graph was not captured for) packs for itself.
        self._drop_packed_caches()

    def _drop_packed_caches(self):
        for m in self.module.modules():
            if hasattr(m, "invalidate_packed"):
                m.invalidate_packed()
            if hasattr(m, "_stage_cache"):
                m._stage_cache = None

    def __call__(self, x: torch.Tensor):
        if x.shape != self.static_in.shape or x.dtype != self.static_in.dtype:
            raise ValueError(f"captured for {tuple(self.static_in.shape)} {self.static_in.dtype}, "
                             f"got {tuple(x.shape)} {x.dtype}")
        self.static_in.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.static_out


class GraphedTrainForward(GraphedForward):
    """hipGraph replay of a TRAIN-mode forward without gradients: search, EMA update and dead-code expiry are nodes of the
    graph, so one replay is one whole training step of the codebooks (a tokenizer trained by EMA alone, or the codebook side of
    a step whose gradients are taken elsewhere).  Every ``Codebook`` below ``module`` must expire its dead codes on the device
    (``set_expire_on_device``): the default expiry step asks the host whether a code died, which a capture cannot record.

    The ``warmup`` forwards on ``example`` are real training steps: they move the codebooks.  Each replay draws a fresh
    expiry seed from torch's generator (the graph registers its Philox offset), so ``torch.manual_seed`` governs replays too.

        vq.set_expire_on_device(module.train())
        step = GraphedTrainForward(module, example_input)
        quantized, indices, loss = step(x)          # outputs are the graph's static tensors
    """

    def __init__(self, module: nn.Module, example: torch.Tensor, warmup: int = 2, **forward_kwargs):
        from .codebook import Codebook

        if not module.training:
            raise ValueError("GraphedTrainForward captures a training forward: call module.train() first "
                             "(GraphedForward captures inference)")
        books = [m for m in module.modules() if isinstance(m, Codebook)]
        if not books or not all(m.expire_on_device for m in books):
            raise ValueError("GraphedTrainForward needs expire_on_device on every Codebook below the module "
                             "(vector_quantization.set_expire_on_device): the default dead-code expiry synchronises")
        if not example.is_cuda:
            raise ValueError("GraphedTrainForward needs a ROCm device tensor")
        # (a replay reads the codes the previous replay left: the packs are nodes of the graph here too)
        self._capture(module, example, warmup, forward_kwargs)
