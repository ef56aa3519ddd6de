"""Configuration dataclasses of the drop-in API.

Field names and defaults ARE the public API of the reference (``CodebookParams`` is what callers pass to
``VectorQuantize(codebook_params=...)``), so they are kept identical:
/root/reference/vector_quantization/codebooks.py:31-78.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional


@dataclass
class AffineParameters:
    """Affine re-parameterisation of a codebook (``use_affine=True``): the codes are searched after being moved to the
    running per-column mean / variance of the batch, ``(codes - codebook_mean) * (batch_std / codebook_std) + batch_mean``,
    and the EMA step sees the rows moved the other way.  ``batch_decay`` / ``codebook_decay`` are the weights of the OLD
    running value (the first forward assigns); the codebook's statistics move only in train mode, the batch's in eval mode
    too.  ``sync``: in a distributed world the batch statistics are those of every rank's rows.  Native column statistics
    and transform kernels.  Not available with a sharded codebook, ``in_place_codebook_optimizer``
    or ``GumbelParams(straight_through=True)`` (NotImplementedError at construction)."""

    sync: bool
    batch_decay: float = 0.99
    codebook_decay: float = 0.9


@dataclass
class KmeansParameters:
    """Lloyd iterations used to seed the codebook from the first batch."""

    iter: int = 10
    sync: bool = True


@dataclass
class GumbelParams:
    """Options of the code selection: deterministic argmax (native, bit-exact) or stochastic Gumbel-max sampling (one native
    sweep with counter-based noise, seeded from torch's generator on the device).  ``straight_through`` (optionally with ``reinmax``) keeps the argmax selection and its value
    and adds the reference's gradient through ``softmax(similarities / temperature)`` to the encoder and to a learnable
    codebook; it is active at ``temperature > 0`` with ``training`` while the module is in train mode (gumbel.py).  On fp32
    rows of up to 256 dims both gradients are fused native sweeps (three for straight-through, four for ``reinmax``); wider
    rows run on bounded row chunks.
    ``reinmax`` needs ``straight_through``; ``stochastic`` together with ``straight_through`` raises NotImplementedError."""

    temperature: float = 1.0
    stochastic: bool = False
    reinmax: bool = False
    straight_through: bool = False
    dim: int = -1
    training: bool = True


@dataclass
class CodebookParams:
    dim: int
    codebook_size: int
    num_codebooks: int = 1
    initialization_by_kmeans: bool = False
    kmeans_params: Optional[KmeansParameters] = None
    decay: float = 0.8
    eps_for_smoothing: float = 1e-5
    threshold_ema_dead_code: int = 2
    reset_cluster_size: Optional[int] = None
    use_ddp: bool = False
    distributed_replace_codes: bool = True
    learnable_codebook: bool = False
    gumbel_params: GumbelParams = field(default_factory=GumbelParams)
    ema_update: bool = True
    use_affine: bool = False
    affine_params: Optional[AffineParameters] = None
    transform_input: str = "identity"
    use_cosine_sim: bool = False
    weights_regularization: str = "identity"
