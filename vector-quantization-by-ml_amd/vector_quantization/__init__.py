"""MI355X-native drop-in for the nearest-codebook hot path of MisterBourbaki/vector-quantization-by-ml.

Import surface kept from the reference (``vector_quantization/__init__.py:11-12,16-28``):

    from vector_quantization import VectorQuantize, ResidualVQ, GroupedResidualVQ
    from vector_quantization.codebooks import CodebookParams, KmeansParameters, GumbelParams, AffineParameters, Codebook

The search itself (distance -> first argmax -> gather, straight-through, squared error, residual loop) is
hand-written HIP for gfx950 behind the C ABI in ``include/vq_mi355x.h``; there is no PyTorch/CPU fallback.
``LFQ`` (lookup-free quantization) runs its sign quantizer and its entropy aux loss -- a sweep over an implicit codebook
of 2^d codes -- in HIP as well, and so do ``ResidualLFQ`` / ``GroupedResidualLFQ`` (every stage's quantize step in one
fused pass, every stage's entropy terms in one stage-batched call).  ``FSQ`` (finite scalar quantization) and
``ResidualFSQ`` / ``GroupedResidualFSQ`` run bound, round, index and every residual stage of every group in one HIP pass,
and their backward in one more.  ``LatentQuantize`` (latent quantization: every latent dimension against its own learnable
table of values) runs the per-dimension level search, the straight-through value, the index and the squared-error loss
in one HIP pass over the caller's channel-first tensor.
"""
from . import ops  # noqa: F401  (registers torch.ops.vq_mi355x.*)
from .codebook import Codebook, set_expire_on_device
from .finite_scalar_quantization import FSQ
from .graphs import GraphedForward, GraphedTrainForward
from .latent_quantization import LatentQuantize
from .lookup_free_quantization import LFQ
from .params import AffineParameters, CodebookParams, GumbelParams, KmeansParameters
from .projection import RandomProjectionQuantizer
from .quantizer import LossBreakdown, VectorQuantize
from .residual import GroupedResidualVQ, ResidualVQ
from .residual_fsq import GroupedResidualFSQ, ResidualFSQ
from .residual_lfq import GroupedResidualLFQ, ResidualLFQ
from .sharded import ShardedCodebookSearch

__all__ = [
    "AffineParameters",
    "Codebook",
    "CodebookParams",
    "FSQ",
    "GraphedForward",
    "GraphedTrainForward",
    "GroupedResidualFSQ",
    "GroupedResidualLFQ",
    "GroupedResidualVQ",
    "GumbelParams",
    "KmeansParameters",
    "LFQ",
    "LatentQuantize",
    "LossBreakdown",
    "RandomProjectionQuantizer",
    "ResidualFSQ",
    "ResidualLFQ",
    "ResidualVQ",
    "ShardedCodebookSearch",
    "VectorQuantize",
    "set_expire_on_device",
]
