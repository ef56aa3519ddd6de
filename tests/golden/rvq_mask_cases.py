"""The masked residual-stack cases shared by make_golden_rvq_mask.py (which imports the reference) and the tests (which never
do).  One small stack -- ResidualVQ(dim=32, num_quantizers=4, K=64) on [3, 40, 32], seeded class-"S" codebooks
(gen.make_rvq_codebooks) -- with ragged lengths 40 / 17 / 1: a full sequence, a partial one and one kept row."""
from __future__ import annotations

import torch

DIM, Q, K = 32, 4, 64
X_SHAPE = (3, 40, DIM)
LENGTHS = (40, 17, 1)
GROUPS = 2  # the grouped case: dim = GROUPS * DIM


def make_mask(lengths=LENGTHS, n=X_SHAPE[1]) -> torch.Tensor:
    mask = torch.zeros((len(lengths), n), dtype=torch.bool)
    for i, length in enumerate(lengths):
        mask[i, :length] = True
    return mask


def _case(name, **kw):
    c = dict(name=name, kind="rvq", training=False, freeze_codebook=True, shared_codebook=False, grad=False, rvq_extra={},
             fwd_extra={}, cb_extra={}, nonfinite=None)
    c.update(kw)
    return c


CASES = [
    _case("rvq_mask_eval"),
    _case("rvq_mask_train", training=True, grad=True),
    # EMA after one step; the expiry draws rows at random, so it is off (threshold 0), as in the other *_ema goldens
    _case("rvq_mask_ema", training=True, freeze_codebook=False, cb_extra=dict(threshold_ema_dead_code=0)),
    _case("rvq_mask_shared", training=True, grad=True, shared_codebook=True),
    _case("rvq_mask_shared_eval", shared_codebook=True),
    _case("rvq_mask_dropout", training=True, grad=True,
          rvq_extra=dict(quantize_dropout=True, quantize_dropout_cutoff_index=0, quantize_dropout_multiple_of=1),
          fwd_extra=dict(rand_quantize_dropout_fixed_seed=3)),
    _case("rvq_mask_grouped", kind="grvq", training=True, grad=True),
    _case("rvq_mask_grouped_eval", kind="grvq"),
    # masked-out rows holding a non-finite element: row 60 (sequence 1, position 20) an inf, row 100 (sequence 2, position
    # 20) a NaN; and kept rows next to them stay as they were
    _case("rvq_mask_nonfinite", nonfinite=dict(x=[[60, 5, "inf"], [100, 0, "nan"]])),
    _case("rvq_mask_nonfinite_train", training=True, nonfinite=dict(x=[[60, 5, "-inf"], [100, 31, "nan"]])),
]

BY_NAME = {c["name"]: c for c in CASES}
