"""Cases of the cross-entropy fixtures with a learnable codebook (make_golden_ce_codes.py writes them, the tests read them).

Every case is VectorQuantize(..., CodebookParams(learnable_codebook=True, ema_update=False)) in train mode; the objective is
the module's loss alone (the cross entropy of the similarities), so dL/dx and dL/dcodebook are the cross entropy's.  The
configurations are those of the frozen-codebook fixtures of the same names in cases.py (ce_commit, ce_commit_mask, ...)."""

_CE = dict(commitment_use_cross_entropy_loss=True)
_MH = dict(heads=2, codebook_dim=32)

CE_CODES_CASES = {
    "commit": dict(dim=64, K=256, x_shape=(4, 64, 64), vq=_CE),
    "commit_mask": dict(dim=64, K=256, x_shape=(3, 40, 64), vq=_CE, mask=True),
    "indices_ignore": dict(dim=64, K=256, x_shape=(4, 64, 64), vq={}, given_indices=True, ignore_some=True),
    "cos": dict(dim=64, K=256, x_shape=(4, 64, 64), vq=_CE, cosine=True),
    "mh_sep": dict(dim=64, K=128, x_shape=(2, 50, 64), vq=dict(_CE, separate_codebook_per_head=True, **_MH)),
    "mh_shared": dict(dim=64, K=128, x_shape=(2, 50, 64), vq=dict(_CE, **_MH)),
}
