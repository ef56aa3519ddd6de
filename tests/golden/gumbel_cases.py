"""Cases of the Gumbel straight-through / reinmax fixtures (make_golden_gumbel.py writes them, the tests read them).

``kind`` "vq": VectorQuantize(dim=32, K=64, learnable_codebook=True, ema_update=False) on x [2, 40, 32];
``kind`` "codebook": a direct Codebook.forward in training with ema_update=True (the live-codes quirk)."""

T = 0.7

GUMBEL_CASES = {
    "st_euclid": dict(kind="vq", gumbel=dict(straight_through=True, temperature=T)),
    "st_cos": dict(kind="vq", gumbel=dict(straight_through=True, temperature=T), cosine=True),
    "st_heads": dict(kind="vq", gumbel=dict(straight_through=True, temperature=T),
                     vq=dict(heads=2, separate_codebook_per_head=True, codebook_dim=16)),
    "st_mask": dict(kind="vq", gumbel=dict(straight_through=True, temperature=T), mask=True),
    "st_sgd": dict(kind="vq", gumbel=dict(straight_through=True, temperature=T), sgd_lr=0.5),
    "rm_euclid": dict(kind="vq", gumbel=dict(straight_through=True, reinmax=True, temperature=T)),
    "rm_cos": dict(kind="vq", gumbel=dict(straight_through=True, reinmax=True, temperature=T), cosine=True),
    "ema_live": dict(kind="codebook", gumbel=dict(straight_through=True, temperature=T)),
    # inactive relaxations: the gradients are the plain path's
    "t0": dict(kind="vq", gumbel=dict(straight_through=True, temperature=0.0)),
    "not_training": dict(kind="vq", gumbel=dict(straight_through=True, temperature=T, training=False)),
}

X_SHAPE = (2, 40, 32)
DIM, K = 32, 64
