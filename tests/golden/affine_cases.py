"""Cases of the use_affine fixtures (make_golden_affine.py writes them, the tests read them).

``kind`` "codebook": a direct ``Codebook(use_affine=True, affine_params=AffineParameters(...))`` -- the reference's
``VectorQuantize(use_affine=True)`` crashes on its first forward, so the ``Codebook`` pins the semantics.
``kind`` "vq": a reference ``VectorQuantize`` built without affine whose ``_codebook`` is swapped for such a ``Codebook``.

Every case runs ``steps`` forwards in a row on ONE module; a step is dict(seed=.., train=.., offset=.., mask=..).  The codes
start from gen.make_codebook(h, K, D, "S") with warm EMA statistics (embed_avg = 10 * codes, cluster_size = 10); dead codes
are never re-seeded (threshold_ema_dead_code = 0: the re-seeding draws random rows)."""

DIM, K = 32, 64
X_SHAPE = (2, 96, 32)
AFFINE = dict(sync=False, batch_decay=0.9, codebook_decay=0.8)


def _step(seed, train=True, offset=0.0, mask=False):
    return dict(seed=seed, train=train, offset=offset, mask=mask)


AFFINE_CASES = {
    "first": dict(kind="codebook", steps=[_step(1234)]),
    "three": dict(kind="codebook", steps=[_step(1234), _step(1235), _step(1236)]),
    "mask": dict(kind="codebook", steps=[_step(1234, mask=True), _step(1235, mask=True)]),
    "heads": dict(kind="codebook", heads=2, steps=[_step(1234), _step(1235)]),
    "cosine": dict(kind="codebook", cosine=True, steps=[_step(1234), _step(1235)]),
    "offset": dict(kind="codebook", steps=[_step(1234, offset=3.0), _step(1235, offset=3.0)]),
    "eval_after_train": dict(kind="codebook", steps=[_step(1234), _step(1235, train=False)]),
    "learnable": dict(kind="codebook", learnable=True, steps=[_step(1234), _step(1235)]),
    "vq_train": dict(kind="vq", steps=[_step(1234), _step(1235)]),
    "vq_ce": dict(kind="vq", vq=dict(commitment_use_cross_entropy_loss=True), steps=[_step(1234), _step(1235)]),
}

STAT_BUFFERS = ("batch_mean", "batch_variance", "codebook_mean", "codebook_variance", "codebook_mean_needs_init",
                "codebook_variance_needs_init")
EMA_BUFFERS = ("cluster_size", "embed_avg", "embeddings")
