"""Host: the one fused residual-stack path (vector_quantization/residual.py) and the helpers the VQ, LFQ and FSQ stacks share
(vector_quantization/residual_common.py), driven on the CPU by the tests-only backends (tests/helpers.py:OracleBackend, and
the mask rule of tests/test_residual_mask_host.py:RuleBackend).

Three things are pinned: a single stack and a grouped stack of one group compute the same; every fused route hands the
backend the same calls, tensor layouts and keywords as before the two stacks shared their path; and every module consumes
``random`` as before.  The literals below (TRACES, NEXT_RANDOM) were read off the commit BEFORE the refactor that made the path
one, with this file's own recorder, and pasted here; they are not what the refactored code happens to give."""
from __future__ import annotations

import random

import pytest
import torch

from test_residual_mask_host import RuleBackend

DIM, K, Q = 8, 16, 3
X_SHAPE = (2, 5, DIM)
DROP = dict(quantize_dropout=True, quantize_dropout_cutoff_index=0, quantize_dropout_multiple_of=1)
CUT1_SEED = 7  # random.Random(7).randrange(0, 3) == 1 (asserted below): stages 0 and 1 run


def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def _x(groups=1):
    return _randn((*X_SHAPE[:-1], groups * DIM), 11)


def _mask():
    mask = torch.ones(X_SHAPE[:2], dtype=torch.bool)
    mask[0, 3:] = False
    mask[1, 1] = False
    return mask


def _build(kind, groups=1, training=False, **extra):
    """ResidualVQ / GroupedResidualVQ on seeded codebooks; group g of a grouped module holds the codebooks a single stack built
    with ``seed0 = 21 + 100 g`` holds."""
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    commitment = extra.pop("commitment_weight", 1.0)
    params = CodebookParams(dim=DIM, codebook_size=K, threshold_ema_dead_code=0)
    if kind == "grvq":
        mod = vq.GroupedResidualVQ(dim=groups * DIM, groups=groups, num_quantizers=Q, codebook_params=params,
                                   commitment_weight=commitment, **extra)
        rvqs = list(mod.rvqs)
    else:
        mod = vq.ResidualVQ(dim=DIM, num_quantizers=Q, codebook_params=params, commitment_weight=commitment, **extra)
        rvqs = [mod]
    with torch.no_grad():
        for g, rvq in enumerate(rvqs):
            for q, layer in enumerate(rvq.layers):
                cb = _randn((1, K, DIM), 21 + 100 * g + (0 if extra.get("shared_codebook") else q))
                layer._codebook.embeddings.copy_(cb)
                layer._codebook.embed_avg.copy_(cb)
    return mod.train(training)


def _ema_state(mod):
    layers = [layer for rvq in (mod.rvqs if hasattr(mod, "rvqs") else [mod]) for layer in rvq.layers]
    return {attr: torch.stack([getattr(layer._codebook, attr) for layer in layers])
            for attr in ("embeddings", "embed_avg", "cluster_size")}


@pytest.fixture
def backend():
    from vector_quantization import search

    RuleBackend.calls = []
    search.set_backend(RuleBackend)
    try:
        yield RuleBackend
    finally:
        search.set_backend(None)


# --------------------------------------------------------------------------------------- single stack vs. one group
@pytest.mark.parametrize("route", ["eval", "train", "train_mask", "eval_mask"])
def test_single_stack_is_a_grouped_stack_of_one_group(route, backend):
    training = route.startswith("train")
    mask = _mask() if route.endswith("mask") else None
    single, grouped = _build("rvq", training=training), _build("grvq", groups=1, training=training)
    x = _x()
    q1, i1, l1 = single(x, mask=mask)
    qg, ig, lg = grouped(x, mask=mask)
    assert len(backend.calls) == (2 if mask is not None else 0), "both took the fused route"
    assert q1.dtype == qg.dtype and q1.shape == qg.shape == x.shape and torch.equal(q1, qg)
    assert i1.shape == (*X_SHAPE[:2], Q) and ig.shape == (1, *X_SHAPE[:2], Q) and torch.equal(i1, ig[0])
    assert l1.shape == (1, Q) and lg.shape == (1, 1, Q) and l1.dtype == lg.dtype == torch.float32
    assert torch.equal(l1, lg.reshape(1, Q))
    assert bool((l1 > 0).all()) == training
    if training:  # one EMA step moved both the same way
        a, b = _ema_state(single), _ema_state(grouped)
        fresh = _ema_state(_build("rvq"))
        for attr in a:
            assert torch.equal(a[attr], b[attr]), attr
            assert not torch.equal(a[attr], fresh[attr]), attr + " did not move"


@pytest.mark.parametrize("training", [False, True])
def test_shared_codebook_stack_against_the_layer_loop(training, backend, monkeypatch):
    """One codebook for every stage (the single stack only: a grouped stack of shared stacks is the loop over the groups).
    In train mode the codebook is frozen: a shared codebook that moves is searched layer by layer in any case.
    The loop's loss is each layer's fp32 mean over 80 squares, the fused one an fp64 sum divided once: they agree to 80
    fp32 roundings, 80 * 2^-24 < 1e-5 relative."""
    import vector_quantization as vq

    x = _x()
    kwargs = dict(freeze_codebook=True) if training else {}
    fused = _build("rvq", training=training, shared_codebook=True)
    entered = []
    fused_forward = fused._forward_fused
    monkeypatch.setattr(fused, "_forward_fused", lambda *a, **k: (entered.append(1), fused_forward(*a, **k))[1])
    qf, idf, lf = fused(x, **kwargs)
    assert entered == [1]
    loop = _build("rvq", training=training, shared_codebook=True)
    monkeypatch.setattr(vq.ResidualVQ, "_fusable", lambda self, x, mask, drop_active: False)
    ql, idl, ll = loop(x, **kwargs)
    assert torch.equal(idf, idl) and len(torch.unique(idf)) > 1
    assert torch.equal(qf, ql)
    assert lf.shape == ll.shape == (1, Q) and lf.dtype == ll.dtype
    assert torch.allclose(lf, ll, rtol=1e-5, atol=0.0)
    if training:
        assert bool((lf > 0).all())
        for attr, t in _ema_state(fused).items():
            assert torch.equal(t, _ema_state(loop)[attr]), attr + ": frozen"


# -------------------------------------------------------------------------------------------------- backend call trace
def _describe(v):
    if isinstance(v, torch.Tensor):
        dtype = {torch.float32: "f32", torch.float64: "f64", torch.int64: "i64", torch.bool: "b8"}[v.dtype]
        return f"{dtype}{list(v.shape)}/{list(v.stride())}"
    return repr(v)


class Recorder:
    """Every backend call as one line: name(tensor arguments as dtype[shape]/[strides]; keywords in the order given)."""

    def __init__(self, inner):
        self._inner, self.lines = inner, []

    def __getattr__(self, name):
        target = getattr(self._inner, name)  # (AttributeError for what the inner backend lacks: hasattr() answers as it does)
        if not callable(target):
            return target

        def call(*args, **kwargs):
            shown = [_describe(a) for a in args] + [f"{k}={_describe(v)}" for k, v in kwargs.items()]
            self.lines.append(f"{name}({', '.join(shown)})")
            return target(*args, **kwargs)

        return call


def _trace(route):
    """One train-mode forward (commitment loss and EMA step included) of a fused route -> the recorder's lines."""
    from vector_quantization import search

    fwd = {}
    if route == "single":
        mod, x = _build("rvq", training=True), _x()
    elif route == "single_cut1":
        mod, x = _build("rvq", training=True, **DROP), _x()
        fwd = dict(rand_quantize_dropout_fixed_seed=CUT1_SEED)
    elif route == "grouped":
        mod, x = _build("grvq", groups=2, training=True), _x(2)
    else:
        mod, x = _build("grvq", groups=2, training=True), _x(2)
        fwd = dict(mask=_mask())
    rec = Recorder(RuleBackend)
    search.set_backend(rec)
    try:
        _q, idx, _losses = mod(x, **fwd)
    finally:
        search.set_backend(None)
    if route == "single_cut1":
        assert bool((idx[..., :2] >= 0).all()) and bool((idx[..., 2] == -1).all())
    return rec.lines


def _ema_update(stages):
    """A layer's EMA step: its own three buffers, then column q of the [1, stages, K] hits and [1, stages, K, D] sums."""
    return ("ema_update(f32[1, 16]/[16, 1], f32[1, 16, 8]/[128, 8, 1], f32[1, 16, 8]/[128, 8, 1], "
            f"f32[1, 16]/[{16 * stages}, 1], f32[1, 16, 8]/[{128 * stages}, 8, 1], decay=0.8, eps=1e-05, l2norm=False)")


_GROUPED_ROWS = "f32[2, 10, 8]/[8, 16, 1]"  # x [2, 5, 16] read in place: group stride d, row stride G * d
_GROUPED_CODES = "f32[2, 3, 16, 8]/[384, 128, 8, 1]"

TRACES = {
    "single": [
        "quantize(f32[1, 10, 8]/[80, 8, 1], f32[1, 3, 16, 8]/[384, 128, 8, 1], metric=0, ste=True, want_sq_err=True, "
        "share=False, out=None, idx=i64[1, 10, 3]/[30, 3, 1])",
        "ema_accumulate_residual(f32[1, 10, 8]/[80, 8, 1], f32[1, 3, 16, 8]/[384, 128, 8, 1], i64[1, 10, 3]/[30, 3, 1], "
        "ste=True, share=False)",
        *[_ema_update(3)] * 3,
    ],
    "single_cut1": [  # views of the first two codebooks and of the first two index columns
        "quantize(f32[1, 10, 8]/[80, 8, 1], f32[1, 2, 16, 8]/[384, 128, 8, 1], metric=0, ste=True, want_sq_err=True, "
        "share=False, out=None, idx=i64[1, 10, 2]/[30, 3, 1])",
        "ema_accumulate_residual(f32[1, 10, 8]/[80, 8, 1], f32[1, 2, 16, 8]/[384, 128, 8, 1], i64[1, 10, 2]/[30, 3, 1], "
        "ste=True, share=False)",
        *[_ema_update(2)] * 2,
    ],
    "grouped": [
        f"quantize({_GROUPED_ROWS}, {_GROUPED_CODES}, metric=0, ste=True, want_sq_err=True, share=False, "
        f"out={_GROUPED_ROWS}, idx=None, sq_err_per_head=True)",
        f"ema_accumulate_residual({_GROUPED_ROWS}, {_GROUPED_CODES}, i64[2, 10, 3]/[30, 3, 1], ste=True, share=False)",
        *[_ema_update(3)] * 6,
    ],
    "grouped_mask": [
        # the all-zero row's answers, once; then the search on every row, the mask pass, and the EMA step
        "quantize(f32[6, 1, 8]/[8, 8, 1], f32[6, 1, 16, 8]/[128, 128, 8, 1], metric=0, ste=False, want_sq_err=False, "
        "share=False)",
        f"quantize({_GROUPED_ROWS}, {_GROUPED_CODES}, metric=0, ste=True, want_sq_err=False, share=False, "
        f"out={_GROUPED_ROWS}, idx=None)",
        f"residual_mask({_GROUPED_ROWS}, {_GROUPED_CODES}, i64[2, 10, 3]/[30, 3, 1], b8[10]/[1], i64[2, 3]/[3, 1], train=True, "
        f"want_sq_err=True, per_group=True, out={_GROUPED_ROWS})",
        f"ema_accumulate_residual({_GROUPED_ROWS}, {_GROUPED_CODES}, i64[2, 10, 3]/[30, 3, 1], ste=True, share=False)",
        *[_ema_update(3)] * 6,
    ],
}


@pytest.mark.parametrize("route", list(TRACES))
def test_backend_calls_of_the_fused_routes(route):
    assert random.Random(CUT1_SEED).randrange(0, Q) == 1
    lines = _trace(route)
    assert lines == TRACES[route]
    search_call = next(line for line in lines if line.startswith("quantize(f32[") and ", 10, 8]/" in line.split(", f32")[0])
    if route.startswith("single"):  # no destination view, no per-group errors: G = 1 is not "grouped with one group"
        assert "out=None" in search_call and "sq_err_per_head" not in search_call
    elif route == "grouped":
        assert "out=f32[2, 10, 8]/[8, 16, 1]" in search_call and "sq_err_per_head=True" in search_call
    else:  # the search of a masked call reports no errors at all; the mask pass reports them per group
        assert "out=f32[2, 10, 8]/[8, 16, 1]" in search_call
        assert any(line.startswith("residual_mask(") and "per_group=True" in line for line in lines)


# ------------------------------------------------------------------------------------------------ `random` consumption
def _module(kind):
    import vector_quantization as vq

    if kind == "rvq":
        return _build("rvq", **DROP)
    if kind == "grvq":
        return _build("grvq", groups=2, **DROP)
    if kind == "rlfq":
        return vq.ResidualLFQ(dim=4, num_quantizers=Q, codebook_size=16, **DROP)
    if kind == "grlfq":
        return vq.GroupedResidualLFQ(dim=8, groups=2, num_quantizers=Q, codebook_size=16, **DROP)
    if kind == "rfsq":
        return vq.ResidualFSQ(dim=4, levels=[5, 5, 3, 3], num_quantizers=Q, **DROP)
    return vq.GroupedResidualFSQ(dim=8, groups=2, levels=[5, 5, 3, 3], num_quantizers=Q, **DROP)


def _random_after_forward(kind, training):
    """random.seed(7), one forward, -> (the state of `random`, its next random()).  The LFQ and FSQ stacks refuse CPU rows
    (native.NativeUnavailable) -- after their draws, which is all that is looked at."""
    from vector_quantization import native

    mod = _module(kind).train(training)
    x = _randn((2, 5, {"rvq": DIM, "grvq": 2 * DIM, "rlfq": 4, "rfsq": 4}.get(kind, 8)), 5)
    random.seed(7)
    if kind in ("rvq", "grvq"):
        mod(x)
    else:
        with pytest.raises(native.NativeUnavailable):
            mod(x)
    return random.getstate(), random.random()


def _state_after_draws(draws):
    random.seed(7)
    for draw in draws:
        draw()
    return random.getstate()


_CUT = lambda: random.randrange(0, Q)  # noqa: E731  a stack's own dropout draw
_SEED = lambda: random.randint(0, int(1e7))  # noqa: E731  a grouped module's seed for its stacks

# (kind, training) -> (what the forward draws from the process-wide generator, the next random.random() after it)
NEXT_RANDOM = {
    ("rvq", True): ([_CUT], 0.9478653606090632),
    ("grvq", True): ([_SEED], 0.9478653606090632),  # (the layer loop over the groups: every stack draws from Random(seed))
    ("rlfq", True): ([_CUT], 0.9478653606090632),
    ("grlfq", True): ([_SEED], 0.9478653606090632),
    ("rfsq", True): ([_CUT], 0.9478653606090632),
    ("grfsq", True): ([_SEED], 0.9478653606090632),
    ("grvq", False): ([], 0.32383276483316237),  # fused: the seed is drawn on the fallback path only
    ("grlfq", False): ([_SEED], 0.9478653606090632),  # drawn before the path is chosen, in eval too, as the reference does
    ("grfsq", False): ([_SEED], 0.9478653606090632),
}


@pytest.mark.parametrize("kind,training", list(NEXT_RANDOM), ids=[f"{k}-{'train' if t else 'eval'}" for k, t in NEXT_RANDOM])
def test_random_consumption(kind, training, backend):
    draws, want_next = NEXT_RANDOM[(kind, training)]
    state, got_next = _random_after_forward(kind, training)
    assert got_next == want_next
    assert state == _state_after_draws(draws)


# ------------------------------------------------------------------------------------------------- the shared helpers
def test_dropout_cut_takes_a_generator_a_seed_or_the_process_wide_one():
    from vector_quantization.residual_common import dropout_cut

    for cutoff, stages, multiple in ((0, 3, 1), (1, 8, 4), (0, 6, 2), (2, 5, 1)):
        for seed in range(10):
            want = random.Random(seed).randrange(cutoff, stages)
            want = -(-(want + 1) // multiple) * multiple - 1  # rounded up to a whole multiple of stages
            assert dropout_cut(cutoff, stages, multiple, seed) == want
            assert dropout_cut(cutoff, stages, multiple, random.Random(seed)) == want
            random.seed(seed)
            assert dropout_cut(cutoff, stages, multiple) == want
            assert random.random() == (random.seed(seed), random.randrange(cutoff, stages), random.random())[2]


def test_pad_stages_and_decode_buffers():
    from vector_quantization.residual_common import grouped_decode_dest, grouped_decode_rows, pad_stages

    idx32 = torch.arange(12, dtype=torch.int32).reshape(2, 3, 2)
    losses = torch.ones(2, 2, dtype=torch.float64)
    same_idx, same_losses = pad_stages(idx32, 2, losses)
    assert same_idx is idx32 and same_losses is losses  # nothing dropped: nothing copied, no promotion
    padded, padded_losses = pad_stages(idx32, 4, losses)
    assert padded.dtype == torch.int64 and padded.shape == (2, 3, 4)  # int64 nulls promote the stack, as torch.stack does
    assert torch.equal(padded[..., :2], idx32.long()) and bool((padded[..., 2:] == -1).all())
    assert padded_losses.dtype == torch.float64 and torch.equal(padded_losses, torch.tensor([[1.0, 1, 0, 0]] * 2, dtype=torch.float64))
    assert pad_stages(idx32, 4)[1] is None

    indices = torch.zeros((2, 3, 5, 4), dtype=torch.int64)  # [G, b, n, q]
    flat, lead = grouped_decode_rows(indices)
    assert flat.shape == (2, 15, 4) and tuple(lead) == (3, 5) and flat.data_ptr() == indices.data_ptr()
    out, dest = grouped_decode_dest(flat, lead, 6)
    assert out.shape == (3, 5, 12) and out.is_contiguous() and dest.shape == (2, 15, 6) and dest.stride() == (6, 12, 1)
    assert dest.data_ptr() == out.data_ptr()
    codes, dest = grouped_decode_dest(flat, lead, 6, stages=4)
    assert codes.shape == (2, 4, 3, 5, 6) and codes.is_contiguous() and dest.shape == (4, 2, 15, 6)
    assert dest.stride() == (90, 360, 6, 1) and dest.data_ptr() == codes.data_ptr()
