"""GPU: VALUE edges of the four cross-entropy producers -- vq_softmax_stats_f32 (the kAuxStats sweep), the search's
log-sum-exp variant (vq_quantize_lse_f32), vq_ce_backward_f32 (one-wave kernel, roles, roles512) and vq_ce_backward_live_f32.
Their shapes, strides and launch roles are covered elsewhere; here the inputs are non-finite, saturated, coincide with the
target code, or carry targets outside [0, K).

Shapes: M = 70 rows (three 32-row blocks, the last holds 6), K = 70 codes (three 32-code sub-tiles, a 6-code tail), every
padded dim (D = 24, 64, 100, 256, 320, 512 -> Dp = 32, 64, 128, 256, 512, 512), both metrics, H = 1 and one H = 2 case.

Reference, one for everything: the CPU oracle's fp32 similarities (bit-identical to vq_similarities_f32, NaN included:
test_similarities_keep_nan) and, on them in float64,
    ref_lse = m + log(sum(exp(s - m))),  m = the NaN-propagating row maximum  (NaN when the row holds a NaN or a +inf logit)
    ref_ce  = F.cross_entropy(s, target, ignore_index=-1, reduction="none")   (ATen: NaN for the same rows, +inf where the
                                                                               target's logit is -inf and ref_lse is finite)
Gradients: the float64 closed form of tests/test_gpu_ce_backward_live.py with the distances written out and subgradient 0
at distance 0.

Tolerances: log-sum-exp and target logit rtol 2e-6 / atol 2e-5 (the documented tolerance of
test_gpu_similarity_consumers.py); gradients atol 2e-5 * max|fp64 gradient|, rtol 2e-4 (the project's for
vq_ce_backward_f32).  The saturation test alone adds 4 * 2^-24 * max|lse| to rtol: the fp32 storage of lse, the product
lse * log2(e) and the fused multiply-add ahead of exp2 together bound the relative error of every softmax weight by that.
Under Euclid the sweep takes the hardware square root (1 ulp), the oracle the correctly rounded one, so a finite target logit
is compared within the tolerance; under dot it is the similarity bit for bit.  Every test prints its figures before it asserts.
"""
from __future__ import annotations

import contextlib
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import poison_rows, same_values  # noqa: E402

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
M = K = 70
DIMS = [24, 64, 100, 256, 320, 512]
COEF = 0.37
LSE_RTOL, LSE_ATOL = 2e-6, 2e-5
ATOL, RTOL = 2e-5, 2e-4
LIVE_MAX_DIM = 256


def _native():
    from vector_quantization import native

    native.load()
    return native


@contextlib.contextmanager
def _env(name):
    os.environ[name] = "1"
    try:
        yield
    finally:
        os.environ.pop(name, None)


# ------------------------------------------------------------------------------------------------ references
def _oracle_sims(oracle, x, cb, metric):
    with np.errstate(all="ignore"):
        return np.stack([oracle.similarities(np.ascontiguousarray(x[h].numpy()), np.ascontiguousarray(cb[h].numpy()), metric)
                         for h in range(x.shape[0])])


def _ref_lse(sims):
    s = sims.astype(np.float64)
    with np.errstate(all="ignore"):
        m = s.max(-1, keepdims=True)  # numpy's max propagates NaN
        return (m + np.log(np.exp(s - m).sum(-1, keepdims=True)))[..., 0]


def _ref_ce(sims, target):
    s = torch.from_numpy(sims).double()
    ce = F.cross_entropy(s.reshape(-1, s.shape[-1]), target.reshape(-1), ignore_index=-1, reduction="none")
    return ce.reshape(target.shape).numpy()


def _closed_form(x, c, live, target, metric, coef):
    """One head: x [R, D], c / live [K, D], target [R] (outside [0, K): ignored) -> float64 gradient [R, D]."""
    x, c, live = x.double(), c.double(), live.double()
    s = -((x[:, None, :] - c[None, :, :]) ** 2).sum(-1).sqrt() if metric == 0 else x @ c.T
    valid = (target >= 0) & (target < c.shape[0])
    onehot = torch.zeros_like(s)
    onehot[valid, target[valid]] = 1.0
    gs = coef * valid[:, None].double() * (torch.softmax(s, -1) - onehot)
    if metric == 1:
        return gs @ live
    r = torch.where(s == 0, torch.zeros_like(gs), gs / s)  # ATen's subgradient 0 at distance 0
    return x * r.sum(-1, keepdim=True) - r @ live


def _live_codebook(cb):
    return torch.randn(cb.shape, generator=torch.Generator().manual_seed(23))


class Case:
    def __init__(self, oracle, x, cb, target, metric, poisoned=None):
        self.x, self.cb, self.target, self.metric = x, cb, target, metric
        self.H, _, self.D = x.shape
        self.poisoned = np.zeros(target.shape, bool) if poisoned is None else poisoned
        self.sims = _oracle_sims(oracle, x, cb, metric)
        self.ref_lse = _ref_lse(self.sims)
        self.live = _live_codebook(cb)

    def finish(self):
        self.ref_ce = _ref_ce(self.sims, self.target)
        return self

    def device(self):
        return self.x.to(DEV), self.cb.to(DEV), self.target.to(DEV)


def _randn_case(H, D, metric, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((H, M, D), generator=g)
    cb = torch.randn((H, K, D), generator=g)
    target = torch.randint(0, K, (H, M), generator=g)
    return x, cb, target


@functools.lru_cache(maxsize=None)
def _poisoned_case(oracle, H, D, metric, kind):
    """Inputs and references of one (shape, metric, poison): computed once, shared, never modified."""
    x, cb, target = _randn_case(H, D, metric, 1000 * metric + 10 * D + H)
    target[:, ::7] = -1
    poisoned = np.zeros((H, M), bool)
    for h in range(H):
        if kind == "rows":
            poisoned[h, poison_rows(x[h], seed=D + h)] = True
        elif kind == "nancode":
            cb[h, K - 3, D // 2] = NAN
        else:
            cb[h, K // 3, D - 1] = INF
    case = Case(oracle, x, cb, target, metric, poisoned)
    if kind == "infcode":  # the ref_ce == +inf class: the target's logit is -inf, the row's log-sum-exp finite
        for h in range(H):
            q = np.flatnonzero(np.isneginf(case.sims[h, :, K // 3]) & np.isfinite(case.ref_lse[h]))
            target[h, q[::3]] = K // 3
    return case.finish()


def _check_classes(case, kind):
    """What the poisoned cases must contain, asserted before the GPU is touched."""
    sims, ref_lse, ref_ce = case.sims, case.ref_lse, case.ref_ce
    assert not np.isneginf(sims).all(-1).any(), "a row whose similarities are all -inf"
    assert not np.isinf(ref_lse).any(), "+-inf in the reference log-sum-exp"
    n_nan, n_fin = int(np.isnan(ref_lse).sum()), int(np.isfinite(ref_lse).sum())
    n_minf = int((np.isneginf(sims).any(-1) & np.isfinite(ref_lse)).sum())
    n_inf_ce = int(np.isposinf(ref_ce).sum())
    print(f"{kind}: {n_nan} NaN-lse rows, {n_fin} finite, {n_minf} finite with a -inf logit, {n_inf_ce} rows with ce == +inf")
    if kind == "rows":
        assert n_fin >= 10 and n_nan >= 10
    elif kind == "nancode":
        assert n_fin == 0
    else:
        assert n_minf >= 10 and n_inf_ce >= 3


def _check_lse(what, lse, ref_lse):
    nan_ref = np.isnan(ref_lse)
    nan_got = np.isnan(lse)
    print(f"{what}: NaN rows {int(nan_got.sum())} (reference {int(nan_ref.sum())})")
    assert np.array_equal(nan_got, nan_ref), \
        f"{what}: NaN mask differs on rows {np.argwhere(nan_got != nan_ref).tolist()[:8]}, got {lse[nan_got != nan_ref][:8]}"
    fin = ~nan_ref
    if fin.any():
        err = np.abs(lse[fin].astype(np.float64) - ref_lse[fin])
        bound = LSE_ATOL + LSE_RTOL * np.abs(ref_lse[fin])
        print(f"{what}: lse max error {err.max():.3e}, worst error / bound {(err / bound).max():.3f}")
        assert bool((err <= bound).all())


def _check_target_logit(what, tl, picked, metric):
    """tl against the oracle's similarity of the target, both 1-d fp32, no NaN in `picked`."""
    if metric == 1:
        assert same_values(tl, picked), f"{what}: the target logit is not the similarity bit for bit"
        return
    inf = np.isinf(picked)
    assert np.array_equal(np.isinf(tl), inf) and same_values(tl[inf], picked[inf]), f"{what}: infinite target logits differ"
    err = np.abs(tl[~inf].astype(np.float64) - picked[~inf])
    bound = LSE_ATOL + LSE_RTOL * np.abs(picked[~inf].astype(np.float64))
    if err.size:
        print(f"{what}: target logit max error {err.max():.3e}, worst error / bound {(err / bound).max():.3f}")
    assert bool((err <= bound).all())


def _check_stats(what, case, lse, tl):
    """The contract of softmax_stats on `case` (lse, tl: fp32 numpy [H, M])."""
    _check_lse(what, lse, case.ref_lse)
    t = case.target.numpy()
    valid = t >= 0
    assert bool((tl[~valid] == 0).all()), f"{what}: the target logit of an ignored row is not 0"
    with np.errstate(all="ignore"):
        ce = (lse - tl)[valid]
    ref = case.ref_ce[valid]
    assert np.array_equal(np.isnan(ce), np.isnan(ref)), \
        f"{what}: lse - tl is NaN on {int(np.isnan(ce).sum())} valid rows, the reference on {int(np.isnan(ref).sum())}"
    assert np.array_equal(np.isposinf(ce), np.isposinf(ref)), f"{what}: lse - tl is +inf on other rows than the reference"
    rest = np.isfinite(ref)
    if rest.any():
        err = np.abs(ce[rest].astype(np.float64) - ref[rest])
        bound = LSE_ATOL + LSE_RTOL * np.abs(ref[rest])
        print(f"{what}: lse - tl max error {err.max():.3e}, worst error / bound {(err / bound).max():.3f}")
        assert bool((err <= bound).all())
    picked = np.take_along_axis(case.sims, np.maximum(t, 0)[..., None], -1)[..., 0]
    sel = valid & ~np.isnan(picked)
    _check_target_logit(what, tl[sel], picked[sel], case.metric)


# ------------------------------------------------------------------------------------------------ (a), (b): the forward
POISON_CASES = [(1, D, kind) for D in DIMS for kind in ("rows", "nancode", "infcode")] + [(2, 100, "rows")]


@pytest.mark.parametrize("H,D,kind", POISON_CASES + [(1, 600, "rows")])
@pytest.mark.parametrize("metric", [0, 1])
def test_softmax_stats_of_poisoned_inputs(oracle, H, D, kind, metric):
    """vq_softmax_stats_f32 (D = 600: the chunked route over vq_similarities_f32): NaN exactly where ATen's cross entropy on
    the same similarities is NaN, +inf exactly where it is +inf, the tolerance elsewhere."""
    native = _native()
    case = _poisoned_case(oracle, H, D, metric, kind)
    _check_classes(case, kind)
    xd, cbd, td = case.device()
    lse, tl = native.softmax_stats(xd, cbd, metric=metric, target=td)
    torch.cuda.synchronize()
    _check_stats(f"softmax_stats D {D} metric {metric} {kind}", case, lse.cpu().numpy(), tl.cpu().numpy())


@pytest.mark.parametrize("H,D,kind", POISON_CASES)
@pytest.mark.parametrize("metric", [0, 1])
def test_search_log_sum_exp_of_poisoned_inputs(oracle, H, D, kind, metric):
    """vq_quantize_lse_f32 under the same contract, and its NaN rows are the NaN rows of vq_softmax_stats_f32: the commitment
    loss takes the one, `indices=` teacher forcing the other."""
    native = _native()
    case = _poisoned_case(oracle, H, D, metric, kind)
    _check_classes(case, kind)
    xd, cbd, _ = case.device()
    r = native.quantize(xd, cbd[:, None].contiguous(), metric=metric, want_lse=True, want_best=True)
    stats, _ = native.softmax_stats(xd, cbd, metric=metric)
    torch.cuda.synchronize()
    lse = r["lse"].cpu().numpy()
    _check_lse(f"search lse D {D} metric {metric} {kind}", lse, case.ref_lse)
    assert np.array_equal(np.isnan(lse), np.isnan(stats.cpu().numpy())), "the two producers disagree on which rows are NaN"


# ------------------------------------------------------------------------------------------------ the backward launches
def _backward_launches(native, case, lse, tl, td=None):
    """name -> (gradient [H, M, D] on the CPU, the codebook its contraction runs over): the default launch (roles at Dp = 256 /
    512, the one-wave kernel below), the one-wave kernel everywhere, and live codes (an independent codebook) where D allows."""
    xd, cbd, t0 = case.device()
    td = t0 if td is None else td
    coef = torch.tensor([COEF], device=DEV)
    out = {"default": (native.ce_backward(xd, cbd, lse, tl, td, coef, metric=case.metric), case.cb)}
    with _env("VQ_CE_NO_ROLES"):
        out["one-wave"] = (native.ce_backward(xd, cbd, lse, tl, td, coef, metric=case.metric), case.cb)
    if case.D <= LIVE_MAX_DIM:
        out["live"] = (native.ce_backward(xd, cbd, lse, tl, td, coef, metric=case.metric, live=case.live.to(DEV)), case.live)
    torch.cuda.synchronize()
    return {name: (g.cpu(), codes) for name, (g, codes) in out.items()}


def _want(case, codes, rows=None, target=None):
    """float64 closed form on the boolean row mask `rows` [H, M] (default: all rows) -> list over heads of [R_h, D]."""
    target = case.target if target is None else target
    rows = np.ones(target.shape, bool) if rows is None else rows
    return [_closed_form(case.x[h][rows[h]], case.cb[h], codes[h], target[h][rows[h]], case.metric, COEF) for h in range(case.H)]


def _assert_grad(what, got, want, scale, extra_rtol=0.0):
    got, want = got.double(), want.double()
    err = (got - want).abs()
    bound = ATOL * scale + (RTOL + extra_rtol) * want.abs()
    print(f"{what}: max error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}, scale {scale:.3e}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("H,D,kind", [c for c in POISON_CASES if c[2] != "infcode"])
@pytest.mark.parametrize("metric", [0, 1])
def test_backward_keeps_poison_in_its_rows(oracle, H, D, kind, metric):
    """Poisoned rows: every clean row keeps its gradient (an ignored one exactly 0) although it shares a 32-row block, its
    codebook tiles and the finalize staging with rows full of NaN / inf; a poisoned row (NaN cross entropy) never comes out
    finite.  A NaN code reaches every row."""
    native = _native()
    case = _poisoned_case(oracle, H, D, metric, kind)
    _check_classes(case, kind)
    xd, cbd, td = case.device()
    lse, tl = native.softmax_stats(xd, cbd, metric=metric, target=td)
    valid = case.target.numpy() >= 0
    clean = ~case.poisoned
    for name, (got, codes) in _backward_launches(native, case, lse, tl).items():
        what = f"backward D {D} metric {metric} {kind} {name}"
        bad = ~torch.isfinite(got).all(-1).numpy()  # rows [H, M] with a non-finite entry
        if kind == "nancode":
            print(f"{what}: {int(bad[valid].sum())} of {int(valid.sum())} non-ignored rows hold a non-finite entry")
            assert bool(bad[valid].all()), f"{what}: finite gradient rows {np.argwhere(valid & ~bad).tolist()[:8]}"
            continue
        want = _want(case, codes, clean)
        scale = max(float(w.abs().max()) for w in want)
        for h in range(H):
            _assert_grad(f"{what} head {h}, clean rows", got[h][clean[h]], want[h], scale)
            zero = clean[h] & ~valid[h]
            assert zero.any() and int(torch.count_nonzero(got[h][zero])) == 0, f"{what}: a clean ignored row is not exactly 0"
        must = case.poisoned & valid & np.isnan(case.ref_ce)
        print(f"{what}: {int(bad[must].sum())} of {int(must.sum())} poisoned non-ignored rows hold a non-finite entry")
        assert must.any() and bool(bad[must].all()), f"{what}: poison became a finite gradient on rows {np.argwhere(must & ~bad).tolist()}"


# ------------------------------------------------------------------------------------------------ (d) saturation
@functools.lru_cache(maxsize=None)
def _saturated_case(oracle, D, metric):
    """Even rows saturated (largest softmax weight > 1 - 1e-6), odd rows far from it (< 0.9).  Dot: the rows scaled so that
    the logits have a standard deviation of 200 / of 0.5.  Euclid: scaling rows or codes cannot do both (with large codes the
    norms of the codes alone separate the logits of EVERY row, with small ones no row is separated), so the codes are scaled by
    3 and an even row is 0.8 of a code -- 0.6 sqrt(D) from it and about 3.2 sqrt(D) from the others, far from the tiny
    distances whose expanded form cancels in fp32."""
    x, cb, target = _randn_case(1, D, metric, 77 + D + metric)
    pick = torch.randint(0, K, (M,), generator=torch.Generator().manual_seed(D))
    if metric == 1:
        x[:, 0::2] *= 200.0 / D ** 0.5
        x[:, 1::2] *= 0.5 / D ** 0.5
    else:
        cb *= 3.0
        x[0, 0::2] = 0.8 * cb[0, pick[0::2]]
    xd, cd = x[0].double(), cb[0].double()
    s = -((xd[:, None, :] - cd[None, :, :]) ** 2).sum(-1).sqrt() if metric == 0 else xd @ cd.T
    pmax, amax = torch.softmax(s, -1).max(-1)
    rows = torch.arange(M)
    target[0, 0::4] = amax[0::4]                                          # saturated, the target is the arg-max
    target[0, 2::4] = (amax[2::4] + 1 + rows[2::4] % (K - 1)) % K         # saturated, another code
    target[0, 5::10] = -1
    case = Case(oracle, x, cb, target, metric).finish()
    case.pmax = pmax.numpy()
    return case


@pytest.mark.parametrize("D", [64, 256, 512])
@pytest.mark.parametrize("metric", [0, 1])
def test_saturated_softmax(oracle, D, metric):
    """One-hot softmax rows: the backward's split into a softmax part (the sweep) and a one-hot part (the finalize) cancels
    when the target is the arg-max, and leaves a full-size gradient when it is another code."""
    native = _native()
    case = _saturated_case(oracle, D, metric)
    n_sat, n_soft = int((case.pmax > 1 - 1e-6).sum()), int((case.pmax < 0.9).sum())
    print(f"D {D} metric {metric}: {n_sat} rows above 1 - 1e-6, {n_soft} rows below 0.9, max |lse| {np.abs(case.ref_lse).max():.1f}")
    assert 4 * n_sat >= M and 4 * n_soft >= M
    t = case.target[0]
    sat = torch.from_numpy(case.pmax > 1 - 1e-6)
    amax = torch.from_numpy(case.sims[0].argmax(-1))
    assert int((sat & (t == amax)).sum()) >= 5 and int((sat & (t >= 0) & (t != amax)).sum()) >= 5
    xd, cbd, td = case.device()
    lse, tl = native.softmax_stats(xd, cbd, metric=metric, target=td)
    torch.cuda.synchronize()
    _check_stats(f"saturated D {D} metric {metric}", case, lse.cpu().numpy(), tl.cpu().numpy())
    extra = 4.0 * 2.0 ** -24 * float(np.abs(case.ref_lse).max())
    for name, (got, codes) in _backward_launches(native, case, lse, tl).items():
        (want,) = _want(case, codes)
        assert bool(torch.isfinite(got).all())
        _assert_grad(f"saturated D {D} metric {metric} {name}", got[0], want, float(want.abs().max()), extra_rtol=extra)
        assert int(torch.count_nonzero(got[0][t < 0])) == 0


# ------------------------------------------------------------------------------------------------ (e) zero distance on the target
@functools.lru_cache(maxsize=None)
def _coinciding_case(oracle, D):
    x, cb, target = _randn_case(1, D, 0, 300 + D)
    target[:, 4::5] = -1
    x[0, 3] = cb[0, K // 2]
    target[0, 3] = K // 2
    return Case(oracle, x, cb, target, 0).finish()


@pytest.mark.parametrize("D", [64, 256, 320])
def test_row_on_its_target_code(oracle, D):
    """Euclid, a row that IS its target code: the target logit is 0, so the finalize's factor coef / logit is replaced by 0 and the
    sweep drops the code's infinite ratio -- ATen's subgradient 0 at distance 0, a finite row."""
    native = _native()
    case = _coinciding_case(oracle, D)
    assert case.sims[0, 3, K // 2] == 0.0, "the fp32 chain must give this pair distance 0"
    xd, cbd, td = case.device()
    lse, tl = native.softmax_stats(xd, cbd, metric=0, target=td)
    torch.cuda.synchronize()
    assert float(tl[0, 3]) == 0.0
    _check_stats(f"coinciding D {D}", case, lse.cpu().numpy(), tl.cpu().numpy())
    for name, (got, codes) in _backward_launches(native, case, lse, tl).items():
        (want,) = _want(case, codes)
        assert bool(torch.isfinite(got[0, 3]).all()), f"{name}: the coinciding row is not finite"
        _assert_grad(f"coinciding D {D} {name}", got[0], want, float(want.abs().max()))
        print(f"coinciding D {D} {name}: row 3 max error {float((got[0, 3].double() - want[3]).abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------ (f) target range
TARGETS = [K - 1, K, K + 5, 2 ** 32 + 3, -1, -7, -2 ** 63]


@pytest.mark.parametrize("D", [64, 320])
@pytest.mark.parametrize("metric", [0, 1])
def test_target_range(oracle, D, metric):
    """The native contract: a target is compared with 0 and K as the 64-bit value it is.  target >= K: logit -inf (stats), row
    ignored (backward) -- 2**32 + 3 is not code 3; target < 0, whatever its value: logit 0, row ignored."""
    native = _native()
    x, cb, _ = _randn_case(1, D, metric, 500 + D + metric)
    target = torch.tensor([TARGETS[r % len(TARGETS)] for r in range(M)], dtype=torch.int64)[None]
    case = Case(oracle, x, cb, target, metric)
    xd, cbd, td = case.device()
    lse0, none = native.softmax_stats(xd, cbd, metric=metric)
    lse, tl = native.softmax_stats(xd, cbd, metric=metric, target=td)
    torch.cuda.synchronize()
    assert none is None and torch.equal(lse.view(torch.int32), lse0.view(torch.int32)), "the target changed the log-sum-exp"
    _check_lse(f"target range D {D} metric {metric}", lse.cpu().numpy(), case.ref_lse)
    t, tln = target[0].numpy(), tl[0].cpu().numpy()
    assert bool(np.isneginf(tln[t >= K]).all()), f"a target >= K has the logit {tln[t >= K]}"
    assert bool((tln[t < 0] == 0).all())
    last = t == K - 1
    _check_target_logit(f"target K - 1, D {D} metric {metric}", tln[last], case.sims[0, last, K - 1], metric)
    for name, (got, codes) in _backward_launches(native, case, lse, tl).items():
        out = torch.from_numpy((t < 0) | (t >= K))
        assert int(torch.count_nonzero(got[0][out])) == 0, f"{name}: a row with a target outside [0, K) has a gradient"
        (want,) = _want(case, codes)
        _assert_grad(f"target range D {D} metric {metric} {name}", got[0], want, float(want.abs().max()))
