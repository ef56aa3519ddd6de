"""The LFQ entropy kernels and the residual-LFQ kernels at every codebook_dim d = 1 .. 20, against the fp64 restatements
(tests/lfq_dense.py, tests/rlfq_dense.py, run on the GPU in fp64) and against their own single-stage / chained forms.

Tolerance of a gradient (see _check): |got - want| <= 1e-4 |want| + a * max|want| per element, max|want| taken per case,
a = 2e-5 up to d = 16 and 2e-5 sqrt(2^d / 2^16) above.  Why the second term grows with d: the entropy backward sums
2^d / 64 products per lane in fp32, sequentially; the rounding of such a sum is a random walk of about
sqrt(n) * 2^-24 * sum|terms|, and the kernel centres the weights g_k at an estimate of sum_k g_k p_k before the sweep
(lfq_entropy_bwd_kernel), which keeps sum|terms| a small multiple of max|want| even where g_k is nearly constant.
Where the gradient is itself a near-cancellation (per-sample against codebook entropy, or a spread-out per-sample term),
max|want| is replaced by the size of the centred terms, computed in fp64 (_spread, or the two terms' own gradients).  2e-5 covers n = 1024 (d = 16) with a margin of ~5; the bound is scaled by sqrt(n / 1024) beyond.  There is no
absolute floor: entropy gradients scale as 1 / rows, so any fixed floor would swallow them."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfq_dense import EPS, dense_entropy, dense_entropy_weighted
from rlfq_dense import restate, stage_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = list(range(1, 21))


def _spread(v, rows, a, tau, w_ps, w_cb, chunk_elems=1 << 24):
    """4 tau a max over tasks of sum_k p_k |g_k - sum_j p_j g_j| in fp64: the size of the centred terms the backward's fp32
    sums carry (g_k = w_ps G(p_k) + w_cb[c, k]).  Where the result is much smaller than that (terms that nearly cancel in
    the gradient itself), the rounding of the sums is measured against it instead of against max|want|."""
    from lfq_dense import code_signs

    N, C, d = v.shape
    vs = v.detach().double()[rows] if rows is not None else v.detach().double()
    codes = code_signs(d, v.device) * a
    wc = w_cb.detach().double().reshape(C, 1 << d)
    out = 0.0
    step = max(1, chunk_elems // (C << d))
    for r0 in range(0, vs.shape[0], step):
        p = torch.softmax(2.0 * tau * torch.einsum("rcd,pd->rcp", vs[r0:r0 + step], codes), dim=-1)
        G = torch.where(p >= EPS, -(p.clamp(min=1e-300).log() + 1.0), torch.full_like(p, -math.log(EPS)))
        g = float(w_ps) * G + wc
        mean = (g * p).sum(-1, keepdim=True)
        out = max(out, float(((g - mean).abs() * p).sum(-1).max()))
    return 4.0 * tau * a * out


def _check(got, want, d, what="", spread=0.0):
    got = got.double()
    want = want.double().to(got.device)
    scale = max(float(want.abs().max()), spread)
    a = 2e-5 * max(1.0, math.sqrt(2.0 ** (d - 16)))
    err = (got - want).abs()
    bound = 1e-4 * want.abs() + a * scale
    assert bool(torch.isfinite(got).all()), what
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).reshape(-1)))
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of tolerance; worst got {float(got.reshape(-1)[i]):.6e} "
                             f"want {float(want.reshape(-1)[i]):.6e}; max err / max|want| = {float(err.max()) / scale:.3e}")


def _rows_for(d, cap=301):
    """Rows of a case, sized by rows * 2^d (the fp64 restatement's work)."""
    return max(7, min(cap, (1 << 22) >> d))


def _layout(d, C, strided, subset, gen, scale=0.5):
    """v [N, C, d] (a strided view when asked: row stride > C * d), rows (sorted subset or None)."""
    N = _rows_for(d)
    N += (4 - (N * C) % 4) % 4 + 1  # R * C not a multiple of the waves per block
    if strided:
        base = torch.randn(N, C * d + 5, device=DEV, generator=gen) * scale
        v = base[:, 3:3 + C * d].reshape(N, C, d)
        assert v.stride(0) == C * d + 5
    else:
        v = torch.randn(N, C, d, device=DEV, generator=gen) * scale
    rows = None
    if subset:
        rows = torch.randperm(N, device=DEV, generator=gen)[: N - N // 5].sort().values
    return v, rows


_LAYOUTS = {"C3_strided_subset": (3, True, True), "C1_all_rows": (1, False, False)}
_TERMS = ["per_sample", "codebook_random", "codebook_near_uniform", "per_sample_small", "saturated_tau100"]
@pytest.mark.parametrize("layout", list(_LAYOUTS))
@pytest.mark.parametrize("term", _TERMS)
@pytest.mark.parametrize("d", DIMS)
def test_entropy_backward_isolated_terms(d, term, layout):
    from vector_quantization import native

    C, strided, subset = _LAYOUTS[layout]
    gen = torch.Generator(device=DEV).manual_seed(1000 * d + 17 * _TERMS.index(term) + C)
    v, rows = _layout(d, C, strided, subset, gen, scale=1e-3 if term == "per_sample_small" else 0.5)
    N = v.shape[0]
    R = N if rows is None else int(rows.numel())
    P = 1 << d
    tau, a = 1.0, 1.0
    w_ps, w_cb = 0.0, torch.zeros(C, P, device=DEV)
    if term in ("per_sample", "per_sample_small"):
        w_ps = 1.0 / (R * C)
    elif term == "codebook_random":
        w_cb = torch.randn(C, P, device=DEV, generator=gen) / (R * C)
    elif term == "codebook_near_uniform":  # the codebook term once avg_prob is near uniform: G(avg) nearly constant
        w_cb = (9.0 + 1e-3 * torch.randn(C, P, device=DEV, generator=gen)) / (R * C)
    else:
        tau = 100.0
        v[::3] *= 1e3
        v[1::7] = 0.0
        w_ps = 0.7 / (R * C)
        w_cb = torch.randn(C, P, device=DEV, generator=gen) / (R * C)
    got = native.lfq_entropy_backward(v, rows, a, tau, torch.tensor(w_ps, device=DEV), w_cb)
    want = dense_entropy_weighted(v, rows, a, tau, w_ps, w_cb)
    if rows is not None:
        unsel = torch.ones(N, dtype=torch.bool, device=DEV)
        unsel[rows] = False
        assert bool((got[unsel] == 0).all())
    if term == "per_sample_small":
        # every code below the 1e-5 clamp (d >= 17 here): the clamped entropy is constant, the exact gradient zero, and
        # the kernel's centred G is exactly zero for every code
        z = (4.0 * tau * a * v.double()).abs()
        lmax = (-torch.log1p(torch.exp(-z))).sum(-1)
        if bool((lmax < math.log(EPS) - 1e-3).all()):
            assert bool((got == 0).all())
            return
    _check(got, want, d, f"d={d} {term} {layout}", _spread(v, rows, a, tau, w_ps, w_cb))


@pytest.mark.parametrize("layout", list(_LAYOUTS))
@pytest.mark.parametrize("d", DIMS)
def test_entropy_forward(d, layout):
    from vector_quantization import native

    C, strided, subset = _LAYOUTS[layout]
    gen = torch.Generator(device=DEV).manual_seed(2000 + d + C)
    v, rows = _layout(d, C, strided, subset, gen)
    ps, avg = native.lfq_entropy_forward(v, rows, 1.0, 1.0)
    ref = dense_entropy(v, rows, 1.0, 1.0)
    R = v.shape[0] if rows is None else int(rows.numel())
    # each task's entropy is an fp32 sum of 2^d / 64 same-signed terms per lane: a random walk of sqrt(n) * 2^-24 relative,
    # so rtol 1e-5 up to n = 1024 (d = 16) and scaled by sqrt(n / 1024) beyond, as the backward's bound (module docstring)
    rtol_ps = 1e-5 * max(1.0, math.sqrt(2.0 ** (d - 16)))
    np.testing.assert_allclose(float(ps) / (R * C), float(ref["per_sample"]), rtol=rtol_ps)
    np.testing.assert_allclose(avg.double().cpu().numpy(), ref["avg_prob"].cpu().numpy(), rtol=1e-5, atol=1e-30)


@pytest.mark.parametrize("R", [40001, 65537])
@pytest.mark.parametrize("d", [3, 6, 8])
def test_entropy_forward_many_splits(d, R):
    """Row counts giving the most splits of the codebook-term sum (lfq_rows_per_split) and a ragged last split."""
    from vector_quantization import native

    gen = torch.Generator(device=DEV).manual_seed(3000 + d + R)
    v = torch.randn(R, 1, d, device=DEV, generator=gen) * 0.6
    ps, avg = native.lfq_entropy_forward(v, None, 1.0, 1.0)
    ref = dense_entropy(v, None, 1.0, 1.0)
    np.testing.assert_allclose(float(ps) / R, float(ref["per_sample"]), rtol=1e-5)
    np.testing.assert_allclose(avg.double().cpu().numpy(), ref["avg_prob"].cpu().numpy(), rtol=1e-5)
    rows = torch.arange(0, R, 2, device=DEV)
    ps, avg = native.lfq_entropy_forward(v, rows, 1.0, 1.0)
    ref = dense_entropy(v, rows, 1.0, 1.0)
    np.testing.assert_allclose(avg.double().cpu().numpy(), ref["avg_prob"].cpu().numpy(), rtol=1e-5)


@pytest.mark.parametrize("term", ["batch_entropy", "per_sample_entropy"])
def test_module_near_uniform_avg_prob_65536_rows(term):
    """LFQ(codebook_size=2^12) on 65 536 rows at inv_temperature 1: avg_prob is close to uniform, so the codebook term's
    weights are nearly constant.  Each loss term back-propagated alone against fp64."""
    from vector_quantization import LFQ

    mod = LFQ(codebook_size=2**12).to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(41)
    x = (torch.randn(16, 4096, 12, device=DEV, generator=gen) * 0.3).requires_grad_(True)
    (out, idx, aux), bd = mod(x, inv_temperature=1.0, return_loss_breakdown=True)
    getattr(bd, term).backward()
    g_ps, g_cb = (0.0, 1.0) if term == "batch_entropy" else (1.0, 0.0)
    ref = dense_entropy(x.detach().reshape(-1, 1, 12), None, mod._code_mag, 1.0, g_ps=g_ps, g_cb=g_cb)
    avg = ref["avg_prob"]
    assert float((avg * 4096 - 1).abs().max()) < 0.1  # the near-uniform regime
    R = x.shape[0] * x.shape[1]
    w_cb = torch.zeros(1, 4096, device=DEV, dtype=torch.float64)
    if term == "batch_entropy":
        w_cb = -(avg.clamp(min=EPS).log() + (avg >= EPS).to(avg.dtype)) / R
    spread = _spread(x.detach().reshape(-1, 1, 12), None, mod._code_mag, 1.0, g_ps / R, w_cb)
    _check(x.grad.reshape(-1, 1, 12), ref["grad"], 12, term, spread)


@pytest.mark.parametrize("d", DIMS)
def test_staged_entropy_bitwise_every_dim(d):
    """Stage t of a staged call is bitwise a single-stage call on stage t's inputs: up to 32 stages, per-stage row lists,
    a shared row list and all rows; the code scale rotates with period 5."""
    from vector_quantization import native

    gen = torch.Generator(device=DEV).manual_seed(4000 + d)
    T = 32 if d <= 12 else (6 if d <= 16 else 3)
    N = max(37, min(1001, (1 << 23) >> d))
    R = N - 5 - d % 7
    v = torch.randn(T, N, d, device=DEV, generator=gen) * 0.4
    per_stage = torch.stack([torch.randperm(N, device=DEV, generator=gen)[:R].sort().values for _ in range(T)])
    scales = [1.0, 0.5, 0.25, 0.125, 0.0625]
    tau = 1.0 if d >= 17 else 100.0
    for rr in (per_stage, per_stage[0], None):
        RR = N if rr is None else rr.shape[-1]
        ps, avg = native.lfq_entropy_staged_forward(v, rr, scales, tau)
        w_ps = torch.rand(T, device=DEV, generator=gen)
        w_cb = (5.0 + torch.randn(T, 1 << d, device=DEV, generator=gen)) / RR
        gv = native.lfq_entropy_staged_backward(v, rr, scales, tau, w_ps, w_cb)
        for t in range(T):
            rt = None if rr is None else (rr[t] if rr.dim() == 2 else rr)
            p1, a1 = native.lfq_entropy_forward(v[t].unsqueeze(1), rt, scales[t % 5], tau)
            assert torch.equal(ps[t], p1) and torch.equal(avg[t], a1[0]), t
            g1 = native.lfq_entropy_backward(v[t].unsqueeze(1), rt, scales[t % 5], tau, w_ps[t], w_cb[t:t + 1])
            assert torch.equal(gv[t], g1[:, 0]), t


# ------------------------------------------------------------------------------------------------
# residual LFQ
# ------------------------------------------------------------------------------------------------
def _rlfq_rows(d):
    return max(300, min(3001, (1 << 24) >> d))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("S", [1, 5, 32])
@pytest.mark.parametrize("d", DIMS)
def test_rlfq_quantize_bitwise_equals_chained_lfq_calls(d, S, masked):
    """No clamp, no l2norm: out, idx, v_all and the commitment sums bitwise the chained single-stage lfq_quantize calls."""
    from vector_quantization import native

    gen = torch.Generator(device=DEV).manual_seed(5000 + 40 * d + S)
    N = _rlfq_rows(d) + 77
    x = torch.randn(N, d, device=DEV, generator=gen)
    mask = (torch.rand(N, device=DEV, generator=gen) > 0.25) if masked else None
    qmag = [2.0**-s for s in range(S)]
    out, idx, v_all, commit = native.rlfq_quantize(x[None], qmag, [None] * S, qmag, mask=mask, want_v=True, want_commit=True)
    r, acc = x, torch.zeros_like(x)
    for s in range(S):
        v = r.reshape(N, 1, d)
        _, o, i, c = native.lfq_quantize(v, qmag[s], xa=v, mask=mask, want_commit=True)
        assert torch.equal(v_all[0, s], r), s
        assert torch.equal(idx[0, :, s], i[:, 0]), s
        assert torch.equal(commit[0, s], c), s
        o = o.reshape(N, d)
        r = r - o
        acc = acc + o
    assert torch.equal(out[0], acc)


def _torch_chain(x, S, clamp0, spherical, d):
    """The fp32 torch chain of the residual stages (the stage-by-stage path's arithmetic): (out, idx [N, S], v per stage)."""
    r, acc, idx = x, torch.zeros_like(x), []
    bits = 2 ** torch.arange(d - 1, -1, -1, device=x.device)
    vs = []
    for s in range(S):
        scale = 2.0**-s
        u = r
        if clamp0 is not None:
            c = clamp0 * 0.5**s
            u = (u / c).tanh() * c
        v = F.normalize(u, dim=-1) * scale if spherical else u
        mag = scale
        if spherical:
            mag = float(F.normalize(torch.full((1, d), scale, dtype=torch.float32), dim=-1)[0, 0] * scale)
        q = torch.where(v > 0, mag, -mag)
        o = v + (q - v)
        idx.append(((v > 0).long() * bits).sum(-1))
        vs.append(v)
        r = r - o
        acc = acc + o
    return acc, torch.stack(idx, -1), vs


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("S", [1, 5, 32])
@pytest.mark.parametrize("variant", ["clamp", "spherical"])
@pytest.mark.parametrize("d", DIMS)
def test_rlfq_quantize_clamp_spherical_against_torch_chain(d, variant, S, masked):
    """Clamp (tanh) or l2norm: the kernel's libm and the torch chain's round apart by an ulp, so out agrees to rtol 1e-6
    and the indices agree exactly wherever the torch chain's stage input is clear of zero by more than that drift (every
    index of the first 16 stages; the deep stages of S = 32 reach the ulp scale of the input)."""
    from vector_quantization import native

    gen = torch.Generator(device=DEV).manual_seed(6000 + 40 * d + S)
    N = _rlfq_rows(d) + 13
    x = torch.randn(N, d, device=DEV, generator=gen)
    mask = (torch.rand(N, device=DEV, generator=gen) > 0.25) if masked else None
    clamp0 = 2.0 if variant == "clamp" else None
    sph = variant == "spherical"
    qmag = []
    for s in range(S):
        scale = 2.0**-s
        qmag.append(float(F.normalize(torch.full((1, d), scale, dtype=torch.float32), dim=-1)[0, 0] * scale) if sph else scale)
    clamp = [None if clamp0 is None else clamp0 * 0.5**s for s in range(S)]
    scale = [2.0**-s for s in range(S)]
    out, idx, v_all, commit = native.rlfq_quantize(x[None], qmag, clamp, scale, spherical=sph, mask=mask, want_v=True,
                                                   want_commit=True)
    want_out, want_idx, vs = _torch_chain(x, S, clamp0, sph, d)
    torch.testing.assert_close(out[0], want_out, rtol=1e-6, atol=1e-7)
    for s in range(min(S, 16)):  # deeper, the residual nears the fp32 ulp of the input and the two chains' drift
        clear = (vs[s].abs() > 1e-4 * 2.0**-s).all(-1)  # rows whose every dim is far from the sign step
        assert torch.equal(idx[0, clear, s], want_idx[clear, s]), s
        if s < 4:
            assert float(clear.float().mean()) > 0.5


_RLFQ_VARIANTS = {
    "plain": dict(),
    "clamp": dict(soft_clamp_input_value=2.0),
    "spherical": dict(spherical=True),
    "spherical_zero_rows": dict(spherical=True),
}
_RLFQ_TERMS = {  # (entropy_loss_weight, commitment_loss_weight, upstream gradient of out, of the losses)
    "g_out": (0.1, 0.25, True, 0.0),
    "commitment": (0.0, 0.25, False, 1.0),
    "entropy": (0.1, 0.0, False, 1.0),
}


@pytest.mark.parametrize("term", list(_RLFQ_TERMS))
@pytest.mark.parametrize("variant", list(_RLFQ_VARIANTS))
@pytest.mark.parametrize("d", DIMS)
def test_rlfq_backward_against_restatement(d, variant, term):
    """The fused ResidualLFQ training step (rlfq_quantize, the staged entropy kernels, rlfq_backward) against
    rlfq_dense.restate in fp64 on the GPU, one gradient source at a time.  At d = 1 an l2-normalised row is +-scale
    whatever its value, so the exact gradient through the norm is zero (the fp64 restatement leaves ~1e-14 of rounding)."""
    from vector_quantization import ResidualLFQ

    ew, cw, with_gout, g_loss = _RLFQ_TERMS[term]
    kw = dict(_RLFQ_VARIANTS[variant], entropy_loss_weight=ew, commitment_loss_weight=cw)
    S = 3
    torch.manual_seed(7)
    mod = ResidualLFQ(dim=d, num_quantizers=S, codebook_size=2**d, **kw).to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(7000 + d)
    N = max(9, min(403, (1 << 21) >> d))
    x0 = torch.randn(1, N, d, device=DEV, generator=gen) * 0.7
    if variant == "spherical_zero_rows":
        x0[0, ::5] = 0.0  # den = 1e-12: the Jacobian is scale / 1e-12 * I, as F.normalize's
    g_out = torch.randn(1, N, d, device=DEV, generator=gen) if with_gout else torch.zeros(1, N, d, device=DEV)
    x = x0.clone().requires_grad_(True)
    out, idx, losses = mod(x)
    (losses.sum() * g_loss + (out * g_out).sum()).backward()
    kwargs = dict(kw, codebook_size=2**d)
    rows = stage_rows(N, None, 1.0, S)
    ref = restate(kwargs, {}, x0, None, g_out, S, rows, g_loss=g_loss)
    assert ref["grad"].device == x.grad.device
    ps_only = None

    def spread(sel=slice(None)):
        if ps_only is None:
            return 0.0
        return max(float(ps_only[0, sel].abs().max()), float((ref["grad"] - ps_only)[0, sel].abs().max()))

    if term == "entropy":
        # the loss is per-sample minus codebook entropy: the two gradients nearly cancel when every row has a code of its
        # own, while each is computed from fp32 inputs (the stage inputs, avg_prob): measure against the larger of them
        ps_only = restate(dict(kwargs, diversity_gamma=0.0), {}, x0, None, g_out, S, rows, g_loss=g_loss)["grad"]
    if d == 1 and variant.startswith("spherical"):
        nz = x0[0, :, 0] != 0
        assert bool((x.grad[0, nz] == 0).all()) and float(ref["grad"][0, nz].abs().max()) < 1e-9
        if variant == "spherical":
            return
    if variant == "spherical_zero_rows":
        zero = torch.zeros(N, dtype=torch.bool, device=DEV)
        zero[::5] = True
        if d == 1:
            _check(x.grad[0, zero], ref["grad"][0, zero], d, "zero rows")
            return
        # the zero rows' gradient is ~1e12 times the others': check the two populations each on its own scale
        _check(x.grad[0, zero], ref["grad"][0, zero], d, "zero rows", spread(zero))
        _check(x.grad[0, ~zero], ref["grad"][0, ~zero], d, "other rows", spread(~zero))
        return
    _check(x.grad, ref["grad"], d, f"d={d} {variant} {term}", spread())


def test_chunked_staged_calls_bitwise_equal_unchunked(monkeypatch):
    """G = 2 groups x S = 5 stages whose staged entropy calls split into chunks of 3 stages (one chunk crosses the group
    boundary, the code scale rotates as scales[(t0 + j) % S]): forward and backward bitwise the unchunked call."""
    from vector_quantization import GroupedResidualLFQ, native, residual_lfq

    d, N = 10, 2000
    torch.manual_seed(3)
    mod = GroupedResidualLFQ(dim=2 * d, groups=2, num_quantizers=5, codebook_size=2**d, frac_per_sample_entropy=0.6,
                             soft_clamp_input_value=3.0).to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(4)
    x0 = torch.randn(2, N // 2, 2 * d, device=DEV, generator=gen)
    w = torch.randn(2, N // 2, 2 * d, device=DEV, generator=gen)

    calls = []
    orig = native.lfq_entropy_staged_forward

    def counting(v, *a, **k):
        calls.append(v.shape[0])
        return orig(v, *a, **k)

    def step():
        x = x0.clone().requires_grad_(True)
        torch.manual_seed(11)
        out, idx, losses = mod(x)
        lw = torch.linspace(0.5, 1.5, losses.numel(), device=DEV).reshape(losses.shape)
        ((losses * lw).sum() + (out * w).sum()).backward()
        return out.detach(), idx, losses.detach(), x.grad

    monkeypatch.setattr(native, "lfq_entropy_staged_forward", counting)
    whole = step()
    assert calls == [10]
    R = int(N * 0.6)  # entropy rows per stage: frac_per_sample_entropy of the 2 x 1000 tokens
    per_stage = int(native.load().vq_lfq_staged_workspace_bytes(R, 1, d))
    monkeypatch.setattr(residual_lfq, "_ENTROPY_WS_BUDGET", 3 * per_stage)
    calls.clear()
    chunked = step()
    assert calls == [3, 3, 3, 1], calls
    for a, b in zip(whole, chunked):
        assert torch.equal(a, b)
