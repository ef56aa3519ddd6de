"""The fp64 restatements (tests/lfq_dense.py, tests/rlfq_dense.py) checked on their own, on the CPU: they are the oracle
of the GPU tests at every codebook_dim, so they are held to fp64 autograd's gradcheck and to central differences here."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from lfq_dense import EPS, dense_entropy, dense_entropy_weighted
from rlfq_dense import restate, stage_rows


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 6])
def test_weighted_gradient_gradchecks(d):
    """The weighted restatement's gradient is d/dv of its own loss, written independently here (gradcheck in fp64)."""
    g = _gen(d)
    C, N = 2, 5
    v = torch.randn(N, C, d, generator=g, dtype=torch.float64) * 0.7
    rows = torch.tensor([0, 2, 3])
    w_ps = 0.37
    w_cb = torch.randn(C, 1 << d, generator=g, dtype=torch.float64)
    from lfq_dense import code_signs

    codes = code_signs(d, "cpu") * 0.8

    def loss(vv):
        p = torch.softmax(2.0 * 1.3 * torch.einsum("rcd,pd->rcp", vv[rows], codes), dim=-1)
        return w_ps * (-p * p.clamp(min=EPS).log()).sum() + (w_cb * p).sum()

    vv = v.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(loss, (vv,), eps=1e-6, atol=1e-8)
    (want,) = torch.autograd.grad(loss(vv), vv)
    got = dense_entropy_weighted(v, rows, 0.8, 1.3, w_ps, w_cb)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)
    assert bool((got[[1, 4]] == 0).all())


@pytest.mark.parametrize("d", [1, 4, 6])
def test_dense_entropy_central_differences(d):
    """dense_entropy's grad against central differences of its own per-sample and codebook values."""
    g = _gen(10 + d)
    v = torch.randn(7, 2, d, generator=g, dtype=torch.float64) * 0.6
    rows = torch.tensor([0, 1, 3, 6])
    g_ps, g_cb = 0.7, -1.3
    ref = dense_entropy(v, rows, 0.9, 1.7, g_ps=g_ps, g_cb=g_cb)

    def f(vv):
        r = dense_entropy(vv, rows, 0.9, 1.7)
        return g_ps * float(r["per_sample"]) + g_cb * float(r["codebook"])

    h = 1e-6
    num = torch.zeros_like(v)
    for idx in range(v.numel()):
        e = torch.zeros(v.numel(), dtype=torch.float64)
        e[idx] = h
        e = e.reshape(v.shape)
        num.view(-1)[idx] = (f(v + e) - f(v - e)) / (2 * h)
    torch.testing.assert_close(ref["grad"], num, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("d", [3, 6, 9])
def test_weighted_equals_dense_entropy_with_module_weights(d):
    """w_cb built from avg_prob as _LfqEntropy.backward builds it reproduces dense_entropy's gradient."""
    g = _gen(20 + d)
    N, C = 40, 3
    v = torch.randn(N, C, d, generator=g, dtype=torch.float64) * 0.5
    rows = torch.randperm(N, generator=g)[:29].sort().values
    g_ps, g_cb, tau, a = 0.6, -0.9, 2.0, 0.7
    ref = dense_entropy(v, rows, a, tau, g_ps=g_ps, g_cb=g_cb)
    R = rows.numel()
    avg = ref["avg_prob"]
    dh = -(avg.clamp(min=EPS).log() + (avg >= EPS).to(avg.dtype))
    got = dense_entropy_weighted(v, rows, a, tau, g_ps / (R * C), dh * (g_cb / (C * R)))
    torch.testing.assert_close(got, ref["grad"], rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("d", [2, 6, 11])
def test_centring_identity(d):
    """Adding one constant to every w_cb[c, k], or to G through w_ps, leaves the fp64 gradient unchanged: the identity the
    entropy backward kernel's centring relies on (sum_k p_k (b_k,i - pi_i) = 0).  The per-sample term's G = -(log p + 1)
    shifts by a constant when w_ps * (log p) is replaced by w_ps * (log p + c); as a loss that is w_ps * c * sum_k p_k."""
    g = _gen(30 + d)
    v = torch.randn(23, 2, d, generator=g, dtype=torch.float64) * 0.8
    w_cb = torch.randn(2, 1 << d, generator=g, dtype=torch.float64)
    base = dense_entropy_weighted(v, None, 1.0, 1.5, 0.3, w_cb)
    scale = float(base.abs().max())
    for c in (1.0, -37.5, 1e3):
        shifted = dense_entropy_weighted(v, None, 1.0, 1.5, 0.3, w_cb + c)
        assert float((shifted - base).abs().max()) <= 1e-12 * max(scale, abs(c))
    per_code = dense_entropy_weighted(v, None, 1.0, 1.5, 0.3, w_cb + torch.tensor([[5.0], [-2.0]], dtype=torch.float64))
    assert float((per_code - base).abs().max()) <= 1e-12 * 5.0
    # a constant in G: w_ps * sum_k p_k is a constant loss (sum_k p_k = 1), so w_cb = w_ps * c adds nothing
    assert float((dense_entropy_weighted(v, None, 1.0, 1.5, 0.3, w_cb + 0.3 * 11.5) - base).abs().max()) <= 1e-12 * 11.5


@pytest.mark.parametrize("spherical,clamp", [(False, None), (False, 2.0), (True, None), (True, 1.5)])
def test_rlfq_restatement_gradchecks(spherical, clamp):
    """restate's dL/dx is the fp64 gradient of the losses and <g_out, out> it states, with the residual detached and the
    straight-through value: checked against an independent fp64 autograd of the chain at d = 4, three stages."""
    d, S, N = 4, 3, 9
    g = _gen(40 + int(spherical) + (0 if clamp is None else 2))
    kwargs = dict(codebook_size=1 << d, spherical=spherical, soft_clamp_input_value=clamp, entropy_loss_weight=0.1,
                  commitment_loss_weight=0.25)
    x = torch.randn(N, d, generator=g) * 0.8
    x[4] = 0.0  # an all-zero row (spherical: the 1e-12 branch of F.normalize)
    g_out = torch.randn(N, d, generator=g)
    mask = torch.ones(N, dtype=torch.bool)
    mask[[1, 7]] = False
    rows = stage_rows(N, mask, 1.0, S)
    res = restate(kwargs, {}, x, mask, g_out, S, rows, g_loss=1.0)
    assert res["grad"].device == x.device and res["losses"].device == x.device

    from lfq_dense import code_signs

    def stage_loss(r64, q):
        scale = 2.0**-q
        c = None if clamp is None else clamp * 0.5**q
        u = r64 if c is None else (r64 / c).tanh() * c
        vq = F.normalize(u, dim=-1) * scale if spherical else u
        mag = scale
        if spherical:
            mag = float(F.normalize(torch.full((1, d), scale, dtype=torch.float32), dim=-1)[0, 0] * scale)
        qv = torch.where(vq > 0, mag, -mag).detach()
        p = torch.softmax(2.0 * 100.0 * vq[rows[q]] @ (code_signs(d, "cpu") * mag).T, dim=-1)

        def ent(pp):
            return (-pp * pp.clamp(min=EPS).log()).sum(-1)

        e = (vq - qv) * mask[:, None].double()
        return 0.1 * (ent(p).mean() - ent(p.mean(0))) + 0.25 * (e * e).sum() / (int(mask.sum()) * d) + (g_out.double() * vq).sum()

    # the residual chain in fp32 as the module runs it; each stage's terms in fp64 at its residual, d r_q / d x = I
    want = torch.zeros(N, d, dtype=torch.float64)
    residual = x.clone()
    for q in range(S):
        r64 = residual.double().requires_grad_(True)
        if q == 0:  # autograd of the stage against finite differences, the all-zero row held fixed (its sign step)
            keep = torch.tensor([i for i in range(N) if i != 4])

            def on_rows(t, r=r64.detach()):
                return stage_loss(r.index_copy(0, keep, t), 0)

            assert torch.autograd.gradcheck(on_rows, (r64.detach()[keep].clone().requires_grad_(True),), eps=1e-7, atol=1e-6)
        want += torch.autograd.grad(stage_loss(r64, q), r64)[0]
        scale = 2.0**-q
        c = None if clamp is None else clamp * 0.5**q
        u = residual if c is None else (residual / c).tanh() * c
        vq = F.normalize(u, dim=-1) * scale if spherical else u
        mag = scale
        if spherical:
            mag = float(F.normalize(torch.full((1, d), scale, dtype=torch.float32), dim=-1)[0, 0] * scale)
        residual = residual - (vq + (torch.where(vq > 0, mag, -mag) - vq))
    # restate takes the commitment error v - q from the fp32 chain's v: 1 ulp of fp32 at most between the two
    torch.testing.assert_close(res["grad"], want, rtol=1e-6, atol=1e-9)
