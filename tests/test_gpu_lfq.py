"""LFQ on the GPU: the reference fixtures (tests/golden/data/lfq_*.npz), the dense fp64 restatement (tests/lfq_dense.py) at
d = 16 / 20, the memory bound, determinism, and saturated inputs at inv_temperature 100."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from lfq_dense import dense_entropy
from test_lfq_host import FIXTURES, build_module, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run(name, seed_draw=True):
    f, c = load_fixture(name)
    mod = build_module(f, c).to(DEV)
    x = torch.from_numpy(f["x"]).to(DEV).requires_grad_(True)
    mask = torch.from_numpy(f["mask"]).to(DEV) if "mask" in f.files else None
    if seed_draw:
        torch.manual_seed(c.get("draw_seed", 5))
    (out, idx, aux), bd = mod(x, inv_temperature=c.get("tau", 100.0), return_loss_breakdown=True, mask=mask)
    grad = None
    if mod.training:
        r = torch.from_numpy(f["r"]).to(DEV)
        (aux.sum() + (out * r).sum()).backward()
        grad = x.grad
    return f, c, mod, out, idx, aux, bd, grad


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(name):
    f, c, mod, out, idx, aux, bd, grad = _run(name)
    assert torch.equal(idx.cpu(), torch.from_numpy(f["idx"])), "indices differ from the reference"
    want = torch.from_numpy(f["out"])
    got = out.detach().cpu()
    if mod.has_projections:
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    elif mod.training:  # x + (q - x): within one ulp of the reference's value
        ulp = torch.abs(torch.nextafter(want, torch.full_like(want, float("inf"))) - want)
        assert bool(((got - want).abs() <= ulp).all())
    else:
        assert torch.equal(got, want)
    # quantized values bit-exact: the kernel's q against indices_to_codes of the reference's indices
    C, d = mod.num_codebooks, mod.codebook_dim
    from vector_quantization import native

    if not (mod.has_projections or mod.spherical or mod.soft_clamp_input_value or mod.channel_first):
        v = torch.from_numpy(f["x"]).reshape(-1, C, d)
        q, _, _, _ = native.lfq_quantize(v.to(DEV), mod._code_mag)
        codes = mod.cpu().indices_to_codes(torch.from_numpy(f["idx"]), project_out=False).reshape(-1, C, d)
        assert torch.equal(q.cpu(), codes)
    for got_s, key in ((aux, "aux"), (bd.per_sample_entropy, "ps"), (bd.batch_entropy, "cb"), (bd.commitment, "commit")):
        np.testing.assert_allclose(float(got_s), float(f[key]), rtol=1e-5, atol=1e-6, err_msg=key)
    if grad is not None:
        np.testing.assert_allclose(grad.cpu().numpy(), f["grad"], rtol=1e-4, atol=1e-6)


def _native_entropy(v, rows, a, tau, g_ps, g_cb):
    from vector_quantization.lookup_free_quantization import _LfqEntropy

    v = v.detach().requires_grad_(True)
    ps, cb = _LfqEntropy.apply(v, rows, a, tau)
    (g_ps * ps + g_cb * cb).backward()
    return ps.detach(), cb.detach(), v.grad


def _compare(v, rows, a, tau, g_ps=1.0, g_cb=-1.0, rtol_grad=1e-4):
    ps, cb, gv = _native_entropy(v, rows, a, tau, g_ps, g_cb)
    ref = dense_entropy(v, rows, a, tau, g_ps=g_ps, g_cb=g_cb)
    assert torch.isfinite(ps) and torch.isfinite(cb) and bool(torch.isfinite(gv).all())
    np.testing.assert_allclose(float(ps), float(ref["per_sample"]), rtol=1e-5)
    np.testing.assert_allclose(float(cb), float(ref["codebook"]), rtol=1e-5)
    scale = float(ref["grad"].abs().max())
    np.testing.assert_allclose(gv.double().cpu().numpy(), ref["grad"].cpu().numpy(), rtol=rtol_grad, atol=1e-6 * max(1.0, scale))


def test_d16_ragged_strided_against_restatement():
    g = torch.Generator(device=DEV).manual_seed(11)
    base = torch.randn(4093, 2, 40, device=DEV, generator=g) * 0.3
    v = base[:, 1, 3:19].unsqueeze(1)  # [4093, 1, 16], row stride 80 floats
    assert v.stride(0) == 80
    rows = torch.randperm(4093, device=DEV, generator=g)[:4001].sort().values
    _compare(v, rows, 1.0, 1.0)
    _compare(v, None, 1.0, 1.0, g_ps=0.3, g_cb=-0.7)


def test_d20_against_restatement():
    g = torch.Generator(device=DEV).manual_seed(12)
    v = torch.randn(256, 1, 20, device=DEV, generator=g) * 0.2
    _compare(v, None, 1.0, 1.0)


def test_d13_two_codebooks_against_restatement():
    g = torch.Generator(device=DEV).manual_seed(13)
    v = torch.randn(777, 2, 13, device=DEV, generator=g) * 0.5
    _compare(v, None, 0.5, 2.0)


def test_memory_bound_d16_32k_rows():
    from vector_quantization import LFQ

    mod = LFQ(codebook_size=2**16).to(DEV).train()
    x = torch.randn(8, 4096, 16, device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    (out, idx, aux) = mod(x, inv_temperature=1.0)
    (aux + out.sum()).backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < 256 * 2**20, f"forward + backward grew device memory by {grown / 2**20:.1f} MiB"


def test_deterministic_training_calls():
    from vector_quantization import LFQ

    torch.manual_seed(3)
    mod = LFQ(dim=24, codebook_size=2**14, frac_per_sample_entropy=0.75).to(DEV).train()
    x0 = torch.randn(4, 1000, 24, device=DEV)
    res = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        torch.manual_seed(9)
        (out, idx, aux), bd = mod(x, inv_temperature=1.0, return_loss_breakdown=True)
        (aux + (out * 0.5).sum()).backward()
        res.append((aux.detach().clone(), torch.stack([t.detach() for t in bd]), out.detach().clone(), x.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_inv_temperature_100_saturated_and_zero_inputs():
    g = torch.Generator(device=DEV).manual_seed(14)
    v = torch.randn(300, 1, 12, device=DEV, generator=g)
    v[::3] *= 1e3
    v[1::7] = 0.0
    v[2::5, :, ::2] = 0.0
    _compare(v, None, 1.0, 100.0)
    # the module itself stays finite
    from vector_quantization import LFQ

    mod = LFQ(codebook_size=2**12).to(DEV).train()
    x = v.reshape(3, 100, 12).clone().requires_grad_(True)
    (out, idx, aux), bd = mod(x, inv_temperature=100.0, return_loss_breakdown=True)
    aux.backward()
    assert torch.isfinite(aux) and bool(torch.isfinite(x.grad).all())
    assert bool((idx[x.reshape(-1, 12).eq(0).all(-1).reshape(3, 100)] == 0).all())


def test_eval_runs_no_entropy_kernel():
    from vector_quantization import LFQ

    mod = LFQ(codebook_size=2**10).to(DEV).eval()
    x = torch.randn(2, 64, 10, device=DEV)
    (out, idx, aux), bd = mod(x, return_loss_breakdown=True)
    assert aux.item() == 0.0 and all(t is mod.zero for t in bd)
    assert torch.equal(out, torch.where(x > 0, 1.0, -1.0))
    want = ((x > 0).long() * mod.mask).sum(-1)
    assert torch.equal(idx, want)


def test_torch_library_ops():
    v = torch.randn(50, 2, 6, device=DEV)
    q, out, idx, commit = torch.ops.vq_mi355x.lfq_quantize(v, v, 1.0, None, True)
    assert torch.equal(q, torch.where(v > 0, 1.0, -1.0)) and torch.equal(out, q)
    np.testing.assert_allclose(float(commit), float(((v.double() - q.double()) ** 2).sum()), rtol=1e-12)
    ps, avg = torch.ops.vq_mi355x.lfq_entropy_fwd(v, None, 1.0, 1.0)
    assert avg.shape == (2, 64)
    np.testing.assert_allclose(avg.sum(-1).cpu().numpy(), [1.0, 1.0], rtol=1e-5)
    gv = torch.ops.vq_mi355x.lfq_entropy_bwd(v, None, 1.0, 1.0, torch.ones((), device=DEV), torch.zeros_like(avg))
    assert gv.shape == v.shape and bool(torch.isfinite(gv).all())
