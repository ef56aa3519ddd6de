"""LatentQuantize on the GPU: every reference fixture (tests/golden/data/lq_*.npz) through the fused path and the torch
fallback, fused against fallback at 65 536 and 1 000 003 positions, the fused loss and gradient against the fixtures'
fp64 restatement, indices_to_codes on GPU indices, the native launch count, determinism, opcheck and torch.compile."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest
import torch

from test_lq_host import FIXTURES, build_module, comparable_rows, load_fixture, projected

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT32_MIN = -(2**31)


@contextlib.contextmanager
def fallback():
    """Route every forward to the torch fallback (the reference's forward, on the GPU)."""
    from vector_quantization import latent_quantization as lq

    orig = lq._fused_ok
    lq._fused_ok = lambda *a: False
    try:
        yield
    finally:
        lq._fused_ok = orig


@contextlib.contextmanager
def count_native():
    """Calls of the native entry points: name -> list of keyword arguments."""
    from vector_quantization import native

    calls = {}
    saved = {}
    for name in ("lq_quantize", "lq_backward", "fsq_quantize", "fsq_backward", "fsq_decode"):
        fn = saved[name] = getattr(native, name)

        def wrap(*a, _fn=fn, _name=name, **k):
            calls.setdefault(_name, []).append(k)
            return _fn(*a, **k)

        setattr(native, name, wrap)
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(native, name, fn)


def _run(name, fused):
    f, c = load_fixture(name)
    mod = build_module(f, c).to(DEV)
    x = torch.from_numpy(f["x"]).to(DEV).requires_grad_(True)
    with contextlib.nullcontext() if fused else fallback():
        with count_native() as calls:
            out, idx, loss = mod(x)
            ((out * torch.from_numpy(f["r"]).to(DEV)).sum() + loss).backward()
    return f, c, mod, out, idx, loss, x.grad, calls


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "fallback"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(name, fused):
    f, c, mod, out, idx, loss, grad, calls = _run(name, fused)
    assert ("lq_quantize" in calls) == fused
    want_idx = torch.from_numpy(f["idx"])
    assert idx.dtype == want_idx.dtype and idx.shape == want_idx.shape and out.shape == f["out"].shape
    got = out.detach().cpu().numpy()
    keep = comparable_rows(f, c)
    assert keep.mean() >= 0.75
    gi, wi = idx.cpu().numpy().reshape(-1), f["idx"].reshape(-1)
    if projected(f):
        np.testing.assert_allclose(got, f["out"], rtol=1e-5, atol=1e-6)
        assert np.array_equal(gi[keep], wi[keep])  # the generator left no row inside the margin
    else:
        assert np.array_equal(got.view(np.uint32), f["out"].view(np.uint32)), "out differs from the reference"
        # every row for d <= 7; for d >= 8 the order-free rows (torch's order over 8 and more terms is not pinned)
        print(f"{name}: {int((gi != wi).sum())} of {gi.size} indices differ from the reference, {int((gi[keep] != wi[keep]).sum())} "
              f"on the {int(keep.sum())} compared rows")
        assert np.array_equal(gi[keep], wi[keep]), "indices differ from the reference"
    # loss: against the fp64 restatement, within 2 x the reference's own fp32 distance or 2^-18 relative (at most 3
    # roundings per term, 16 serial adds per thread and an 8-level tree per workgroup in fp32, the partials in fp64, then
    # the mean, two weight products and their sum in fp32: under 32 x 2^-24 = 2^-19, doubled)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    got_loss, loss64 = float(loss.detach()), float(f["loss64"])
    print(f"{name} {'fused' if fused else 'fallback'}: loss {got_loss!r} fp64 {loss64!r} ref dev {float(f['loss_ref_dev']):.3e}")
    if not c.get("train", True):
        assert got_loss == 0.0
    elif np.isnan(loss64):
        assert np.isnan(got_loss)
    elif projected(f):
        np.testing.assert_allclose(got_loss, loss64, rtol=1e-5, atol=1e-7)  # hipBLASLt's last bits of z and out
    else:
        assert abs(got_loss - loss64) <= max(2 * float(f["loss_ref_dev"]), 2.0**-18 * abs(loss64))
    # gradient: against the fixture's fp32 dL/dx within 2 x its distance from the fp64 restatement + 1e-6
    g = grad.cpu().numpy()
    fin = np.isfinite(f["grad64"]) & np.isfinite(f["grad"])
    tol = 2 * float(f["grad_ref_dev"]) + 1e-6
    print(f"{name}: largest gradient distance {np.abs(g[fin] - f['grad'][fin]).max(initial=0.0):.3e} (bound {tol:.3e})")
    np.testing.assert_allclose(g[fin], f["grad"][fin], rtol=1e-5 if projected(f) else 0, atol=tol)
    if not projected(f) and not fused:
        # (fused, equal weights: the loss terms' gradients cancel and g_out is returned as it is, also at a non-finite
        # element, where the reference's autograd leaves NaN - NaN)
        assert np.array_equal(np.isnan(g), np.isnan(f["grad"]))
    for t in mod.values_per_latent:
        assert getattr(t, "grad", None) is None
    # indices_to_codes on GPU indices: the decode kernel, bitwise the CPU helper
    with torch.no_grad():
        valid = torch.from_numpy(f["idx_valid"])
        codes = mod.indices_to_codes(valid.to(DEV)).cpu().numpy()
        cpu_codes = build_module(f, c).indices_to_codes(valid, project_out=False).numpy()
        dev_codes = mod.indices_to_codes(valid.to(DEV), project_out=False).cpu().numpy()
    assert np.array_equal(dev_codes.view(np.uint32), cpu_codes.view(np.uint32))
    if projected(f):
        np.testing.assert_allclose(codes, f["codes_from_idx"], rtol=1e-5, atol=1e-6)
    else:
        assert np.array_equal(codes.view(np.uint32), f["codes_from_idx"].view(np.uint32))


def test_backward_kernel_runs_only_for_unequal_weights():
    """Weights 0.25 / 0.1 launch lq_backward_kernel; the defaults (equal weights: the two loss gradients cancel) and a
    forward whose loss is not differentiated launch nothing."""
    for name, want in (("lq_w025_01", 1), ("lq_w025_01_img", 1), ("lq_seq", 0), ("lq_w0", 0), ("lq_d16", 0)):
        *_, calls = _run(name, True)
        assert len(calls.get("lq_backward", [])) == want, (name, calls)
        assert len(calls["lq_quantize"]) == 1


@pytest.mark.parametrize("positions", [65536, 1_000_003])
@pytest.mark.parametrize("case", ["seq", "img", "d7", "c2_proj", "train"])
def test_fused_equals_fallback(case, positions):
    from vector_quantization import LatentQuantize

    torch.manual_seed(1)
    g = torch.Generator(device=DEV).manual_seed(9)
    kw = dict(seq=dict(levels=[6, 7, 10, 11], dim=4), img=dict(levels=[5, 5, 8], dim=3),
              d7=dict(levels=[3, 4, 5, 6, 7, 4, 3], dim=7), c2_proj=dict(levels=[5, 5, 8], dim=32, num_codebooks=2),
              train=dict(levels=[15, 22, 24], dim=3, commitment_loss_weight=0.25, quantization_loss_weight=0.1))[case]
    mod = LatentQuantize(**kw).to(DEV).train(case == "train")
    if case == "img":
        assert positions in (65536, 1_000_003)
        shape = (1, 3, 256, 256) if positions == 65536 else (1, 3, 1_000_003, 1)
    else:
        shape = (1, kw["dim"], positions)
    x = torch.randn(*shape, device=DEV, generator=g) * 0.5
    if case == "c2_proj":
        # projections: hand both paths the same quantizer input, so the comparison is of the kernel alone
        with torch.no_grad():
            z = mod.project_in(x.movedim(1, -1))  # [1, positions, 2 * 3]
            from vector_quantization.latent_quantization import fused_quantize

            codes, idx, _ = fused_quantize(z, mod._level_values, mod._flat_tables(mod._tables_on(z.device)), 2, None)
            want = mod.quantize(z.reshape(1, positions, 2, 3))
            want_idx = mod.codes_to_indices(want)
        assert torch.equal(codes.reshape(want.shape), want) and torch.equal(idx, want_idx)
        out, idx2, _ = mod(x)
        assert out.shape == x.shape and idx2.shape == (1, positions, 2)
        return
    res = []
    for fused in (True, False):
        xi = x.clone().requires_grad_(True)
        with contextlib.nullcontext() if fused else fallback():
            out, idx, loss = mod(xi)
            (out.sum() + loss * 1000.0).backward()
        res.append((out.detach(), idx, loss.detach(), xi.grad))
    (o1, i1, l1, g1), (o2, i2, l2, g2) = res
    assert o1.shape == x.shape and i1.shape == i2.shape and i1.dtype == i2.dtype == torch.int32
    assert torch.equal(o1, o2), "out differs between the fused path and the fallback"
    assert torch.equal(i1, i2), "indices differ between the fused path and the fallback"
    if case == "train":
        print(f"train {positions}: fused loss {float(l1)!r} fallback {float(l2)!r}")
        # the fused loss is within 2^-19 relative of the exact value (test_fixture); torch's fp32 mean over n = 3 x positions
        # elements is a tree of at most log2(n) + a few roundings per path, under 32 x 2^-24 relative as well
        assert abs(float(l1) - float(l2)) <= 2 * 2.0**-19 * abs(float(l2))
        np.testing.assert_allclose(g1.cpu().numpy(), g2.cpu().numpy(), rtol=1e-5, atol=1e-6)
    else:
        assert float(l1) == 0.0 == float(l2)


def test_reference_test_forward_configurations():
    """The reference's own four test_forward configurations (all dim = 4) on GPU tensors."""
    from vector_quantization import LatentQuantize

    torch.manual_seed(4)
    for kw in (dict(levels=[5, 5, 8]), dict(levels=[5, 5, 8], optimize_values=False), dict(levels=[5, 5, 5]),
               dict(levels=5, codebook_dim=3)):
        mod = LatentQuantize(dim=4, **kw).to(DEV)
        x = torch.randn(2, 4, 32, device=DEV)
        quantized, indices, loss = mod(x)
        assert quantized.shape == x.shape and indices.shape == (2, 32) and loss.dim() == 0
        np.testing.assert_allclose(quantized.detach().cpu().numpy(), mod.indices_to_codes(indices).detach().cpu().numpy(),
                                   rtol=1e-5, atol=1e-6)


def test_plain_list_tables_follow_the_input_device():
    from vector_quantization import LatentQuantize

    mod = LatentQuantize(levels=[5, 5, 8], dim=3, optimize_values=False).to(DEV).eval()
    assert all(t.device.type == "cpu" for t in mod.values_per_latent)
    x = torch.randn(2, 3, 500, device=DEV)
    out, idx, _ = mod(x)
    mod.values_per_latent = [t * 0.5 for t in mod.values_per_latent]  # new tensors: the device copy is refreshed
    out2, _, _ = mod(x)
    with fallback():
        want2, _, _ = mod(x)
    assert not torch.equal(out, out2) and torch.equal(out2, want2)


def test_native_launch_count():
    """An eval forward without projections is one native call that launches one kernel (no loss requested); a training
    forward is one call that launches two (quantize + loss reduce: the call carries loss_weights)."""
    from vector_quantization import LatentQuantize

    mod = LatentQuantize(levels=[5, 5, 8], dim=3).to(DEV)
    x = torch.randn(2, 3, 4096, device=DEV)
    mod(x)  # caches
    for training, kernels in ((False, 1), (True, 2)):
        mod.train(training)
        with count_native() as calls:
            mod(x)
        assert list(calls) == ["lq_quantize"] and len(calls["lq_quantize"]) == 1, calls
        assert 1 + (calls["lq_quantize"][0]["loss_weights"] is not None) == kernels


def test_two_training_steps_bitwise_equal():
    from vector_quantization import LatentQuantize

    mod = LatentQuantize(levels=[6, 7, 10, 11], dim=4, commitment_loss_weight=0.25, quantization_loss_weight=0.1).to(DEV).train()
    x0 = torch.randn(3, 4, 70001, device=DEV) * 0.5
    res = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        out, idx, loss = mod(x)
        ((out * out).sum() + loss).backward()
        res.append((out.detach(), idx, loss.detach(), x.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_nonfinite_and_unsorted_tables_at_scale():
    from vector_quantization import LatentQuantize

    mod = LatentQuantize(levels=[5, 5, 8], dim=3).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(3)
    with torch.no_grad():
        for t in mod.values_per_latent:
            t.copy_(t[torch.randperm(t.numel(), device=DEV, generator=g)])
        mod.values_per_latent[2][3] = float("nan")
    x = torch.randn(1, 3, 5000, device=DEV, generator=g)
    x[0, 0, 7] = float("nan")
    x[0, 1, 9] = float("inf")
    out, idx, _ = mod(x)
    with fallback():
        want, want_idx, _ = mod(x)
    assert torch.equal(out.isnan(), want.isnan()) and torch.equal(out.nan_to_num(7.0), want.nan_to_num(7.0))
    assert torch.equal(idx, want_idx) and bool((idx == INT32_MIN).all())


def test_torch_library_opcheck():
    g = torch.Generator(device=DEV).manual_seed(2)
    levels = [6, 7, 10, 11]
    z = torch.randn(2, 4, 300, device=DEV, generator=g).transpose(1, 2)
    tab = torch.randn(sum(levels), device=DEV, generator=g)
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.vq_mi355x.lq_quantize.default, (z, levels, tab, 1, True, True, 0.25, 0.1), test_utils=utils)
    torch.library.opcheck(torch.ops.vq_mi355x.lq_quantize.default, (z, levels, tab, 1, False, False, 0.0, 0.0), test_utils=utils)
    out, idx, loss = torch.ops.vq_mi355x.lq_quantize(z, levels, tab, 1, True, True, 0.25, 0.1)
    gl = torch.ones((), device=DEV)
    torch.library.opcheck(torch.ops.vq_mi355x.lq_backward.default, (z, out, torch.ones_like(z), gl, 0.01), test_utils=utils)
    gx = torch.ops.vq_mi355x.lq_backward(z, out, torch.ones_like(z), gl, 0.01)
    np.testing.assert_allclose(gx.cpu().numpy(), (1 + 0.01 * (out - z)).cpu().numpy(), rtol=1e-6, atol=1e-7)
    m = float(((out - z) ** 2).double().mean())
    np.testing.assert_allclose(loss.cpu().numpy(), [0.35 * m, m], rtol=1e-6)


def test_compiled_eval_forward_equals_eager():
    from vector_quantization import LatentQuantize

    mod = LatentQuantize(levels=[6, 7, 10, 11], dim=4).to(DEV).eval()
    x = torch.randn(2, 4, 3000, device=DEV) * 0.5
    with torch.no_grad():
        want = mod(x)
        got = torch.compile(mod, backend="aot_eager", fullgraph=True)(x)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
