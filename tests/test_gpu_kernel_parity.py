"""GPU parity proper: HIP kernels (through the C ABI) vs the CPU oracle, bit-exact.

Indices AND winning distances must be identical (the MFMA chain order is the oracle's chain order);
quantized rows are exact gathers; squared-error sums agree to 1e-6 relative.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gen import make_codebook, make_rvq_codebooks, make_x  # noqa: E402


def _native():
    from vector_quantization import native

    native.load()
    return native


def _run(native, x, cb, metric, **kw):
    dev = torch.device("cuda:0")
    r = native.quantize(x.to(dev), cb.to(dev), metric=metric, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu() if v is not None else None) for k, v in r.items()}


SHAPES = [
    # (H, M, K, D)
    (1, 8192, 256, 64),
    (1, 4096, 1024, 256),
    (1, 1024, 8192, 256),
    (8, 256, 8192, 64),
    (1, 111, 300, 100),
    (2, 33, 7, 5),
    (1, 40, 1, 16),
    (1, 257, 1000, 128),
    (1, 64, 4096, 512),
    (1, 1000, 96, 32),
    (1, 130, 70, 24),
]


@pytest.mark.parametrize("H,M,K,D", SHAPES)
@pytest.mark.parametrize("cls", ["S", "G", "Gdup", "R"])
@pytest.mark.parametrize("metric", [0, 1])
def test_single_stage_bit_exact(oracle, H, M, K, D, cls, metric):
    native = _native()
    x = make_x((H, M, D), cls)
    cb = make_codebook(H, K, D, cls)
    ref = oracle.vq_forward(x.numpy(), cb.numpy(), metric, training=False)
    got = _run(native, x, cb[:, None].contiguous(), metric, want_sq_err=True)
    idx = got["idx"][..., 0].numpy()
    np.testing.assert_array_equal(idx, ref["idx"])
    assert np.array_equal(got["best"][..., 0].numpy().view(np.uint32), ref["best"].view(np.uint32)), "distances differ"
    np.testing.assert_array_equal(got["out"].numpy(), ref["out"])
    np.testing.assert_allclose(got["sq_err"].numpy()[0], ref["sq_err"], rtol=1e-6)
    if cls == "Gdup" and K >= 2 and K % 2 == 0:
        assert idx.max() < max(K // 2, 1)


@pytest.mark.parametrize("flags_name", ["F_FORCE_SIMPLE", "F_FORCE_SPLIT"])
@pytest.mark.parametrize("H,M,K,D", [(1, 300, 1000, 256), (2, 100, 333, 48), (1, 64, 4096, 512)])
@pytest.mark.parametrize("metric", [0, 1])
def test_alternate_paths_bit_exact(oracle, flags_name, H, M, K, D, metric):
    native = _native()
    x = make_x((H, M, D), "S")
    cb = make_codebook(H, K, D, "S")
    ref = oracle.vq_forward(x.numpy(), cb.numpy(), metric, training=True)
    got = _run(native, x, cb[:, None].contiguous(), metric, want_sq_err=True, ste=True,
               flags=getattr(native, flags_name))
    np.testing.assert_array_equal(got["idx"][..., 0].numpy(), ref["idx"])
    assert np.array_equal(got["best"][..., 0].numpy().view(np.uint32), ref["best"].view(np.uint32))
    np.testing.assert_array_equal(got["out"].numpy(), ref["out"])
    np.testing.assert_allclose(got["sq_err"].numpy()[0], ref["sq_err"], rtol=1e-6)


def _check_residual(oracle, native, Q, M, K, D, training, cls):
    x = make_x((M, D), cls)
    cbs = make_rvq_codebooks(Q, K, D, cls)
    ref = oracle.rvq_forward(x.numpy(), cbs.numpy(), 0, training=training)
    got = _run(native, x[None], cbs[None].contiguous(), 0, ste=training, want_sq_err=True)
    np.testing.assert_array_equal(got["idx"][0].numpy(), ref["idx"])
    assert np.array_equal(got["best"][0].numpy().view(np.uint32), ref["best"].view(np.uint32))
    np.testing.assert_array_equal(got["out"][0].numpy(), ref["out"])
    np.testing.assert_allclose(got["sq_err"].numpy(), ref["sq_err"], rtol=1e-6)


@pytest.mark.parametrize("Q,M,K,D", [(8, 1024, 1024, 256), (4, 300, 256, 64), (3, 77, 100, 40), (2, 64, 512, 512),
                                     (5, 200, 64, 128)])
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("cls", ["S", "G"])
def test_residual_bit_exact(oracle, Q, M, K, D, training, cls, residual_plan):
    _check_residual(oracle, _native(), Q, M, K, D, training, cls)


# The finalize of the one-wave kernel where no case above reaches it (M = 70: two full row blocks and one of 6 rows): the
# scalar path with residual stages (D = 5; D = 130 is Dp = 256 with D % 4 != 0), and the stage batch of the float4 path
# crossed at Dp = 256 (batches of 8 stages) and at Dp = 512 (batches of 4; K = 64 keeps the launch off the wave-pair kernel).
@pytest.mark.parametrize("Q,M,K,D", [(3, 70, 40, 5), (3, 70, 40, 130), (9, 70, 64, 256), (5, 70, 64, 512)])
@pytest.mark.parametrize("training", [False, True])
def test_residual_finalize_paths_bit_exact(oracle, Q, M, K, D, training, residual_plan):
    _check_residual(oracle, _native(), Q, M, K, D, training, "S")


def test_strided_rows_and_heads(oracle):
    """Head-split view 'b n (h d) -> h (b n) d' is searched in place (no copy)."""
    native = _native()
    H, M, D, K = 4, 200, 64, 512
    x = make_x((M, H * D), "S")
    cb = make_codebook(H, K, D, "S")
    xv = x.view(M, H, D).permute(1, 0, 2)  # [H, M, D], row stride H*D, head stride D
    ref = oracle.vq_forward(np.ascontiguousarray(xv.numpy()), cb.numpy(), 0)
    dev = torch.device("cuda:0")
    xg = x.to(dev)
    out = torch.empty_like(xg)
    r = native.quantize(xg.view(M, H, D).permute(1, 0, 2), cb[:, None].contiguous().to(dev), metric=0,
                        out=out.view(M, H, D).permute(1, 0, 2))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(r["idx"][..., 0].cpu().numpy(), ref["idx"])
    np.testing.assert_array_equal(out.cpu().view(M, H, D).permute(1, 0, 2).numpy(), ref["out"])


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("Q", [1, 3])
def test_unaligned_destination_rows_take_the_scalar_finalize(oracle, Q, training, residual_plan):
    """D % 4 == 0, but the destination's row stride (H * D + 1 floats) is no multiple of 4: no float4 access in the finalize.
    The head-split views of test_strided_rows_and_heads, one stage and three (the one-wave kernel's residual finalize)."""
    native = _native()
    H, M, D, K = 4, 200, 64, 512
    x = make_x((M, H * D), "S")
    xv = x.view(M, H, D).permute(1, 0, 2)  # [H, M, D], row stride H*D, head stride D
    cbs = torch.stack([make_rvq_codebooks(Q, K, D, "S", seed=4242 + 16 * h) for h in range(H)])  # [H, Q, K, D]
    refs = [oracle.rvq_forward(np.ascontiguousarray(xv[h].numpy()), cbs[h].numpy(), 0, training=training) for h in range(H)]
    dev = torch.device("cuda:0")
    xg = x.to(dev)
    out = torch.zeros((M, H * D + 1), dtype=torch.float32, device=dev)
    out_view = out[:, :H * D].view(M, H, D).permute(1, 0, 2)
    r = native.quantize(xg.view(M, H, D).permute(1, 0, 2), cbs.contiguous().to(dev), metric=0, ste=training, want_sq_err=True,
                        sq_err_per_head=True, out=out_view)
    torch.cuda.synchronize()
    for h in range(H):
        np.testing.assert_array_equal(r["idx"][h].cpu().numpy(), refs[h]["idx"])
        assert np.array_equal(r["best"][h].cpu().numpy().view(np.uint32), refs[h]["best"].view(np.uint32))
        np.testing.assert_array_equal(out_view[h].cpu().numpy(), refs[h]["out"])
        np.testing.assert_allclose(r["sq_err"][h].cpu().numpy(), refs[h]["sq_err"], rtol=1e-6)
    assert float(out[:, H * D].abs().max()) == 0.0  # the column behind the rows is not written


def _check_loss_only(oracle, Q, M, K, D):
    native = _native()
    x = make_x((M, D), "S")
    cbs = make_rvq_codebooks(Q, K, D, "S")
    dev = torch.device("cuda:0")
    xg, cg = x[None].to(dev), cbs[None].contiguous().to(dev)
    full = native.quantize(xg, cg, metric=0, ste=True, want_sq_err=True)
    r = native.quantize(xg, cg, metric=0, ste=True, want_sq_err=True, want_out=False)
    torch.cuda.synchronize()
    assert r["out"] is None
    assert torch.equal(r["idx"], full["idx"]) and torch.equal(r["best"].view(torch.int32), full["best"].view(torch.int32))
    np.testing.assert_allclose(r["sq_err"].cpu().numpy(), full["sq_err"].cpu().numpy(), rtol=1e-6)
    if M <= 1000:
        ref = oracle.rvq_forward(x.numpy(), cbs.numpy(), 0, training=True)
        np.testing.assert_array_equal(r["idx"][0].cpu().numpy(), ref["idx"])
        np.testing.assert_allclose(r["sq_err"].cpu().numpy(), ref["sq_err"], rtol=1e-6)


@pytest.mark.parametrize("M,K,D", [(70, 40, 64), (33000, 256, 512)])
def test_loss_only_call_without_destination(oracle, M, K, D):
    """No `out` buffer, squared errors wanted: the finalize computes the sums and stores no rows (the one-wave kernel's short
    rows; the wave-pair kernel at M = 33000)."""
    _check_loss_only(oracle, 1, M, K, D)


@pytest.mark.parametrize("D", [256, 130])
def test_loss_only_residual_call_without_destination(oracle, D, residual_plan):
    """The same with three stages: float4 rows (D = 256) and scalar rows (D = 130)."""
    _check_loss_only(oracle, 3, 70, 40, D)
