"""GPU suite of the fused orthogonal regularisation loss (vq_orthogonal_gram_f32, the kOrth role of the sweep;
losses._OrthogonalFn) against the fp64 closed form of tests/orthogonal_run.py on the CPU.

The tolerance is the project's rule (tests/test_gpu_diversity_codes.py, tests/gumbel_run.py): assert_grad_close with
atol = max(GRAD_ATOL_OF_MAX, 4 x the error the reference's own fp32 op sequence has on the same inputs, on this device, against
fp64) of the largest fp64 entry, and GRAD_RTOL.  Every measured reference error and kernel error is printed.

Shapes: the staged tile holds 32 * max(1, 256 / Dp) codes (Geo<DP, 4>: 256 / 128 / 64 / 32 codes at Dp = 32 / 64 / 128 / 256), a
workgroup owns 128 rows (four waves of 32)."""
from __future__ import annotations

import copy
import functools
import gc

import numpy as np
import pytest
import torch

from orthogonal_run import GRAD_ATOL_OF_MAX, assert_grad_close, closed_form64, gram64, make_codes, reference_sequence, rule

pytestmark = pytest.mark.gpu

DIMS = (8, 20, 32, 64, 100, 128, 200, 256)
ROWS = (1, 31, 32, 33, 129)
HEADS = (1, 3)
CUT_ONE = {32: {1: 1}, 64: {1: 1}, 128: {1: 1}, 256: {1: 1}}


def _tile_codes(d):
    dp = next(p for p in (32, 64, 128, 256) if d <= p)
    return 32 * max(1, 256 // dp)


# per padded width: three whole staged tiles and a partial fourth, and more than 128 rows (two workgroups, a partial last
# wave); at Dp = 256 three tiles are 96 codes, so it takes a fifth tile to pass 128 rows
MULTI_TILE = {d: max(3 * _tile_codes(d), 128) + 5 for d in (32, 64, 128, 256)}


@functools.lru_cache(maxsize=None)
def _case(h, n, d, unit=True, seed=1):
    """(rows, fp64 rowsq and G, the reference's fp32 sequence on the device), computed once and left unchanged."""
    rows = make_codes(h, n, d, seed + 1000 * h + n + 7 * d, unit=unit)
    if not unit:
        rows = rows * 1.7
    rowsq, G = gram64(rows)
    ref32 = reference_sequence(rows.cuda(), torch.float32, normalize=False)
    return rows, rowsq, G, {k: v.cpu() for k, v in ref32.items()}


def _check(h, n, d, unit=True, xd=None):
    from vector_quantization import native

    rows, rowsq, G, ref32 = _case(h, n, d, unit)
    got_sq, got_g = native.orthogonal_gram(rows.cuda() if xd is None else xd)
    torch.cuda.synchronize()
    assert tuple(got_sq.shape) == (h, n) and tuple(got_g.shape) == (h, n, d)
    name = f"[{h}, {n}, {d}]" + ("" if unit else " general rows")
    rule(name, "rowsq", got_sq, rowsq, ref32["rowsq"])
    rule(name, "G", got_g, G, ref32["G"])
    return got_sq, got_g


# ------------------------------------------------------------------------------------------------ kernel against fp64
@pytest.mark.parametrize("h", HEADS, ids=lambda h: f"h{h}")
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_gram_against_fp64(d, h):
    for n in ROWS:
        _check(h, n, d)


@pytest.mark.parametrize("h", HEADS, ids=lambda h: f"h{h}")
@pytest.mark.parametrize("d", sorted(MULTI_TILE), ids=lambda d: f"dp{d}")
def test_several_tiles_and_two_workgroups(d, h):
    n = MULTI_TILE[d]
    assert n > 3 * _tile_codes(d) and n % _tile_codes(d) and n > 128 and n % 32
    _check(h, n, d)


def test_general_rows():
    """The entry does not normalise: rows of any finite length."""
    _check(2, 133, 100, unit=False)


@pytest.mark.parametrize("d,pad", [(100, 3), (20, 1), (64, 12), (7, 0)])
def test_strided_rows(d, pad):
    """Rows inside a wider NaN-filled buffer (odd strides: the scalar row loads; +12: float4 loads with a stride) give the same
    result: nothing between the rows is read."""
    h, n = 2, 70
    rows = _case(h, n, d)[0]
    buf = torch.full((h, n, d + pad), float("nan"), device="cuda")
    buf[..., :d] = rows.cuda()
    got_sq, got_g = _check(h, n, d, xd=buf[..., :d])
    want_sq, want_g = _check(h, n, d)
    assert torch.equal(got_sq, want_sq) and torch.equal(got_g, want_g)


# ------------------------------------------------------------------------------------------------ exactness, determinism
@pytest.mark.parametrize("h,n,d", [(3, 133, 256), (1, 389, 64), (2, 33, 20)])
def test_runs_are_bit_identical_and_rowsq_does_not_depend_on_g(h, n, d):
    from vector_quantization import native

    x = _case(h, n, d)[0].cuda()
    sq1, g1 = native.orthogonal_gram(x)
    sq2, g2 = native.orthogonal_gram(x)
    sq3, g3 = native.orthogonal_gram(x, want_g=False)
    torch.cuda.synchronize()
    assert g3 is None
    assert torch.equal(sq1, sq2) and torch.equal(g1, g2) and torch.equal(sq1, sq3)


def test_rowsq_past_n_is_left_alone():
    from vector_quantization import native

    h, n, d = 2, 133, 32
    x = _case(h, n, d)[0].cuda()
    stride = int(native.load().vq_gumbel_row_stride(n))
    assert stride == 256
    buf = torch.full((h, stride), -7.0, device="cuda")
    sq, _ = native.orthogonal_gram(x, rowsq_out=buf)
    torch.cuda.synchronize()
    assert sq.data_ptr() == buf.data_ptr() and bool((buf[:, n:] == -7.0).all()) and bool((buf[:, :n] > 0).all())


def test_identity_is_exact():
    from vector_quantization import native

    eye = torch.eye(32, device="cuda")[None]
    sq, g = native.orthogonal_gram(eye)
    assert torch.equal(sq, torch.ones((1, 32), device="cuda")) and torch.equal(g, eye)


# ------------------------------------------------------------------------------------------------ values
def test_zero_rows_are_exactly_zero():
    from vector_quantization import native

    h, n, d = 2, 70, 20
    rows = _case(h, n, d)[0].clone()
    rows[0, 3:8] = 0.0
    rows[1, 69] = 0.0
    sq, g = native.orthogonal_gram(rows.cuda())
    assert not bool(sq[0, 3:8].any()) and not bool(g[0, 3:8].any()) and not bool(sq[1, 69].any()) and not bool(g[1, 69].any())
    want_sq, want_g = gram64(rows)
    ref32 = reference_sequence(rows.cuda(), torch.float32, normalize=False)
    rule("zero rows", "rowsq", sq, want_sq, ref32["rowsq"])
    rule("zero rows", "G", g, want_g, ref32["G"])


def test_duplicated_row():
    """Among orthonormal rows the duplicate's cos with its twin is exactly 1: rowsq = 1 + 1, G = twice the row; a duplicated
    generic row gets bit for bit its twin's results."""
    from vector_quantization import native

    rows = torch.eye(32)[None].clone()
    rows[0, 31] = rows[0, 5]
    sq, g = native.orthogonal_gram(rows.cuda())
    want = torch.ones(32)
    want[5] = want[31] = 2.0
    assert torch.equal(sq.cpu()[0], want)
    assert torch.equal(g.cpu()[0, 5], 2 * rows[0, 5]) and torch.equal(g.cpu()[0, 31], 2 * rows[0, 5])
    rows = _case(1, 133, 100)[0].clone()
    rows[0, 130] = rows[0, 2]
    sq, g = native.orthogonal_gram(rows.cuda())
    assert torch.equal(sq[0, 130], sq[0, 2]) and torch.equal(g[0, 130], g[0, 2])
    want_sq, want_g = gram64(rows)
    ref32 = reference_sequence(rows.cuda(), torch.float32, normalize=False)
    rule("duplicate", "rowsq", sq, want_sq, ref32["rowsq"])
    rule("duplicate", "G", g, want_g, ref32["G"])
    assert abs(float((rows[0, 130].double() * rows[0, 2].double()).sum()) - 1) < 1e-6


def test_nan_reaches_every_row(monkeypatch):
    """cos of any row with the row that holds a NaN is NaN: every rowsq entry, every G row and the loss -- on both paths."""
    from vector_quantization import losses, native

    rows = _case(1, 70, 20)[0].clone()
    rows[0, 7, 3] = float("nan")
    sq, g = native.orthogonal_gram(rows.cuda())
    assert bool(torch.isnan(sq).all()) and bool(torch.isnan(g).all())
    monkeypatch.setattr(losses, "ORTHOGONAL_FUSED_MIN_CODES", dict(CUT_ONE))
    assert bool(torch.isnan(losses.orthogonal_loss(rows.cuda())))
    monkeypatch.setenv("VQ_ORTHOGONAL_NO_FUSED", "1")
    assert bool(torch.isnan(losses.orthogonal_loss(rows.cuda())))


# ------------------------------------------------------------------------------------------------ the reference's goldens
def _count_calls(monkeypatch):
    from vector_quantization import search

    calls = []
    original = search._NativeBackend.orthogonal_gram

    def counting(x, *, want_g=True):
        calls.append((tuple(x.shape), want_g))
        return original(x, want_g=want_g)

    monkeypatch.setattr(search._NativeBackend, "orthogonal_gram", staticmethod(counting))
    return calls


def test_fused_loss_matches_the_reference_goldens(monkeypatch):
    """tests/golden/data/orthogonal_fn.npz with the tolerances of tests/test_host_logic_golden.py, through the fused path."""
    from gen import CB_SEED, make_codebook
    from helpers import load_golden
    from vector_quantization import losses

    monkeypatch.setattr(losses, "ORTHOGONAL_FUSED_MIN_CODES", dict(CUT_ONE))
    calls = _count_calls(monkeypatch)
    arrays, _ = load_golden("orthogonal_fn")
    for i, shape in enumerate([(1, 256, 64), (4, 100, 32), (1, 1024, 256)]):
        assert tuple(int(v) for v in arrays[f"shape{i}"]) == shape
        cb = make_codebook(*shape, "S", seed=CB_SEED + i).cuda().requires_grad_(True)
        v = losses.orthogonal_loss(cb)
        v.backward()
        assert calls[-1] == (shape, True) and len(calls) == i + 1
        print(f"{shape}: loss {float(v.detach()):.9g} (golden {float(arrays[f'value{i}']):.9g})")
        np.testing.assert_allclose(float(v.detach()), float(arrays[f"value{i}"]), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(cb.grad[:, :4].cpu().numpy(), arrays[f"grad_rows{i}"], rtol=1e-4, atol=1e-9)


# ------------------------------------------------------------------------------------------------ module level
def _module(variant):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    kw, head_dim = dict(orthogonal_reg_weight=10.0), 64
    if variant == "active_codes_only":
        kw.update(orthogonal_reg_active_codes_only=True)
    elif variant == "max_codes":
        kw.update(orthogonal_reg_max_codes=100)
    elif variant == "separate_heads":
        kw.update(heads=2, codebook_dim=32, separate_codebook_per_head=True)
        head_dim = 32
    torch.manual_seed(17)
    params = CodebookParams(dim=head_dim, codebook_size=256, learnable_codebook=True, ema_update=False)
    return vq.VectorQuantize(dim=64, codebook_params=params, **kw).cuda().train()


def _step(monkeypatch, mod, x):
    """One training step -> the module's loss, x.grad, the codebook's grad and, recorded at the call of the orthogonal loss,
    the selected codes and the gradient it sent back to them (they are handed on as a view of themselves, whose hook sees
    that gradient alone)."""
    from vector_quantization import losses

    seen = {}
    original = losses.orthogonal_loss

    def recording(codes):
        alias = codes.view_as(codes)
        alias.register_hook(lambda g: seen.__setitem__("gc", g.detach().clone()))
        seen.update(c=codes.detach().clone())
        return original(alias)

    monkeypatch.setattr(losses, "orthogonal_loss", recording)
    torch.manual_seed(29)  # (orthogonal_reg_max_codes draws its codes with torch.randperm)
    xd = x.clone().requires_grad_(True)
    _, _, loss, parts = mod(xd, return_loss_breakdown=True)
    loss.sum().backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(losses, "orthogonal_loss", original)
    return dict(loss=loss.detach().sum().reshape(1), orth=parts.orthogonal_reg.detach().reshape(1), gx=xd.grad,
                gcb=mod._codebook.embeddings.grad.detach().clone(), seen=seen)


@pytest.mark.parametrize("variant", ["plain", "active_codes_only", "max_codes", "separate_heads"])
def test_module_step_matches_the_gemm_path(monkeypatch, variant):
    """VectorQuantize(dim=64, K=256, learnable_codebook=True, ema_update=False, orthogonal_reg_weight=10) in train mode,
    x [8, 16, 64], the cut lowered to 1: one step against the same step of a deep copy under VQ_ORTHOGONAL_NO_FUSED=1.  The fp64
    closed form of the recorded codes is the reference, the GEMM path (the reference's fp32 op sequence on this device) measures
    its own error e against it, and the fused path may be 4 e off (floors GRAD_ATOL_OF_MAX, GRAD_RTOL).  The module's outputs
    hold the same other terms on both paths, so fused and GEMM outputs may differ by 4 e + e."""
    from vector_quantization import losses

    monkeypatch.setattr(losses, "ORTHOGONAL_FUSED_MIN_CODES", dict(CUT_ONE))
    fused_mod = _module(variant)
    gemm_mod = copy.deepcopy(fused_mod)
    x = torch.randn((8, 16, 64), generator=torch.Generator().manual_seed(23)).cuda()

    monkeypatch.setenv("VQ_ORTHOGONAL_NO_FUSED", "1")
    calls = _count_calls(monkeypatch)
    want = _step(monkeypatch, gemm_mod, x)
    assert calls == []
    monkeypatch.delenv("VQ_ORTHOGONAL_NO_FUSED")
    got = _step(monkeypatch, fused_mod, x)
    codes = got["seen"]["c"]
    assert calls == [(tuple(codes.shape), True)]
    assert torch.equal(codes, want["seen"]["c"]), "both paths were handed the same codes"
    h, n, d = codes.shape
    print(f"{variant}: codes {tuple(codes.shape)}")
    if variant == "active_codes_only":
        assert h == 1 and 1 < n < 256 and n % 32 != 0, n
    elif variant == "max_codes":
        assert (h, n, d) == (1, 100, 64)
    else:
        assert (h, n, d) == ((2, 256, 32) if variant == "separate_heads" else (1, 256, 64))

    ref64 = closed_form64(codes.cpu())
    loss_err = abs(float(want["orth"]) - float(ref64["loss"])) / abs(float(ref64["loss"]))
    print(f"{variant}: the GEMM path's loss is {loss_err:.2e} off fp64")
    assert_grad_close(got["orth"], ref64["loss"].reshape(1), f"{variant} orthogonal_reg", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * loss_err))
    gc64 = 10.0 * ref64["grad"]  # (d module loss / d orthogonal loss = orthogonal_reg_weight)
    scale = float(gc64.abs().max())
    err = float((want["seen"]["gc"].double().cpu() - gc64).abs().max()) / scale
    print(f"{variant}: the GEMM path's d loss / d codes is {err:.2e} of the largest entry off fp64")
    assert_grad_close(got["seen"]["gc"], gc64, f"{variant} d loss / d codes", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * err))
    # the module's outputs: everything but the orthogonal term is the same computation on both paths
    orth_share = 10.0 * abs(float(ref64["loss"])) / abs(float(want["loss"]))
    assert_grad_close(got["loss"], want["loss"], f"{variant} loss", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * loss_err * orth_share))
    share = scale / float(want["gcb"].abs().max())
    assert_grad_close(got["gcb"], want["gcb"], f"{variant} codebook.grad", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * err * share))
    assert_grad_close(got["gx"], want["gx"], f"{variant} x.grad")  # (the orthogonal loss does not reach x)


# ------------------------------------------------------------------------------------------------ memory
def test_peak_memory_stays_below_one_cosine_matrix(monkeypatch):
    """h = 1, n = 8192, d = 64, fused: forward + backward of losses.orthogonal_loss never have as much as ONE [n, n] fp32 matrix
    (256 MiB) allocated above what the process held before -- the fused path holds the normalised codes, their packed image,
    rowsq [n] and G [n, d]."""
    from vector_quantization import losses

    monkeypatch.setattr(losses, "ORTHOGONAL_FUSED_MIN_CODES", dict(CUT_ONE))
    calls = _count_calls(monkeypatch)
    gc.collect()
    torch.cuda.synchronize()
    foreign = torch.cuda.memory_allocated()  # what earlier tests of the process still hold: not this step's
    n, d = 8192, 64
    codes = torch.randn((1, n, d), generator=torch.Generator().manual_seed(3)).cuda().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    loss = losses.orthogonal_loss(codes)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - foreign
    print(f"peak {peak / 2**20:.1f} MiB (beside {foreign / 2**20:.1f} MiB held by earlier tests); one [n, n] matrix: {n * n * 4 / 2**20:.0f} MiB")
    assert calls == [((1, n, d), True)]
    assert peak < n * n * 4
    assert codes.grad is not None and bool(torch.isfinite(codes.grad).all()) and bool(torch.isfinite(loss.detach()))
    # (the value: E cos^2 = 1 / d between independent random directions)
    assert abs(float(loss.detach()) - (1 - 1 / n) / d) < 0.05 / d
