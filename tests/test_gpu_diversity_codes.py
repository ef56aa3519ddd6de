"""GPU suite of the diversity loss's fused gradient with respect to a learnable codebook (vq_diversity_backward_codes_f32,
the kDivC role of the sweep; losses._DiversityFn with codes that require grad) against the fp64 closed form of
tests/diversity_codes_run.py on the CPU.

The tolerance is the project's rule (tests/test_gpu_diversity.py, tests/gumbel_run.py): assert_grad_close with
atol = max(GRAD_ATOL_OF_MAX, 4 x the error the reference's own fp32 op sequence has on the same inputs against fp64) of the
largest fp64 entry, and GRAD_RTOL.  The shapes, inputs and seeds are those of tests/test_gpu_diversity.py (restated), so that
no fp64 entry of A lies within 2 % of the clamp 1e-5 -- asserted per case on the CPU.  Every measured reference error and
kernel error is printed."""
from __future__ import annotations

import copy
import functools
import gc

import pytest
import torch

from diversity_codes_run import codes_gradient64, reference_sequence_codes
from diversity_run import clamp_margin, make_inputs
from gumbel_run import GRAD_ATOL_OF_MAX, GRAD_RTOL, assert_grad_close

pytestmark = pytest.mark.gpu

G_LOSS = 0.7  # upstream gradient of the loss
TEMPERATURES = (1.0, 100.0)
METRICS = ("euclid", "dot")

# name -> ((H, B, N, K, D), pos_div), as in tests/test_gpu_diversity.py: M = B * N * pos_div rows per head, Ch = B * pos_div
SHAPES = {
    "c33": ((1, 33, 2, 301, 100), 1),         # one real row in a second sub-tile: 31 padding rows with |x|^2 = +inf under Euclid
    "c5": ((1, 5, 7, 40, 16), 1),             # mostly padding
    "c1": ((1, 1, 40, 7, 5), 1),
    "n1": ((1, 70, 1, 520, 64), 1),
    "k1": ((1, 8, 3, 1, 8), 1),               # one code: the gradient is exactly 0
    "k7": ((1, 40, 2, 7, 24), 1),             # fewer codes than a wave's 32
    "k1000": ((1, 8, 9, 1000, 128), 1),       # a partial last block of codes
    "dp256": ((1, 32, 3, 512, 256), 1),
    "heads2": ((2, 16, 4, 130, 32), 1),
    "shared2": ((1, 6, 5, 90, 40), 2),        # pos_div = 2
    "splits": ((1, 2, 70, 64, 32), 1),        # nine staged tiles, one workgroup column: nine blockIdx.z
    "splits_spp2": ((1, 40, 6, 64, 64), 1),   # positions of two sub-tiles, three staged tiles
}
SEEDS = {("c33", "euclid", 100.0): 2, ("c33", "dot", 100.0): 2, ("c1", "euclid", 100.0): 2, ("n1", "dot", 100.0): 2,
         ("k1000", "dot", 100.0): 5, ("dp256", "euclid", 100.0): 3, ("dp256", "dot", 100.0): 4, ("heads2", "dot", 100.0): 2,
         ("shared2", "dot", 100.0): 2, ("splits", "euclid", 100.0): 2, ("splits", "dot", 100.0): 8,
         ("splits_spp2", "dot", 100.0): 6}


def _metric(metric):
    from vector_quantization import search

    return search.DOT if metric == "dot" else search.EUCLID


@functools.lru_cache(maxsize=None)
def _case(name, metric, T):
    """(x, c, fp64 closed form, the reference's fp32 sequence) on the CPU, computed once and left unchanged."""
    (h, b, n, k, d), pos_div = SHAPES[name]
    dot = metric == "dot"
    x, c = make_inputs(h, b, n, k, d, dot, SEEDS.get((name, metric, T), 1), pos_div)
    ref64 = codes_gradient64(x, c, T, n, pos_div, dot, g_loss=G_LOSS)
    margin = clamp_margin(ref64["A"])
    assert margin > 0.02, f"{name} {metric} T={T}: an fp64 A entry lies within {margin:.2%} of the clamp; pick another seed"
    ref32 = reference_sequence_codes(x, c, T, n, pos_div, dot, dtype=torch.float32, g_loss=G_LOSS)
    return x, c, ref64, ref32


def _native(x, c, T, n, pos_div, mt, xd=None, gc_out=None):
    """The existing stats / accumulate / upstream / delta calls, then the codes sweep -> gc [H, K, D] on the GPU."""
    from vector_quantization import losses, native

    xd = x.cuda() if xd is None else xd
    cd = c.cuda()
    h, m, _ = x.shape
    k = c.shape[1]
    packed = native.pack_codebooks(cd, mt)
    lse2 = native.diversity_stats(xd, cd, metric=mt, temperature=T, packed=packed)
    table = native.diversity_accumulate(xd, cd, lse2, metric=mt, temperature=T, n_positions=n, pos_div=pos_div)
    U, _ = losses.diversity_upstream(table, G_LOSS, n, h * m // n, k)
    kw = dict(metric=mt, temperature=T, n_positions=n, pos_div=pos_div)
    delta = native.diversity_delta(xd, cd, lse2, U, packed=packed, **kw)
    out = native.diversity_backward_codes(xd, cd, lse2, delta, U, out=gc_out, **kw)
    torch.cuda.synchronize()
    return out


def _rule(case, what, have, want, r32):
    """assert_grad_close under the rule of the module docstring; prints the reference's error and the kernel's."""
    want = torch.as_tensor(want).detach().double().cpu()
    have = torch.as_tensor(have).detach().double().cpu().reshape(want.shape)
    r32 = torch.as_tensor(r32).detach().double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(have).all()), (case, what)
    ref_err = float((r32 - want).abs().max() / max(float(want.abs().max()), 1e-300))
    print(f"{case} {what}: the reference's fp32 sequence is {ref_err:.2e} of the largest entry off fp64")
    assert_grad_close(have, want, f"{case} {what}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * ref_err))


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("T", TEMPERATURES, ids=lambda t: f"T{t:g}")
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_grad_codes_against_fp64(name, metric, T):
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, ref64, ref32 = _case(name, metric, T)
    got = _native(x, c, T, n, pos_div, _metric(metric))
    assert tuple(got.shape) == (h, k, d)
    _rule(f"{name} {metric} T={T:g}", "gc", got, ref64["gc"], ref32["gc"])
    if name == "k1":  # p = 1 and U - delta = 0: no rounding to forgive
        assert float(ref64["gc"].abs().max()) == 0.0 and not bool(got.any()), "one code: the gradient is exactly 0"


@pytest.mark.parametrize("metric", METRICS)
def test_strided_x_rows(metric):
    """x rows inside wider NaN-filled buffers (row stride D + 12, a 16-byte multiple, and D + 3: the scalar row loads) give
    the same result: nothing between the rows is read."""
    name, T = "c33", 1.0
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, ref64, ref32 = _case(name, metric, T)
    for pad in (12, 3):
        xbuf = torch.full((h, x.shape[1], d + pad), float("nan"), device="cuda")
        xbuf[..., :d] = x.cuda()
        got = _native(x, c, T, n, pos_div, _metric(metric), xd=xbuf[..., :d])
        _rule(f"{name} {metric} strided +{pad}", "gc", got, ref64["gc"], ref32["gc"])


@pytest.mark.parametrize("name", ["c33", "heads2", "splits", "k7"])
def test_nothing_outside_grad_codes_is_written(name):
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, ref64, ref32 = _case(name, "euclid", 1.0)
    guard, size = 1024, h * k * d
    buf = torch.full((size + 2 * guard,), 7.0, device="cuda")
    out = buf[guard:guard + size].view(h, k, d)
    got = _native(x, c, 1.0, n, pos_div, _metric("euclid"), gc_out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + size:] == 7.0).all()), "grad_codes wrote outside [H, K, D]"
    _rule(f"{name} guarded", "gc", got, ref64["gc"], ref32["gc"])


@pytest.mark.parametrize("name", ["splits", "splits_spp2", "heads2"])
def test_two_runs_are_bit_identical(name):
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, _, _ = _case(name, "euclid", 100.0)
    first = _native(x, c, 100.0, n, pos_div, _metric("euclid"))
    second = _native(x, c, 100.0, n, pos_div, _metric("euclid"))
    assert torch.equal(first, second)


def _plan(h, m, k, d, n, cus):
    """(image rows Mp, padded dim, splits) of the documented plan: every CU a workgroup, at most 64 splits, whole staged tiles."""
    dp = next(p for p in (32, 64, 128, 256) if d <= p)
    tile = 32 * max(1, 256 // dp)
    cp = (m // n + 31) // 32 * 32
    mp = (n * cp + tile - 1) // tile * tile
    ntiles = mp // tile
    want = max(1, min(64, ntiles, -(-cus // ((k + 127) // 128 * h))))
    per = -(-ntiles // want)
    return mp, dp, -(-ntiles // per)


def test_row_splits_cover_several_workgroups():
    """The `splits` shapes really run more than one blockIdx.z, and the sizer holds one partial [H, K, D] per split."""
    from vector_quantization import native

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name in ("splits", "splits_spp2"):
        (h, b, n, k, d), pos_div = SHAPES[name]
        m = b * n * pos_div
        mp, dp, splits = _plan(h, m, k, d, n, cus)
        assert splits >= 2, (name, splits)
        floats = h * (mp * (dp + 4) + 2048) + 2 * h * mp + splits * h * k * d
        assert native.load().vq_diversity_codes_workspace_bytes(h, m, k, d, n) == 4 * floats, name


def test_no_rows_clears_grad_codes():
    from vector_quantization import native

    h, k, d, n = 2, 40, 24, 4
    x = torch.empty((h, 0, d), device="cuda")
    cb = torch.randn((h, k, d), device="cuda")
    stat = torch.empty((h, 0), device="cuda")
    U = torch.zeros((n, int(native.load().vq_gumbel_row_stride(k))), device="cuda")
    out = torch.full((h, k, d), 7.0, device="cuda")
    got = native.diversity_backward_codes(x, cb, stat, stat, U, n_positions=n, pos_div=1, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and not bool(out.any())


# ------------------------------------------------------------------------------------------------ the loss function
def _loss_step(x, c, metric, T, n, x_grad=True):
    from vector_quantization import losses

    xd = x.cuda().requires_grad_(x_grad)
    cd = c.cuda().requires_grad_(True)
    loss = losses.codebook_diversity_loss(xd, cd, _metric(metric), T, lambda: torch.arange(x.shape[1], device="cuda") % n, n,
                                          pos_div=1)
    (loss * G_LOSS).backward()
    torch.cuda.synchronize()
    return loss.detach().reshape(1), xd.grad, cd.grad


@pytest.mark.parametrize("metric", METRICS)
def test_loss_function_with_learnable_codes(monkeypatch, metric):
    """losses.codebook_diversity_loss with codes that require grad, fused (the similarity matrix is never asked for) and
    chunked (VQ_DIVERSITY_NO_FUSED=1): loss, x.grad and c.grad of each path against the fp64 closed form."""
    from vector_quantization import search

    name, T = "c33", 1.0
    (h, b, n, k, d), _ = SHAPES[name]
    x, c, ref64, ref32 = _case(name, metric, T)
    monkeypatch.setenv("VQ_DIVERSITY_NO_FUSED", "1")
    chunked = _loss_step(x, c, metric, T, n)
    monkeypatch.delenv("VQ_DIVERSITY_NO_FUSED")

    def no_matrix(*a, **k):
        raise AssertionError("the [M, K] similarity matrix was asked for")

    monkeypatch.setattr(search._NativeBackend, "similarities", staticmethod(no_matrix))
    fused = _loss_step(x, c, metric, T, n)
    for path, (loss, gx, gc_) in (("chunked", chunked), ("fused", fused)):
        _rule(f"{name} {metric} {path}", "loss", loss, ref64["loss"].reshape(1), ref32["loss"].reshape(1))
        _rule(f"{name} {metric} {path}", "x.grad", gx, ref64["gx"], ref32["gx"])
        _rule(f"{name} {metric} {path}", "c.grad", gc_, ref64["gc"], ref32["gc"])
    # only the codes need a gradient: the rows' sweep is skipped, c.grad is the same sweep's result
    loss, gx, gc_ = _loss_step(x, c, metric, T, n, x_grad=False)
    assert gx is None
    assert torch.equal(gc_, fused[2]) and torch.equal(loss, fused[0])


# ------------------------------------------------------------------------------------------------ module level
def _module(variant):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    kw, head_dim = dict(codebook_diversity_loss_weight=0.5), 64
    if variant == "shared_heads":
        kw.update(heads=2, codebook_dim=32)
        head_dim = 32
    elif variant == "separate_heads":
        kw.update(heads=2, codebook_dim=32, separate_codebook_per_head=True)
        head_dim = 32
    elif variant == "orthogonal":
        kw.update(orthogonal_reg_weight=1.0)
    torch.manual_seed(17)
    params = CodebookParams(dim=head_dim, codebook_size=256, learnable_codebook=True, ema_update=False)
    return vq.VectorQuantize(dim=64, codebook_params=params, **kw).cuda().train()


def _step(monkeypatch, mod, x):
    """One training step -> the module's loss, x.grad, the codebook's grad and, recorded at the call of the diversity loss,
    its inputs and the gradients it sent back to its rows and to its codes (both are handed on as views of themselves,
    whose hooks see that gradient alone)."""
    from vector_quantization import losses

    seen = {}
    original = losses.codebook_diversity_loss

    def recording(rows, codes, metric, temperature, position, n_positions, live_codes=None, **kw):
        rows_alias, codes_alias = rows.view_as(rows), codes.view_as(codes)
        rows_alias.register_hook(lambda g: seen.__setitem__("gx", g.detach().clone()))
        codes_alias.register_hook(lambda g: seen.__setitem__("gc", g.detach().clone()))
        seen.update(x=rows.detach().clone(), c=codes.detach().clone(), metric=metric, T=temperature, n=n_positions, live=live_codes,
                    pos_div=kw.get("pos_div"))
        return original(rows_alias, codes_alias, metric, temperature, position, n_positions, live_codes, **kw)

    monkeypatch.setattr(losses, "codebook_diversity_loss", recording)
    torch.manual_seed(29)
    xd = x.clone().requires_grad_(True)
    _, _, loss, parts = mod(xd, return_loss_breakdown=True)
    loss.sum().backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(losses, "codebook_diversity_loss", original)
    return dict(loss=loss.detach().sum().reshape(1), div=parts.codebook_diversity.detach().reshape(1), gx=xd.grad,
                gcb=mod._codebook.embeddings.grad.detach().clone(), seen=seen)


# seeds of x for which no fp64 A entry of the recorded call is within 2 % of the clamp
X_SEEDS = {"plain": 23, "separate_heads": 23, "shared_heads": 23, "orthogonal": 23}


@pytest.mark.parametrize("variant", list(X_SEEDS))
def test_learnable_module_trains_without_the_similarity_matrix(monkeypatch, variant):
    """VectorQuantize(dim=64, K=256, learnable_codebook=True, ema_update=False, codebook_diversity_loss_weight=0.5) in train
    mode, x [32, 16, 64]: forward + backward with the backend's `similarities` raising, against the same step of a deep copy
    on the chunked path (VQ_DIVERSITY_NO_FUSED=1).  The rule of test_module_trains_without_the_similarity_matrix: the fp64
    closed form of the recorded call is the reference, the chunked path (the reference's fp32 op sequence on this device)
    measures its own error against it, and the fused path may be 4 x that far off (floors GRAD_ATOL_OF_MAX, GRAD_RTOL)."""
    from vector_quantization import search

    fused_mod = _module(variant)
    chunk_mod = copy.deepcopy(fused_mod)
    x = torch.randn((32, 16, 64), generator=torch.Generator().manual_seed(X_SEEDS[variant])).cuda()

    monkeypatch.setenv("VQ_DIVERSITY_NO_FUSED", "1")
    want = _step(monkeypatch, chunk_mod, x)
    monkeypatch.delenv("VQ_DIVERSITY_NO_FUSED")

    def no_matrix(*a, **k):
        raise AssertionError("the [M, K] similarity matrix was asked for")

    monkeypatch.setattr(search._NativeBackend, "similarities", staticmethod(no_matrix))
    got = _step(monkeypatch, fused_mod, x)

    seen = got["seen"]
    assert torch.equal(seen["x"], want["seen"]["x"]) and torch.equal(seen["c"], want["seen"]["c"])
    assert seen["live"] is None, "a learnable codebook without EMA is not rewritten before backward"
    h, m, _ = seen["x"].shape
    assert h * m // seen["n"] == 32 * (2 if variant in ("shared_heads", "separate_heads") else 1)
    ref64 = codes_gradient64(seen["x"].cpu(), seen["c"].cpu(), seen["T"], seen["n"], seen["pos_div"], seen["metric"] == search.DOT,
                             g_loss=0.5)
    margin = clamp_margin(ref64["A"])
    assert margin > 0.02, f"an fp64 A entry lies within {margin:.2%} of the clamp; pick another seed in X_SEEDS"
    loss_err = abs(float(want["div"]) - float(ref64["loss"])) / abs(float(ref64["loss"]))
    assert_grad_close(got["div"], ref64["loss"].reshape(1), f"{variant} diversity loss", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * loss_err))
    errs = {}
    for key, what in (("gx", "d loss / d rows"), ("gc", "d loss / d codes")):
        scale = float(ref64[key].abs().max())
        errs[key] = float((want["seen"][key].double().cpu() - ref64[key]).abs().max()) / scale
        print(f"{variant}: the chunked path's {what} is {errs[key]:.2e} of the largest entry off fp64")
        assert_grad_close(seen[key], ref64[key], f"{variant} {what}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * errs[key]))
    # the module's outputs: everything but the diversity term is the same computation on both paths
    assert_grad_close(got["loss"], want["loss"], f"{variant} loss", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * loss_err))
    for key, out in (("gx", "gx"), ("gc", "gcb")):
        share = float(ref64[key].abs().max()) / float(want[out].abs().max())
        assert_grad_close(got[out], want[out], f"{variant} module {out}", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * errs[key] * share))


# ------------------------------------------------------------------------------------------------ memory
def test_peak_memory_stays_below_one_similarity_matrix():
    """[64, 256, 64] with K = 4096 and a learnable codebook, fused: forward + backward never allocate as much as ONE [M, K]
    fp32 matrix (256 MiB)."""
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    gc.collect()
    torch.cuda.synchronize()
    foreign = torch.cuda.memory_allocated()  # what earlier tests of the process still hold: not this step's
    torch.manual_seed(3)
    params = CodebookParams(dim=64, codebook_size=4096, learnable_codebook=True, ema_update=False)
    mod = vq.VectorQuantize(dim=64, codebook_params=params, codebook_diversity_loss_weight=0.5).cuda().train()
    x = torch.randn((64, 256, 64), device="cuda", requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    _, _, loss = mod(x)
    loss.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - foreign
    m, k = 64 * 256, 4096
    print(f"peak {peak / 2**20:.1f} MiB (beside {foreign / 2**20:.1f} MiB held by earlier tests); one [M, K] matrix: {m * k * 4 / 2**20:.0f} MiB")
    assert peak < m * k * 4
    grad = mod._codebook.embeddings.grad
    assert x.grad is not None and grad is not None and bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(grad).all())
