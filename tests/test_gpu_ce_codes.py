"""GPU suite of the cross-entropy loss's fused gradient with respect to a learnable codebook (vq_ce_backward_codes_f32, the
kCeC role of the sweep; losses._CrossEntropyFn with codes that require grad) against the fp64 closed form of
tests/ce_codes_run.py on the CPU.

The tolerance is the project's rule (tests/test_gpu_diversity_codes.py::_rule): assert_grad_close with
atol = max(GRAD_ATOL_OF_MAX, 4 x the error the reference's own fp32 op sequence has on the same inputs against fp64) of the
largest fp64 entry, and GRAD_RTOL.  Every measured reference error and kernel error is printed.

The table of native calls (tests/native_cases.py) holds one case per launch path (one row split, several), so that the poison
suites cover the call.  grad_codes is written completely: it needs no extent sentence."""
from __future__ import annotations

import copy
import functools
import gc

import pytest
import torch

from ce_codes_cases import CE_CODES_CASES
from ce_codes_run import check_fixture, closed_form, reference_sequence
from gumbel_run import GRAD_ATOL_OF_MAX, GRAD_RTOL, assert_grad_close  # noqa: F401  (GRAD_RTOL: assert_grad_close's default)
from test_ce_codes_host import documented_floats

pytestmark = pytest.mark.gpu

G_LOSS = 0.7  # upstream gradient of the loss
METRICS = ("euclid", "dot")

# name -> (H, M, K, D)
SHAPES = {
    "m33": (1, 33, 301, 100),     # one real row in a second sub-tile
    "m5": (1, 5, 40, 16),
    "m1": (1, 1, 7, 5),
    "k1": (1, 24, 1, 8),          # one code: the fp64 gradient is exactly 0
    "k7": (1, 80, 7, 24),
    "k1000": (1, 72, 1000, 128),  # a partial last block of codes
    "dp256": (1, 96, 512, 256),
    "heads2": (2, 64, 130, 32),
    "splits": (1, 2100, 64, 32),  # nine staged tiles, one workgroup column
}


def _metric(metric):
    from vector_quantization import search

    return search.DOT if metric == "dot" else search.EUCLID


def _inputs(name, metric, seed=1):
    """x [H, M, D], c [H, K, D] and targets: the argmax of the similarities for every other row, a random code for the rest."""
    h, m, k, d = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * seed + len(name) + (7 if metric == "dot" else 0))
    scale = 1.0 / max(1.0, d ** 0.5) if metric == "dot" else 1.0  # (dot logits of unit variance)
    x, c = torch.randn((h, m, d), generator=g) * scale ** 0.5, torch.randn((h, k, d), generator=g) * scale ** 0.5
    s = x.double() @ c.double().transpose(-1, -2) if metric == "dot" else -torch.cdist(x.double(), c.double())
    target = s.argmax(-1)
    rnd = torch.randint(0, k, (h, m), generator=g)
    target[:, 1::2] = rnd[:, 1::2]
    return x, c, target


@functools.lru_cache(maxsize=None)
def _case(name, metric):
    """(x, c, target, coef, fp64 closed form, the reference's fp32 sequence) on the CPU, computed once and left unchanged."""
    x, c, target = _inputs(name, metric)
    coef = G_LOSS / target.numel()
    ref64 = closed_form(x, c, target, metric == "dot", coef=coef)
    ref32 = reference_sequence(x, c, target, metric == "dot", coef=coef)
    return x, c, target, coef, ref64, ref32


def _native(x, c, target, coef, mt, xd=None, td=None, gc_out=None):
    """softmax_stats (the forward's sweep), then the codes sweep -> gc [H, K, D] on the GPU."""
    from vector_quantization import native

    xd = x.cuda() if xd is None else xd
    td = target.cuda() if td is None else td
    cd = c.cuda()
    lse, _ = native.softmax_stats(xd, cd, metric=mt, scale=1.0, target=td)
    out = native.ce_backward_codes(xd, cd, lse, td, torch.tensor([coef], dtype=torch.float32, device="cuda"), metric=mt, out=gc_out)
    torch.cuda.synchronize()
    return out


def _rule(case_name, what, have, want, r32):
    """assert_grad_close under the rule of the module docstring; prints the reference's error and the kernel's."""
    want = torch.as_tensor(want).detach().double().cpu()
    have = torch.as_tensor(have).detach().double().cpu().reshape(want.shape)
    r32 = torch.as_tensor(r32).detach().double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(have).all()), (case_name, what)
    ref_err = float((r32 - want).abs().max() / max(float(want.abs().max()), 1e-300))
    print(f"{case_name} {what}: the reference's fp32 sequence is {ref_err:.2e} of the largest entry off fp64")
    assert_grad_close(have, want, f"{case_name} {what}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * ref_err))


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_grad_codes_against_fp64(name, metric):
    h, m, k, d = SHAPES[name]
    x, c, target, coef, ref64, ref32 = _case(name, metric)
    got = _native(x, c, target, coef, _metric(metric))
    assert tuple(got.shape) == (h, k, d)
    _rule(f"{name} {metric}", "gc", got, ref64["gc"], ref32["gc"])
    if name == "k1":
        assert float(ref64["gc"].abs().max()) == 0.0, "one code: the fp64 gradient is exactly 0"


def test_row_splits_cover_several_workgroups():
    """The `splits` shape really runs more than one blockIdx.z, and the sizer holds one partial [H, K, D] per split."""
    from vector_quantization import native

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    h, m, k, d = SHAPES["splits"]
    floats, splits = documented_floats(h, m, k, d, cus)
    assert splits >= 2, splits
    one_split, _ = documented_floats(h, m, k, d, 1)  # (one CU to fill: the image, the targets and the lse alone)
    assert floats == one_split + splits * h * k * d
    assert native.load().vq_ce_codes_workspace_bytes(h, m, k, d) == 4 * floats
    for name in ("m33", "heads2", "dp256"):
        hh, mm, kk, dd = SHAPES[name]
        assert native.load().vq_ce_codes_workspace_bytes(hh, mm, kk, dd) == 4 * documented_floats(hh, mm, kk, dd, cus)[0], name


@pytest.mark.parametrize("metric", METRICS)
def test_ignored_rows_are_never_read(metric):
    """Targets of -1, K, K + 5 and 2^32 + 3 with x rows of NaN and +-inf: the result is the fp64 form over the valid rows."""
    name = "m33"
    h, m, k, d = SHAPES[name]
    x, c, target, _, _, _ = _case(name, metric)
    x, target = x.clone(), target.clone()
    bad = {0: -1, 3: k, 7: k + 5, 32: 2 ** 32 + 3, 12: -1}
    fills = (float("nan"), float("inf"), float("-inf"))
    for i, (row, t) in enumerate(bad.items()):
        target[0, row] = t
        x[0, row] = fills[i % 3]
    x[0, 12, 1] = float("-inf")  # +inf and -inf in one row
    coef = G_LOSS / (m - len(bad))
    ref64 = closed_form(x, c, target, metric == "dot", coef=coef)
    ref32 = reference_sequence(x, c, target, metric == "dot", coef=coef)
    assert ref64["count"] == m - len(bad)
    got = _native(x, c, target, coef, _metric(metric))
    _rule(f"{name} {metric} ignored rows", "gc", got, ref64["gc"], ref32["gc"])
    # every row ignored, a finite coef: exactly zero
    target[:] = -1
    target[0, 1::3] = k
    got = _native(x, c, target, 0.25, _metric(metric))
    assert not bool(got.any()), "every row ignored: grad_codes is exactly zero"


def test_rows_that_coincide_with_codes():
    """Euclid, rows bit-equal to codes (s == 0: ATen's subgradient 0), as the row's target and not."""
    name = "k7"
    h, m, k, d = SHAPES[name]
    x, c, target, coef, _, _ = _case(name, "euclid")
    x, target = x.clone(), target.clone()
    x[0, 2], target[0, 2] = c[0, 3], 3   # the target itself
    x[0, 5], target[0, 5] = c[0, 6], 1   # another code
    x[0, 40], target[0, 40] = c[0, 0], 0
    x[0, 79], target[0, 79] = c[0, 4], 5
    ref64 = closed_form(x, c, target, False, coef=coef)
    ref32 = reference_sequence(x, c, target, False, coef=coef)
    got = _native(x, c, target, coef, _metric("euclid"))
    _rule(f"{name} euclid coincidence", "gc", got, ref64["gc"], ref32["gc"])


@pytest.mark.parametrize("metric", METRICS)
def test_strided_x_rows_and_targets(metric):
    """x rows inside wider NaN-filled buffers (row stride D + 12, a 16-byte multiple, and D + 3: the scalar row loads) and the
    targets as a strided view give the same result: nothing between the rows is read."""
    name = "m33"
    h, m, k, d = SHAPES[name]
    x, c, target, coef, ref64, ref32 = _case(name, metric)
    tbuf = torch.full((h, m, 3), 2 ** 32 + 3, dtype=torch.int64, device="cuda")
    tbuf[..., 1] = target.cuda()
    for pad in (12, 3):
        xbuf = torch.full((h, m, d + pad), float("nan"), device="cuda")
        xbuf[..., :d] = x.cuda()
        got = _native(x, c, target, coef, _metric(metric), xd=xbuf[..., :d], td=tbuf[..., 1])
        _rule(f"{name} {metric} strided +{pad}", "gc", got, ref64["gc"], ref32["gc"])


@pytest.mark.parametrize("name", ["m33", "heads2", "splits", "k7"])
def test_nothing_outside_grad_codes_is_written(name):
    h, m, k, d = SHAPES[name]
    x, c, target, coef, ref64, ref32 = _case(name, "euclid")
    guard, size = 1024, h * k * d
    buf = torch.full((size + 2 * guard,), 7.0, device="cuda")
    out = buf[guard:guard + size].view(h, k, d)
    got = _native(x, c, target, coef, _metric("euclid"), gc_out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + size:] == 7.0).all()), "grad_codes wrote outside [H, K, D]"
    _rule(f"{name} guarded", "gc", got, ref64["gc"], ref32["gc"])


@pytest.mark.parametrize("name", ["splits", "heads2"])
def test_two_runs_are_bit_identical(name):
    x, c, target, coef, _, _ = _case(name, "euclid")
    first = _native(x, c, target, coef, _metric("euclid"))
    second = _native(x, c, target, coef, _metric("euclid"))
    assert torch.equal(first, second)


def test_no_rows_clears_grad_codes():
    from vector_quantization import native

    h, k, d = 2, 40, 24
    x = torch.empty((h, 0, d), device="cuda")
    cb = torch.randn((h, k, d), device="cuda")
    lse = torch.empty((h, 0), device="cuda")
    target = torch.empty((h, 0), dtype=torch.int64, device="cuda")
    out = torch.full((h, k, d), 7.0, device="cuda")
    got = native.ce_backward_codes(x, cb, lse, target, torch.ones(1, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and not bool(out.any())


# ------------------------------------------------------------------------------------------------ the loss function
def _loss_step(x, c, target, metric, x_grad=True):
    from vector_quantization import losses

    xd = x.cuda().requires_grad_(x_grad)
    cd = c.cuda().requires_grad_(True)
    loss = losses.cross_entropy_to_codes(xd, cd, target.cuda(), _metric(metric))
    (loss * G_LOSS).backward()
    torch.cuda.synchronize()
    return loss.detach().reshape(1), xd.grad, cd.grad


def _no_matrix(*a, **k):
    raise AssertionError("the [M, K] similarity matrix was asked for")


def _fused_at_every_row_count(monkeypatch):
    """The dispatch cut (losses.CE_CODES_FUSED_MIN_ROWS) is a measured speed rule; a test of the fused path's numbers at a
    shape below it lowers every entry to 1 row, as tools/ce_codes_bench.py --codes-min-rows 1 does."""
    from vector_quantization import losses

    monkeypatch.setattr(losses, "CE_CODES_FUSED_MIN_ROWS", {dp: 1 for dp in losses.CE_CODES_FUSED_MIN_ROWS})


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["m33", "splits"])
def test_loss_function_with_learnable_codes(monkeypatch, name, metric):
    """losses.cross_entropy_to_codes with codes that require grad, fused (the similarity matrix is never asked for) and
    chunked (VQ_CE_CODES_NO_FUSED=1): loss, x.grad and c.grad of each path against the fp64 closed form.  `splits` (2100 rows
    of 32 dims) lies above the dispatch cut as it is; `m33` (33 rows of 100 dims) below it."""
    from vector_quantization import losses, search

    h, m, _, d = SHAPES[name]
    if name == "m33":
        assert not losses.ce_codes_runs_fused(m, d)
        _fused_at_every_row_count(monkeypatch)
    assert losses.ce_codes_runs_fused(m, d)
    x, c, target, _, _, _ = _case(name, metric)
    target = target.clone()
    target[0, ::6] = -1
    ref64 = closed_form(x, c, target, metric == "dot", g_loss=G_LOSS)
    ref32 = reference_sequence(x, c, target, metric == "dot", g_loss=G_LOSS)
    monkeypatch.setenv("VQ_CE_CODES_NO_FUSED", "1")
    chunked = _loss_step(x, c, target, metric)
    monkeypatch.delenv("VQ_CE_CODES_NO_FUSED")
    monkeypatch.setattr(search._NativeBackend, "similarities", staticmethod(_no_matrix))
    fused = _loss_step(x, c, target, metric)
    for path, (loss, gx, gc_) in (("chunked", chunked), ("fused", fused)):
        _rule(f"{name} {metric} {path}", "loss", loss, ref64["loss"].reshape(1), ref32["loss"].reshape(1))
        _rule(f"{name} {metric} {path}", "x.grad", gx, ref64["gx"], ref32["gx"])
        _rule(f"{name} {metric} {path}", "c.grad", gc_, ref64["gc"], ref32["gc"])
    # only the codes need a gradient: the rows' sweep is skipped, c.grad is the same sweep's result
    loss, gx, gc_ = _loss_step(x, c, target, metric, x_grad=False)
    assert gx is None
    assert torch.equal(gc_, fused[2]) and torch.equal(loss, fused[0])


# ------------------------------------------------------------------------------------------------ module level
@pytest.mark.parametrize("name", list(CE_CODES_CASES))
def test_reference_fixture_through_the_module(monkeypatch, name):
    """Every fixture through VectorQuantize on the GPU with the backend's `similarities` raising: indices exact, loss and both
    gradients under assert_grad_close against what the reference recorded."""
    from vector_quantization import search

    _fused_at_every_row_count(monkeypatch)  # (commit_mask has 120 rows of 64 dims: below the cut of that width)
    monkeypatch.setattr(search._NativeBackend, "similarities", staticmethod(_no_matrix))
    check_fixture(name, "cuda")


def _module(variant, **cb_kw):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    kw, head_dim = dict(commitment_use_cross_entropy_loss=True), 64
    if variant == "shared_heads":
        kw.update(heads=2, codebook_dim=32)
        head_dim = 32
    elif variant == "separate_heads":
        kw.update(heads=2, codebook_dim=32, separate_codebook_per_head=True)
        head_dim = 32
    elif variant in ("orthogonal", "ema_orthogonal"):
        kw.update(orthogonal_reg_weight=1.0)
    torch.manual_seed(17)
    learn = dict(ema_update=True, threshold_ema_dead_code=0) if variant == "ema_orthogonal" else dict(learnable_codebook=True, ema_update=False)
    params = CodebookParams(dim=head_dim, codebook_size=256, **learn)
    return vq.VectorQuantize(dim=64, codebook_params=params, **kw).cuda().train()


def _step(monkeypatch, mod, x):
    """One training step -> the module's loss, indices, x.grad, the codebook's grad and, recorded at the call of the cross
    entropy, its inputs and the gradients it sent back to its rows and to its codes (both are handed on as views of
    themselves, whose hooks see that gradient alone)."""
    from vector_quantization import losses

    seen = {}
    original = losses.cross_entropy_to_codes

    def recording(rows, codes, target, metric, live_codes=None, **kw):
        rows_alias, codes_alias = rows.view_as(rows), codes.view_as(codes)
        rows_alias.register_hook(lambda g: seen.__setitem__("gx", g.detach().clone()))
        codes_alias.register_hook(lambda g: seen.__setitem__("gc", g.detach().clone()))
        seen.update(x=rows.detach().clone(), c=codes.detach().clone(), target=target.detach().clone(), metric=metric, live=live_codes)
        return original(rows_alias, codes_alias, target, metric, live_codes, **kw)

    monkeypatch.setattr(losses, "cross_entropy_to_codes", recording)
    xd = x.clone().requires_grad_(True)
    _, ind, loss, parts = mod(xd, return_loss_breakdown=True)
    loss.sum().backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(losses, "cross_entropy_to_codes", original)
    return dict(loss=loss.detach().sum().reshape(1), ce=parts.commitment.detach().reshape(1), ind=ind, gx=xd.grad,
                gcb=mod._codebook.embeddings.grad.detach().clone(), seen=seen)


@pytest.mark.parametrize("variant", ["plain", "separate_heads", "shared_heads", "orthogonal"])
def test_learnable_module_trains_without_the_similarity_matrix(monkeypatch, variant):
    """VectorQuantize(dim=64, K=256, learnable_codebook=True, ema_update=False, commitment_use_cross_entropy_loss=True) in train
    mode, x [32, 16, 64]: forward + backward with the backend's `similarities` raising, against the same step of a deep copy
    on the switched-off path (VQ_CE_CODES_NO_FUSED=1).  The rule of tests/test_gpu_diversity_codes.py: the fp64 closed form of
    the recorded call is the reference, the chunked path (the reference's fp32 op sequence on this device) measures its own
    error against it, and the fused path may be 4 x that far off (floors GRAD_ATOL_OF_MAX, GRAD_RTOL)."""
    from vector_quantization import search

    fused_mod = _module(variant)
    chunk_mod = copy.deepcopy(fused_mod)
    x = torch.randn((32, 16, 64), generator=torch.Generator().manual_seed(23)).cuda()  # (512 rows, or 2 x 512 / 1024 of 32 dims: above the cut)
    monkeypatch.setenv("VQ_CE_CODES_NO_FUSED", "1")
    want = _step(monkeypatch, chunk_mod, x)
    monkeypatch.delenv("VQ_CE_CODES_NO_FUSED")
    monkeypatch.setattr(search._NativeBackend, "similarities", staticmethod(_no_matrix))
    got = _step(monkeypatch, fused_mod, x)

    seen = got["seen"]
    assert torch.equal(seen["x"], want["seen"]["x"]) and torch.equal(seen["c"], want["seen"]["c"])
    assert torch.equal(seen["target"], want["seen"]["target"]) and torch.equal(got["ind"], want["ind"])
    assert seen["live"] is None, "a learnable codebook without EMA is not rewritten before backward"
    ref64 = closed_form(seen["x"].cpu(), seen["c"].cpu(), seen["target"].cpu(), seen["metric"] == search.DOT)
    loss_err = abs(float(want["ce"]) - float(ref64["loss"])) / abs(float(ref64["loss"]))
    assert_grad_close(got["ce"], ref64["loss"].reshape(1), f"{variant} cross entropy", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * loss_err))
    errs = {}
    for key, what in (("gx", "d loss / d rows"), ("gc", "d loss / d codes")):
        scale = float(ref64[key].abs().max())
        errs[key] = float((want["seen"][key].double().cpu() - ref64[key]).abs().max()) / scale
        print(f"{variant}: the chunked path's {what} is {errs[key]:.2e} of the largest entry off fp64")
        assert_grad_close(seen[key], ref64[key], f"{variant} {what}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * errs[key]))
    # the module's outputs: everything but the cross-entropy term is the same computation on both paths
    assert_grad_close(got["loss"], want["loss"], f"{variant} loss", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * loss_err))
    for key, out in (("gx", "gx"), ("gc", "gcb")):
        share = float(ref64[key].abs().max()) / float(want[out].abs().max())
        assert_grad_close(got[out], want[out], f"{variant} module {out}", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * errs[key] * share))


def test_ema_codebook_with_the_orthogonal_loss_keeps_the_chunks(monkeypatch):
    """An EMA codebook that learns through the orthogonal loss: its codes require grad AND are rewritten before backward
    (live codes).  That call stays on the chunked path -- it asks for the matrix."""
    from vector_quantization import search

    mod = _module("ema_orthogonal")
    x = torch.randn((32, 16, 64), generator=torch.Generator().manual_seed(23)).cuda()
    asked = []
    original = search._NativeBackend.similarities

    def recording(*a, **k):
        asked.append(1)
        return original(*a, **k)

    monkeypatch.setattr(search._NativeBackend, "similarities", staticmethod(recording))
    res = _step(monkeypatch, mod, x)
    assert res["seen"]["live"] is not None and res["seen"]["c"].requires_grad is False
    assert asked, "live codes that require grad run on the chunks"
    assert bool(torch.isfinite(res["gx"]).all()) and bool(torch.isfinite(res["gcb"]).all())


# ------------------------------------------------------------------------------------------------ memory
def test_peak_memory_stays_below_one_similarity_matrix(monkeypatch):
    """[64, 256, 64] with K = 4096, a learnable codebook and the cross-entropy commitment loss, fused: forward + backward never
    allocate as much as ONE [M, K] fp32 matrix (256 MiB).  (By the documented plan the workspace is 4.3 MiB of image, 128 KiB
    of targets and lse and 8 partials of 1 MiB.)"""
    import vector_quantization as vq
    from vector_quantization import search
    from vector_quantization.codebooks import CodebookParams

    monkeypatch.setattr(search._NativeBackend, "similarities", staticmethod(_no_matrix))
    gc.collect()
    torch.cuda.synchronize()
    foreign = torch.cuda.memory_allocated()  # what earlier tests of the process still hold: not this step's
    torch.manual_seed(3)
    params = CodebookParams(dim=64, codebook_size=4096, learnable_codebook=True, ema_update=False)
    mod = vq.VectorQuantize(dim=64, codebook_params=params, commitment_use_cross_entropy_loss=True).cuda().train()
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
