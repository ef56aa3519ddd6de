"""GPU suite of the fused codebook diversity loss (vq_diversity_stats_f32, vq_diversity_accumulate_f32, vq_diversity_delta_f32,
vq_diversity_backward_x_f32, losses._DiversityFn) against the fp64 closed form of tests/diversity_run.py on the CPU.

Tolerances are the project's rules (tests/test_gpu_reinmax.py, tests/gumbel_run.py); the margin is 4 x the error the
reference's own fp32 op sequence has on the same inputs, because the kernels may legitimately reorder sums:
* loss, delta, gx: assert_grad_close with atol = max(GRAD_ATOL_OF_MAX, 4 x that error) of the largest fp64 entry, GRAD_RTOL;
* lse: the LSE_ATOL / LSE_RTOL rule;
* A: entry by entry and RELATIVE, |got - want| <= max(GRAD_RTOL, 4 x the fp32 sequence's worst relative error) x want + FLT_MIN
  (the smallest normal fp32: what no fp32 sum of fp32 terms resolves) -- a tolerance scaled by the largest entry would hide
  a padding row counted into a small entry.
The mask [A >= 1e-5] of the gradient is discontinuous: every case asserts, on the CPU, that no fp64 entry of A lies within
2 % of 1e-5 for its seed (SEEDS: chosen on the CPU for exactly that), so kernel and reference are on the same side everywhere.
Every measured reference error and kernel error is printed."""
from __future__ import annotations

import copy
import functools
import gc

import pytest
import torch

from diversity_run import CLAMP, clamp_margin, closed_form64, make_inputs, positions, reference_sequence
from gumbel_run import GRAD_ATOL_OF_MAX, GRAD_RTOL, assert_grad_close

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
LSE_ATOL, LSE_RTOL = 2e-5, 2e-6
FLT_MIN = 1.1754943508222875e-38
G_LOSS = 0.7  # upstream gradient of the loss
TEMPERATURES = (1.0, 100.0)
METRICS = ("euclid", "dot")

# name -> ((H, B, N, K, D), pos_div): rows per head M = B * N * pos_div, Ch = B * pos_div rows of a head per position
SHAPES = {
    "c32": ((1, 32, 3, 256, 64), 1),          # Ch a multiple of 32
    "c33": ((1, 33, 2, 301, 100), 1),         # one row into a second sub-tile
    "c5": ((1, 5, 7, 40, 16), 1),
    "c1": ((1, 1, 40, 7, 5), 1),
    "n1": ((1, 70, 1, 520, 64), 1),
    "k1": ((1, 8, 3, 1, 8), 1),               # below one tile of codes
    "k7": ((1, 40, 2, 7, 24), 1),
    "k1000": ((1, 8, 9, 1000, 128), 1),       # a partial last tile
    "dp256": ((1, 32, 3, 512, 256), 1),
    "heads2": ((2, 16, 4, 130, 32), 1),       # separate codebooks, summed into one A
    "shared2": ((1, 6, 5, 90, 40), 2),        # two heads of one codebook interleaved in the rows
    "splits": ((1, 2, 70, 64, 32), 1),        # one workgroup column: the positions split over blockIdx.z inside one staged tile
    "splits_spp2": ((1, 40, 6, 64, 64), 1),   # split positions of two sub-tiles each
}
# seeds for which no fp64 A entry is within 2 % of the clamp (searched on the CPU from 1 upwards; 1 unless listed)
SEEDS = {("c33", "euclid", 100.0): 2, ("c33", "dot", 100.0): 2, ("c1", "euclid", 100.0): 2, ("n1", "dot", 100.0): 2,
         ("k1000", "dot", 100.0): 5, ("dp256", "euclid", 100.0): 3, ("dp256", "dot", 100.0): 4, ("heads2", "dot", 100.0): 2,
         ("shared2", "dot", 100.0): 2, ("splits", "euclid", 100.0): 2, ("splits", "dot", 100.0): 8,
         ("splits_spp2", "dot", 100.0): 6}


def _seed(name, metric, T):
    return SEEDS.get((name, metric, T), 1)


def _metric(metric):
    from vector_quantization import search

    return search.DOT if metric == "dot" else search.EUCLID


@functools.lru_cache(maxsize=None)
def _case(name, metric, T, live=False):
    """(x, c, live codes | None, fp64 closed form, fp32 references) on the CPU, computed once and left unchanged."""
    (h, b, n, k, d), pos_div = SHAPES[name]
    dot = metric == "dot"
    x, c = make_inputs(h, b, n, k, d, dot, _seed(name, metric, T), pos_div)
    lv = c + 0.05 * torch.randn(c.shape, generator=torch.Generator().manual_seed(99)) if live else None
    ref64 = closed_form64(x, c, T, n, pos_div, dot, live=lv, g_loss=G_LOSS)
    margin = clamp_margin(ref64["A"])
    assert margin > 0.02, f"{name} {metric} T={T}: an fp64 A entry lies within {margin:.2%} of the clamp; pick another seed"
    ref32 = reference_sequence(x, c, T, n, pos_div, dot, dtype=torch.float32, live=lv, g_loss=G_LOSS)
    ref32["delta"] = closed_form64(x, c, T, n, pos_div, dot, live=lv, g_loss=G_LOSS, dtype=torch.float32)["delta"]
    return x, c, lv, ref64, ref32


def _native(x, c, T, n, pos_div, mt, live=None, xd=None, gx_out=None):
    """The four sweeps and the [N, K] tensor ops between them -> dict(lse, A, loss, delta, gx) on the GPU."""
    from vector_quantization import losses, native

    xd = x.cuda() if xd is None else xd
    cd = c.cuda()
    h, m, _ = x.shape
    k = c.shape[1]
    packed = native.pack_codebooks(cd, mt)
    lse2 = native.diversity_stats(xd, cd, metric=mt, temperature=T, packed=packed)
    table = native.diversity_accumulate(xd, cd, lse2, metric=mt, temperature=T, n_positions=n, pos_div=pos_div)
    A = table[:, :k]
    assert not bool(table[:, k:].any()), "the padding of A past K is written as 0"
    loss = -(-A * A.clamp(min=CLAMP).log()).sum(-1).sum() / n
    # (the host hands every row of U to the sweeps minus its mean: delta and U as the formulas define them are those plus the shift)
    U, centre = losses.diversity_upstream(table, G_LOSS, n, h * m // n, k)
    kw = dict(metric=mt, temperature=T, n_positions=n, pos_div=pos_div, packed=packed)
    delta = native.diversity_delta(xd, cd, lse2, U, **kw)
    gx = native.diversity_backward_x(xd, cd, lse2, delta, U, live=None if live is None else live.cuda(), out=gx_out, **kw)
    torch.cuda.synchronize()
    pos = positions(m, n, pos_div).cuda()
    return dict(lse=lse2[:, :m].double() / LOG2E, A=A, loss=loss.reshape(1), delta=delta[:, :m].double() + centre.double()[pos], gx=gx,
                U=U[:, :k].double() + centre.double()[:, None])


def _compare(case, got, ref64, ref32, names=("lse", "A", "loss", "delta", "gx")):
    for name in names:
        want = torch.as_tensor(ref64[name]).detach().double().cpu().reshape(got[name].shape)
        r32 = torch.as_tensor(ref32[name]).detach().double().cpu().reshape(got[name].shape)
        have = got[name].detach().double().cpu()
        assert bool(torch.isfinite(have).all()), (case, name)
        if name == "lse":
            ref_err = float((r32 - want).abs().max())
            atol = max(LSE_ATOL, 4 * ref_err)
            err = (have - want).abs()
            print(f"{case} lse: the reference's fp32 sequence is {ref_err:.3e} off fp64 | kernel max err {float(err.max()):.3e} "
                  f"(atol {atol:.3e})")
            assert float((err - LSE_RTOL * want.abs()).max()) <= atol, (case, name, float(err.max()), atol)
        elif name == "A":
            ref_rel = float((((r32 - want).abs() - FLT_MIN).clamp(min=0) / want).max())
            rtol = max(GRAD_RTOL, 4 * ref_rel)
            rel = ((have - want).abs() - FLT_MIN).clamp(min=0) / want
            print(f"{case} A: the reference's fp32 sequence is {ref_rel:.2e} (worst relative) off fp64 | kernel worst relative "
                  f"err {float(rel.max()):.3e} (rtol {rtol:.3e})")
            assert float(((have - want).abs() - rtol * want).max()) <= FLT_MIN, (case, name, float(rel.max()), rtol)
        else:
            ref_err = float((r32 - want).abs().max() / max(float(want.abs().max()), 1e-300))
            print(f"{case} {name}: the reference's fp32 sequence is {ref_err:.2e} of the largest entry off fp64")
            assert_grad_close(have, want, f"{case} {name}", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * ref_err))


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("T", TEMPERATURES, ids=lambda t: f"T{t:g}")
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_output_against_fp64(name, metric, T):
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, _, ref64, ref32 = _case(name, metric, T)
    got = _native(x, c, T, n, pos_div, _metric(metric))
    _compare(f"{name} {metric} T={T:g}", got, ref64, ref32)


@pytest.mark.parametrize("metric", METRICS)
def test_strided_rows_and_strided_grad_x(metric):
    """x rows and grad_x rows inside wider buffers (row stride D + 12, a 16-byte multiple, and D + 3: the scalar row loads)."""
    name, T = "c33", 1.0
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, _, ref64, ref32 = _case(name, metric, T)
    m = x.shape[1]
    for pad in (12, 3):
        xbuf = torch.full((h, m, d + pad), float("nan"), device="cuda")
        xbuf[..., :d] = x.cuda()
        obuf = torch.full((h, m, d + pad), 7.0, device="cuda")
        got = _native(x, c, T, n, pos_div, _metric(metric), xd=xbuf[..., :d], gx_out=obuf[..., :d])
        assert got["gx"].data_ptr() == obuf.data_ptr() and bool((obuf[..., d:] == 7.0).all()), "grad_x wrote outside its rows"
        _compare(f"{name} {metric} strided +{pad}", got, ref64, ref32)


@pytest.mark.parametrize("metric", METRICS)
def test_both_sides_of_the_clamp(metric):
    """Constructed: half of the codes sit far from every row (Euclid: they get the mass; dot: large negative products),
    the other half close, so A has entries well above 1e-5 and well below it; U and the gradient are checked on each side."""
    h, b, n, k, d, T = 1, 32, 2, 64, 16, 4.0
    dot = metric == "dot"
    g = torch.Generator().manual_seed(5)
    x = torch.randn((h, b * n, d), generator=g) * 0.3
    c = torch.randn((h, k, d), generator=g) * 0.3
    if dot:
        c[:, : k // 2] -= 2.0 * x.mean(1, keepdim=True) / x.mean(1, keepdim=True).norm() * 3.0  # products around -6: z = +24
        x = x + x.mean(1, keepdim=True) / x.mean(1, keepdim=True).norm() * 2.0
    else:
        c[:, : k // 2] += 6.0 / d ** 0.5  # distance ~ 6 against ~ 1.7: z = 24 against 7
    ref64 = closed_form64(x, c, T, n, 1, dot, g_loss=G_LOSS)
    A = ref64["A"]
    above, below = A >= CLAMP, A < CLAMP
    assert int(above.sum()) >= k // 2 and int(below.sum()) >= k // 4, (int(above.sum()), int(below.sum()))
    assert float(A[above].min()) > 10 * CLAMP and float(A[below].max()) < CLAMP / 10, (float(A[above].min()), float(A[below].max()))
    ref32 = reference_sequence(x, c, T, n, 1, dot, dtype=torch.float32, g_loss=G_LOSS)
    ref32["delta"] = closed_form64(x, c, T, n, 1, dot, g_loss=G_LOSS, dtype=torch.float32)["delta"]
    got = _native(x, c, T, n, 1, _metric(metric))
    _compare(f"clamp {metric}", got, ref64, ref32)
    U, want = got["U"].double().cpu(), ref64["U"]
    # below the clamp U is the constant g / (N C) log(1e-5), above it g / (N C) (log A + 1): each side on its own
    assert float((U[below] - want[below]).abs().max()) <= GRAD_RTOL * float(want[below].abs().max())
    assert float(((U[above] - want[above]).abs() - GRAD_RTOL * want[above].abs()).max()) <= GRAD_ATOL_OF_MAX * float(want[above].abs().max())
    assert float(U[below].max()) < 0 < float(want[below].abs().min())


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["c33", "dp256", "heads2"])
def test_live_codes(name, metric):
    """Weights from c, contraction with l; l bit-equal to c gives the plain path's result bit for bit."""
    T = 1.0
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, lv, ref64, ref32 = _case(name, metric, T, True)
    mt = _metric(metric)
    got = _native(x, c, T, n, pos_div, mt, live=lv)
    _compare(f"{name} {metric} live", got, ref64, ref32)
    plain = _native(x, c, T, n, pos_div, mt)
    same = _native(x, c, T, n, pos_div, mt, live=c.clone())
    assert torch.equal(plain["gx"], same["gx"]), "live codes bit-equal to the searched codes must give the plain path's bits"
    assert not torch.equal(plain["gx"], got["gx"])


@pytest.mark.parametrize("name", ["splits", "splits_spp2", "heads2"])
def test_two_runs_are_bit_identical(name):
    (h, b, n, k, d), pos_div = SHAPES[name]
    x, c, _, _, _ = _case(name, "euclid", 100.0)
    a = _native(x, c, 100.0, n, pos_div, _metric("euclid"))
    b2 = _native(x, c, 100.0, n, pos_div, _metric("euclid"))
    for key in ("lse", "A", "delta", "gx"):
        assert torch.equal(a[key], b2[key]), key


def test_position_splits_cover_several_workgroups():
    """The `splits` shapes really run more than one blockIdx.z: the plan gives every CU a workgroup, one workgroup column here."""
    props = torch.cuda.get_device_properties(0)
    for name in ("splits", "splits_spp2"):
        (h, b, n, k, d), _ = SHAPES[name]
        blocks = (k + 127) // 128 * h
        want = min(64, n, -(-props.multi_processor_count // blocks))
        assert want >= 2 and -(-n // -(-n // want)) >= 2, name


# ------------------------------------------------------------------------------------------------ NaN
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chunked"])
def test_nan_row_gives_nan_loss(monkeypatch, fused):
    from vector_quantization import losses, search

    if not fused:
        monkeypatch.setenv("VQ_DIVERSITY_NO_FUSED", "1")
    (h, b, n, k, d), pos_div = SHAPES["c33"]
    x, c = make_inputs(h, b, n, k, d, False, 3)
    x[0, 5, 2] = float("nan")
    xd = x.cuda().requires_grad_(True)
    loss = losses.codebook_diversity_loss(xd, c.cuda(), search.EUCLID, 1.0, lambda: (torch.arange(x.shape[1], device="cuda") % n), n,
                                          pos_div=1)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss)), float(loss)
    assert xd.grad is not None and tuple(xd.grad.shape) == tuple(x.shape)


# ------------------------------------------------------------------------------------------------ module level
def _module(variant):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    kw, cb_kw, head_dim = dict(codebook_diversity_loss_weight=0.5), {}, 64
    if variant == "shared_heads":
        kw.update(heads=2, codebook_dim=32)
        head_dim = 32
    elif variant == "separate_heads":
        kw.update(heads=2, codebook_dim=32, separate_codebook_per_head=True)
        head_dim = 32
    elif variant == "cosine":
        # similarities in [-1, 1]: at the default temperature 100 the 16 x 256 entries of A cross 1e-5 so densely that none of
        # 17 seeds tried kept every entry 2 % away from it (margins of 0.01 % to 0.6 %); at 2 the clamp is out of reach
        cb_kw.update(use_cosine_sim=True, transform_input="l2norm", weights_regularization="l2norm")
        kw.update(codebook_diversity_temperature=2.0)
    elif variant == "ce_commitment":
        kw.update(commitment_use_cross_entropy_loss=True)
    torch.manual_seed(17)
    return vq.VectorQuantize(dim=64, codebook_params=CodebookParams(dim=head_dim, codebook_size=256, **cb_kw), **kw).cuda().train()


def _step(monkeypatch, mod, x):
    """One training step -> what the module returned and, recorded at the call of the diversity loss, its inputs and the
    gradient it sent back to its rows (the rows are handed on as a view of themselves, whose hook sees that gradient alone)."""
    from vector_quantization import losses

    seen = {}
    original = losses.codebook_diversity_loss

    def recording(rows, codes, metric, temperature, position, n_positions, live_codes=None, **kw):
        alias = rows.view_as(rows)
        alias.register_hook(lambda g: seen.__setitem__("gx", g.detach().clone()))
        seen.update(x=rows.detach().clone(), c=codes.detach().clone(), metric=metric, T=temperature, n=n_positions, live=live_codes,
                    pos_div=kw.get("pos_div"))
        return original(alias, codes, metric, temperature, position, n_positions, live_codes, **kw)

    monkeypatch.setattr(losses, "codebook_diversity_loss", recording)
    torch.manual_seed(29)  # (the EMA step replaces dead codes with random rows)
    xd = x.clone().requires_grad_(True)
    _, _, loss, parts = mod(xd, return_loss_breakdown=True)
    loss.sum().backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(losses, "codebook_diversity_loss", original)
    seen["live"] = seen["live"].detach().clone()  # the codes as the backward pass found them
    return dict(loss=loss.detach().sum().reshape(1), div=parts.codebook_diversity.detach().reshape(1), gx=xd.grad, seen=seen)


# seeds of x for which no fp64 A entry of the recorded call is within 2 % of the clamp
X_SEEDS = {"plain": 23, "shared_heads": 23, "separate_heads": 23, "cosine": 23, "ce_commitment": 23}


@pytest.mark.parametrize("variant", list(X_SEEDS))
def test_module_trains_without_the_similarity_matrix(monkeypatch, variant):
    """VectorQuantize(dim=64, K=256, codebook_diversity_loss_weight=0.5) in train mode with the default EMA codebook, x
    [32, 16, 64] (32 rows per position): forward + backward with the backend's `similarities` raising, against the same step
    on the chunked path (VQ_DIVERSITY_NO_FUSED=1).  The gradient rule: the fp64 closed form of the recorded call is the
    reference, the chunked path (the reference's fp32 op sequence on this device) measures its own error against it, and
    the fused path may be 4 x that far off (floors GRAD_ATOL_OF_MAX, GRAD_RTOL); x.grad of the two paths differs by no
    more than the two distances together."""
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
    # (the EMA step sums with atomics: the two modules' updated codes agree to rounding, each path is held to its own)
    torch.testing.assert_close(seen["live"], want["seen"]["live"], rtol=1e-5, atol=1e-6)
    assert not torch.equal(seen["live"], seen["c"]), "the EMA step rewrote the codes between forward and backward"
    h, m, _ = seen["x"].shape
    assert h * m // seen["n"] == 32 * (2 if variant in ("shared_heads", "separate_heads") else 1)
    ref64, ref64_chunked = (closed_form64(seen["x"].cpu(), seen["c"].cpu(), seen["T"], seen["n"], seen["pos_div"],
                                          seen["metric"] == search.DOT, live=r["seen"]["live"].cpu(), g_loss=0.5) for r in (got, want))
    margin = clamp_margin(ref64["A"])
    assert margin > 0.02, f"an fp64 A entry lies within {margin:.2%} of the clamp; pick another seed in X_SEEDS"
    scale = float(ref64["gx"].abs().max())
    ref_err = float((want["seen"]["gx"].double().cpu() - ref64_chunked["gx"]).abs().max()) / scale
    loss_err = abs(float(want["div"]) - float(ref64["loss"])) / abs(float(ref64["loss"]))
    print(f"{variant}: the chunked path is {ref_err:.2e} of the largest entry (gradient) and {loss_err:.2e} (loss) off fp64")
    atol_of_max = max(GRAD_ATOL_OF_MAX, 4 * ref_err)
    assert_grad_close(got["div"], ref64["loss"].reshape(1), f"{variant} diversity loss", atol_of_max=max(GRAD_ATOL_OF_MAX, 4 * loss_err))
    assert_grad_close(seen["gx"], ref64["gx"], f"{variant} d loss / d rows", atol_of_max=atol_of_max)
    # the module's outputs: everything but the diversity term is the same computation on both paths
    assert_grad_close(got["loss"], want["loss"], f"{variant} loss", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * loss_err))
    diversity_share = scale / float(want["gx"].abs().max())
    assert_grad_close(got["gx"], want["gx"], f"{variant} x.grad", atol_of_max=max(GRAD_ATOL_OF_MAX, 5 * ref_err * diversity_share))


# ------------------------------------------------------------------------------------------------ memory
def test_peak_memory_stays_below_one_similarity_matrix():
    """[64, 256, 64] with K = 4096, fused: forward + backward never allocate as much as ONE [M, K] fp32 matrix (256 MiB) --
    the fused path holds the packed row image, lse2 / delta [H, M] and A / U [N, K], nothing of M x K."""
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    gc.collect()
    torch.cuda.synchronize()
    foreign = torch.cuda.memory_allocated()  # what earlier tests of the process still hold (cached references): not this step's
    torch.manual_seed(3)
    mod = vq.VectorQuantize(dim=64, codebook_params=CodebookParams(dim=64, codebook_size=4096),
                            codebook_diversity_loss_weight=0.5).cuda().train()
    x = torch.randn((64, 256, 64), device="cuda", requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    _, _, loss = mod(x)
    loss.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - foreign  # the module, x and everything forward + backward allocated
    m, k = 64 * 256, 4096
    print(f"peak {peak / 2**20:.1f} MiB (beside {foreign / 2**20:.1f} MiB held by earlier tests); one [M, K] matrix: {m * k * 4 / 2**20:.0f} MiB")
    assert peak < m * k * 4
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
