"""fsq_quantize_kernel<D>, fsq_backward_kernel<D> and fsq_decode_kernel<D> at every D = 1 .. 16, with the levels and inputs
of tests/fsq_dense.py (levels_for: every level <= 25, where every index term is a whole number, and a codebook of at most
2^24 codes, so that a row's index does not depend on the order of the sum; tests/test_fsq_host.py checks that recipe on
the CPU).  Inputs are randn * 2 on 20 011 rows: 79 workgroups, the last one ragged.

What is compared with what:
  * the fused forward with the torch fallback on the GPU (FSQ, ResidualFSQ with Q = 3, GroupedResidualFSQ with G = 3 and
    Q = 3, no projections): out and idx bitwise on the rows whose every stage clears a rounding boundary by 1e-5 in fp64
    (fsq_dense.chain64); fewer than 1 % of the rows may be left out.  The indices are compared at d >= 8 as well, which is
    valid only because every term of the kernel's codes is a whole number; the test asserts that.
  * a single stage with fp64: out == float32(round(bound64(x)) / hw) and idx == sum (k_i + hw_i) basis_i in int64 on the
    clearing rows.  Deeper stages are not compared with fp64: stage t divides the residual by (L - 1)^-t, which amplifies
    one ulp of the residual beyond any margin.
  * idx with the numpy index model (fsq_dense.indices_np, the kernel's expression and order) applied to the kernel's own
    codes, on every row, also with a last level of 26, where codes collide.
  * the backward with the fp64 restatement (fsq_dense.restate) at S = 1 and S = 3, saturated rows included.
  * the decode with a gather from the implicit codebook, bitwise."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest
import torch

from fsq_dense import bound64, chain64, exact_indices, indices_np, levels_for, restate, sweep_input, whole_terms
from test_gpu_fsq import fallback
from test_gpu_lq import count_native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT32_MIN = -(2**31)
CANARY = -77.25
DIMS = list(range(1, 17))
ROWS = 20011
Q3 = 3
G3 = 3


def _scales(levels, Q):
    lv = torch.tensor(levels, dtype=torch.float32)
    return torch.stack([(lv - 1) ** -q for q in range(Q)]).to(DEV)


def _consts(levels, Q=None):
    from vector_quantization.finite_scalar_quantization import kernel_consts

    return kernel_consts(torch.tensor(levels, dtype=torch.int32, device=DEV), None if Q is None else _scales(levels, Q))


def _build(kind, levels):
    from vector_quantization import FSQ, GroupedResidualFSQ, ResidualFSQ

    d = len(levels)
    if kind == "fsq":
        return FSQ(levels).to(DEV)
    if kind == "rfsq":
        return ResidualFSQ(dim=d, levels=levels, num_quantizers=Q3).to(DEV)
    return GroupedResidualFSQ(dim=G3 * d, groups=G3, levels=levels, num_quantizers=Q3).to(DEV)


def _clearing(kind, levels, x):
    """x [1, N, dim] on the GPU -> [1, N] bool: every stage of every group clears a rounding boundary by 1e-5 in fp64."""
    d = len(levels)
    if kind == "fsq":
        _, margin = chain64(x.double(), levels, None, False)
    elif kind == "rfsq":
        _, margin = chain64(x.double(), levels, _scales(levels, Q3).double(), True)
    else:
        xs = x.double().reshape(x.shape[0], x.shape[1], G3, d)
        _, margin = chain64(xs, levels, _scales(levels, Q3).double(), True)
        margin = margin.min(dim=-1).values
    return margin >= 1e-5


def _rows_view(kind, d, out, idx):
    """out, idx of a module -> [1, N, G, d] and [1, N, G, S]."""
    if kind == "fsq":
        return out[:, :, None, :], idx[:, :, None, None]
    if kind == "rfsq":
        return out[:, :, None, :], idx[:, :, None, :]
    return out.reshape(*out.shape[:2], G3, d), idx.permute(1, 2, 0, 3)


@pytest.mark.parametrize("kind", ["fsq", "rfsq", "grfsq"])
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_quantize_against_fallback(d, kind):
    levels = levels_for(d)
    mod = _build(kind, levels).eval()
    width = d * (G3 if kind == "grfsq" else 1)
    x = torch.from_numpy(sweep_input(ROWS, width, 300 + d)[None]).to(DEV)
    with torch.no_grad():
        with count_native() as calls:
            out, idx = mod(x)
        with fallback(), count_native() as fb_calls:
            want, want_idx = mod(x)
    assert len(calls["fsq_quantize"]) == 1 and "fsq_quantize" not in fb_calls
    assert out.shape == want.shape == x.shape and idx.shape == want_idx.shape and idx.dtype == want_idx.dtype
    ok = _clearing(kind, levels, x)
    left_out = 1.0 - float(ok.double().mean())
    o1, i1 = _rows_view(kind, d, out, idx)
    o2, i2 = _rows_view(kind, d, want, want_idx)
    n_diff = int(((o1 != o2).flatten(2).any(-1) | (i1 != i2).flatten(2).any(-1))[ok].sum())
    print(f"d{d} {kind}: {left_out:.4%} of rows within 1e-5 of a rounding boundary; {n_diff} clearing rows differ")
    assert left_out < 0.01
    assert torch.equal(o1[ok].view(torch.int32), o2[ok].view(torch.int32)), "out differs from the fallback"
    assert torch.equal(i1[ok], i2[ok]), "idx differs from the fallback"
    # the kernel's codes, stage by stage (gathered from the implicit codebook by the kernel's indices; they must rebuild its
    # out): every index term is a whole number, so the comparison of the indices above holds in any order of the sum
    if kind == "fsq":
        stage_codes = out
    else:
        cb = (mod if kind == "rfsq" else mod.rvqs[0]).layers[0].implicit_codebook
        stage_codes = cb[i1.long()]  # [1, N, G, S, d]
        sc = _scales(levels, Q3)
        acc = torch.zeros_like(o1)
        for q in range(Q3):
            acc = acc + stage_codes[..., q, :] * sc[q]
        assert torch.equal(acc, o1), "the stage codes of the kernel's indices do not sum to its out"
    assert whole_terms(stage_codes.cpu().numpy().reshape(-1, d), levels).all()


@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_single_stage_against_fp64(d):
    from vector_quantization import native

    levels = levels_for(d)
    x = sweep_input(ROWS, d, 300 + d)
    out, idx = native.fsq_quantize(torch.from_numpy(x[None]).to(DEV), levels, _consts(levels))
    out, idx = out.cpu().numpy()[0], idx.cpu().numpy()[0, :, 0]
    x64 = torch.from_numpy(x).double()
    _, margin = chain64(x64, levels, None, False)
    ok = (margin >= 1e-5).numpy()
    assert 1.0 - ok.mean() < 0.01
    k = torch.round(bound64(x64, levels)).numpy()
    hw = np.array([v // 2 for v in levels], dtype=np.float64)
    want = (k / hw).astype(np.float32)
    assert np.array_equal(out[ok], want[ok]), "out is not float32(round(bound64(x)) / hw)"
    assert np.array_equal(idx[ok].astype(np.int64), exact_indices(k, levels)[ok]), "idx is not the integer index"


def _collide_levels(d):
    levels = list(levels_for(d))
    levels[-1] = 26  # hw = 13: fl(fl(k / 13) * 13) != k for some k, the term is not whole and the truncation collides
    return levels


@pytest.mark.parametrize("variant", ["sweep", "collide"])
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_index_model_on_the_kernels_codes(d, variant):
    """idx == fsq_dense.indices_np(the kernel's own codes) on every row.  collide: the last level is 26 (at d >= 8 too: the
    model's order t0, t4 .. t(d-1), t1, t2, t3 is the kernel's), and some term is not a whole number."""
    from vector_quantization import native

    levels = levels_for(d) if variant == "sweep" else _collide_levels(d)
    assert int(np.prod(np.array(levels, dtype=np.int64))) <= 2**24
    x = sweep_input(ROWS, d, 400 + d)
    if variant == "collide":  # every code of the last dimension: inputs whose bound lands on k exactly
        L = 26
        k = np.arange(L, dtype=np.float64) - L // 2
        half_l, offset = (L - 1) * 1.001 / 2, 0.5
        x[:L, d - 1] = (np.arctanh((k + offset) / half_l) - np.arctanh(offset / half_l)).astype(np.float32)
    out, idx = native.fsq_quantize(torch.from_numpy(x[None]).to(DEV), levels, _consts(levels))
    codes = out.cpu().numpy()[0]
    got = idx.cpu().numpy()[0, :, 0]
    assert np.array_equal(got, indices_np(codes, levels))
    if variant == "collide":
        assert len(np.unique(np.rint(codes[:26, d - 1] * 13))) == 26
        assert not whole_terms(codes, levels).all()
    else:
        assert whole_terms(codes, levels).all()


@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_strided_groups_and_padded_rows(d):
    """x [G, N, d] read from a padded [N, G * d + 5] buffer (group stride d, row stride G * d + 5), out written into a
    canary-filled buffer of the same layout; S = 3 with the extra bound."""
    from vector_quantization import native

    levels = levels_for(d)
    consts = _consts(levels, Q3)
    W = G3 * d
    xc = torch.from_numpy(sweep_input(ROWS, W, 600 + d)).to(DEV)
    buf = torch.full((ROWS, W + 5), 3.0, device=DEV)
    buf[:, 3:3 + W] = xc
    obuf = torch.full((ROWS, W + 5), CANARY, device=DEV)
    x = buf[:, 3:3 + W].unflatten(1, (G3, d)).transpose(0, 1)
    out = obuf[:, 3:3 + W].unflatten(1, (G3, d)).transpose(0, 1)
    assert x.stride() == (d, W + 5, 1) and out.stride() == (d, W + 5, 1)
    got, idx = native.fsq_quantize(x, levels, consts, prebound=True, out=out)
    assert got.data_ptr() == out.data_ptr()
    want, want_idx = native.fsq_quantize(xc.reshape(ROWS, G3, d).transpose(0, 1).contiguous(), levels, consts, prebound=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(idx, want_idx)
    assert idx.shape == (G3, ROWS, Q3)
    assert bool((obuf[:, :3] == CANARY).all()) and bool((obuf[:, 3 + W:] == CANARY).all())
    # the backward with strided operands: bitwise the contiguous call
    g = torch.from_numpy(sweep_input(ROWS, W, 601 + d)).to(DEV)
    gbuf = torch.full((ROWS, W + 5), CANARY, device=DEV)
    gx = native.fsq_backward(x, levels, consts, g.reshape(ROWS, G3, d).transpose(0, 1), prebound=True,
                             grad_x=gbuf[:, 3:3 + W].unflatten(1, (G3, d)).transpose(0, 1))
    want_gx = native.fsq_backward(x.contiguous(), levels, consts, g.reshape(ROWS, G3, d).transpose(0, 1).contiguous(),
                                  prebound=True)
    assert torch.equal(gx.view(torch.int32), want_gx.view(torch.int32))
    assert bool((gbuf[:, :3] == CANARY).all()) and bool((gbuf[:, 3 + W:] == CANARY).all())


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_backward_against_fp64(d, S):
    """dL/dx of (out * r).sum() against fsq_dense.restate on the clearing rows: |got - want| <= 1e-4 |want| + 1e-6 S, the
    form of test_gpu_fsq.py::test_fixture.  Should that fail, the floor is 2 x the largest distance of the torch
    fallback's own fp32 gradient from the same restatement (the fixtures' grad_ref_dev rule), measured on the rows that
    do not saturate; both distances are printed.  A fifth of the rows is spread over [-12, 12], where tanh saturates: the
    gradient there is finite and matches fp64 (fsq_sech2)."""
    levels = levels_for(d)
    kind = "fsq" if S == 1 else "rfsq"
    mod = _build(kind, levels).train()
    x0 = sweep_input(ROWS, d, 700 + d)
    x0[::5] = np.clip(x0[::5] * 3, -12, 12)
    r = torch.from_numpy(sweep_input(ROWS, d, 701 + d, 1.0)[None]).to(DEV)
    grads = []
    for fused in (True, False):
        x = torch.from_numpy(x0[None]).to(DEV).requires_grad_(True)
        with contextlib.nullcontext() if fused else fallback(), count_native() as calls:
            out, _ = mod(x)
            (out * r).sum().backward()
        assert (len(calls.get("fsq_quantize", [])), len(calls.get("fsq_backward", []))) == ((1, 1) if fused else (0, 0))
        grads.append(x.grad.double())
    got, fb = grads
    assert bool(torch.isfinite(got).all())
    kw = dict(levels=levels) if S == 1 else dict(levels=levels, num_quantizers=S)
    want = restate(kind, kw, {}, torch.from_numpy(x0[None]).to(DEV), r)["grad"]
    ok = _clearing(kind, levels, torch.from_numpy(x0[None]).to(DEV))[..., None].expand_as(want)
    err = (got - want).abs()
    bound = 1e-4 * want.abs() + 1e-6 * S
    worst = float((err - bound)[ok].max())
    calm = torch.ones_like(ok)
    calm[:, ::5] = False  # the rows spread over [-12, 12]: the fallback's fp32 1 - tanh^2 cancels there
    fb_dev = float((fb - want).abs()[ok & calm].max())
    print(f"d{d} S{S}: largest |fused - fp64| {float(err[ok].max()):.3e}, largest excess over the bound {worst:.3e}; "
          f"fallback's own distance from fp64 {fb_dev:.3e}")
    if worst > 0:
        assert bool((err <= bound + 2 * fb_dev)[ok].all())


_CODEBOOK = {}


def _implicit_codebook(d):
    """[K, d] built on the CPU by the module's torch arithmetic (the reference's), then moved."""
    from vector_quantization import FSQ

    if _CODEBOOK.get("d") != d:
        _CODEBOOK.clear()
        _CODEBOOK.update(d=d, cb=FSQ(levels_for(d)).implicit_codebook.to(DEV))
    return _CODEBOOK["cb"]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_decode_bitwise_equals_gather(d, Q, dtype):
    from vector_quantization import native

    levels = levels_for(d)
    K = int(np.prod(np.array(levels, dtype=np.int64)))
    cb = _implicit_codebook(d)
    assert cb.shape == (K, d)
    N = 5003
    g = torch.Generator(device=DEV).manual_seed(50 + d)
    idx = torch.randint(0, K, (N, Q), device=DEV, generator=g).to(dtype)
    idx[0] = 0
    idx[1] = K - 1
    idx[N - 1] = K - 1
    idx[2, Q - 1] = 0
    scales = _scales(levels, Q).contiguous()
    want = torch.stack([cb[idx[:, q].long()] * scales[q] for q in range(Q)])
    acc = torch.zeros_like(want[0])
    for q in range(Q):
        acc = acc + want[q]
    s, a = native.fsq_decode(idx, levels, scales, want_sum=True, want_all=True)
    assert torch.equal(s.view(torch.int32), acc.view(torch.int32)) and torch.equal(a.view(torch.int32), want.view(torch.int32))
    s2, a2 = native.fsq_decode(idx, levels, scales, want_sum=True, want_all=False)
    s3, a3 = native.fsq_decode(idx, levels, scales, want_sum=False, want_all=True)
    assert a2 is None and s3 is None and torch.equal(s2, s) and torch.equal(a3, a)
    # dropped stages
    idx[5:700:3, Q - 1] = -1
    idx[N - 2] = -1
    null = (idx == -1).T[..., None]
    want = torch.stack([cb[idx[:, q].clamp(min=0).long()] * scales[q] for q in range(Q)]).masked_fill(null, 0.0)
    acc = torch.zeros_like(want[0])
    for q in range(Q):
        acc = acc + want[q]
    s, a = native.fsq_decode(idx, levels, scales, drop_null=True, want_sum=True, want_all=True)
    assert torch.equal(s.view(torch.int32), acc.view(torch.int32)) and torch.equal(a.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("kind", ["fsq", "rfsq"])
@pytest.mark.parametrize("d", DIMS, ids=lambda d: f"d{d}")
def test_nonfinite_in_the_last_dimension(d, kind):
    """NaN, +inf and -inf, each alone in dimension d - 1 of a row: the NaN row's index is INT32_MIN and its last value NaN,
    an infinite input saturates tanh and quantizes to the outermost code; all as the fallback has it."""
    levels = levels_for(d)
    mod = _build(kind, levels).eval()
    x0 = sweep_input(1003, d, 800 + d)
    x0[[10, 500, 1002], d - 1] = [np.nan, np.inf, -np.inf]
    x = torch.from_numpy(x0[None]).to(DEV)
    with torch.no_grad():
        with count_native() as calls:
            out, idx = mod(x)
        with fallback(), count_native() as fb_calls:
            want, want_idx = mod(x)
    assert len(calls["fsq_quantize"]) == 1 and "fsq_quantize" not in fb_calls
    ok = _clearing(kind, levels, x)
    assert bool(ok[0, [10, 500, 1002]].all())
    o1, i1 = _rows_view(kind, d, out, idx)
    o2, i2 = _rows_view(kind, d, want, want_idx)
    assert torch.equal(o1.isnan(), o2.isnan())
    # bitwise off the NaNs (the payload of a generated NaN is the machine's)
    assert torch.equal(o1.nan_to_num(7.0)[ok].view(torch.int32), o2.nan_to_num(7.0)[ok].view(torch.int32))
    assert torch.equal(i1[ok], i2[ok])
    assert bool(out[0, 10, d - 1].isnan()) and int(out[0].isnan().sum()) == 1
    assert bool((i1[0, 10] == INT32_MIN).all())
    assert bool(torch.isfinite(out[0, [500, 1002]]).all()) and bool((i1[0, [500, 1002]] >= 0).all())
