"""vq_affine_stats_f32 / vq_affine_apply_f32 against fp64 models on the device: every column-width path (float4 and scalar,
one and several column groups), row counts around the lane / block boundaries, one and several heads, contiguous rows, rows
cut out of a wider buffer at an unaligned base, the modules' permuted [rows, heads, d] view, with and without masks.

The bound is computed from the kernel's documented geometry (include/vq_mi355x.h): with
gamma = (rows a lane folds sequentially + ceil(log2(number of merged partials)) + 4) * 2^-24,
|mean - mean64| <= 4 gamma mean|x| and |m2 / n - var64| <= 4 gamma (var64 + 2^-24 mean64^2); 4 is margin for the merges."""
from __future__ import annotations

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = (1, 3, 4, 5, 64, 100, 256, 257, 512, 1100)
ROWS = (1, 2, 63, 64, 65, 257, 4099)
EPS = 2.0 ** -24
_worst = {"mean": 0.0, "var": 0.0}


def geometry(H, M, D, vec):
    """(rows a lane folds, partials merged per column) -- the formulas of include/vq_mi355x.h"""
    per_row = -(-D // (4 if vec else 1))
    tc = 1
    while tc < per_row and tc < 64:
        tc *= 2
    tr = 256 // tc
    cg = -(-per_row // tc)
    nblk = max(1, min(-(-M // (16 * tr)), max(1, 1024 // (H * cg))))
    return -(-M // (nblk * tr)), nblk * tr


def layouts(H, M, D, gen):
    """name -> x [H, M, D] views over fresh buffers"""
    base = torch.randn((H, M, D), generator=gen, device=DEV)
    wide = torch.zeros((H, M, D + 7), device=DEV)
    wide[..., 3:3 + D] = base
    perm = torch.zeros((M, H, D), device=DEV)
    perm.copy_(base.permute(1, 0, 2))
    return {"contiguous": base, "slice": wide[..., 3:3 + D], "permuted": perm.permute(1, 0, 2)}


def masks(H, M, gen):
    out = {"none": None}
    if M > 1:
        out["random"] = torch.rand((H, M), generator=gen, device=DEV) < 0.6
        one = torch.zeros((H, M), dtype=torch.bool, device=DEV)
        one[H - 1, M // 2] = True  # a single row of one head
        out["one_row"] = one
    return out


def check_stats(x, mask, what):
    from vector_quantization import native

    H, M, D = x.shape
    count, mean, m2 = native.column_stats(x, mask)
    again = native.column_stats(x, mask)
    for a, b in zip((count, mean, m2), again):
        assert torch.equal(a, b), f"{what}: two runs differ"
    keep = torch.ones((H, M), dtype=torch.bool, device=x.device) if mask is None else mask
    n = keep.sum(dim=1)
    assert torch.equal(count, n), what
    w = keep[..., None].double()
    x64 = x.double()
    n64 = n.double().clamp(min=1)[:, None]
    mean64 = (x64 * w).sum(1) / n64
    var64 = (((x64 - mean64[:, None]) ** 2) * w).sum(1) / n64
    mean_abs = (x64.abs() * w).sum(1) / n64
    vec = D % 4 == 0 and x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0 and x.stride(1) % 4 == 0
    per_lane, merges = geometry(H, M, D, vec)
    gamma = (per_lane + math.ceil(math.log2(merges)) + 4) * EPS
    empty = (n == 0)[:, None].expand(H, D)
    assert bool((mean[empty] == 0).all()) and bool((m2[empty] == 0).all()), f"{what}: empty head"
    single = (n == 1)[:, None].expand(H, D)
    assert bool((m2[single] == 0).all()), f"{what}: one row must give m2 == 0"
    err_mean = (mean.double() - mean64).abs()
    err_var = (m2.double() / n64 - var64).abs()
    bound_mean = 4 * gamma * mean_abs
    bound_var = 4 * gamma * (var64 + EPS * mean64 ** 2)
    live = ~empty
    if bool(live.any()):
        rm = float((err_mean[live] / bound_mean[live].clamp(min=1e-300)).max())
        rv = float((err_var[live] / bound_var[live].clamp(min=1e-300)).max())
        _worst["mean"], _worst["var"] = max(_worst["mean"], rm), max(_worst["var"], rv)
    assert bool((err_mean <= bound_mean).all()), f"{what}: mean off by {float((err_mean - bound_mean).max()):.3e} beyond the bound"
    assert bool((err_var <= bound_var).all()), f"{what}: variance off by {float((err_var - bound_var).max()):.3e} beyond the bound"


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", DIMS)
def test_column_stats_against_fp64(D, H):
    gen = torch.Generator(device=DEV).manual_seed(1000 * H + D)
    for M in ROWS:
        for lname, x in layouts(H, M, D, gen).items():
            for mname, mask in masks(H, M, gen).items():
                check_stats(x, mask, f"D={D} M={M} H={H} {lname} mask={mname}")
    print(f"worst error / bound so far: mean {_worst['mean']:.3f}, variance {_worst['var']:.3f}")


@pytest.mark.parametrize("H", [1, 3])
def test_column_stats_many_rows(H):
    gen = torch.Generator(device=DEV).manual_seed(77 + H)
    for lname, x in layouts(H, 70001, 8, gen).items():
        for mname, mask in masks(H, 70001, gen).items():
            check_stats(x, mask, f"D=8 M=70001 H={H} {lname} mask={mname}")
    print(f"worst error / bound so far: mean {_worst['mean']:.3f}, variance {_worst['var']:.3f}")


def test_column_stats_of_offset_columns():
    """Columns of mean 1000 and sigma 1: sum x^2 - (sum x)^2 / n on the raw values is off by ~2^-24 * 1000^2 * sqrt(n) / n,
    orders of magnitude beyond the bound; the kernel never forms it."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    for D in (64, 100):
        x = 1000.0 + torch.randn((2, 4099, D), generator=gen, device=DEV)
        check_stats(x, None, f"offset columns D={D}")
        check_stats(x, torch.rand((2, 4099), generator=gen, device=DEV) < 0.5, f"offset columns D={D} masked")
    raw = (x * x).sum(1) / 4099 - (x.sum(1) / 4099) ** 2  # what the kernel must not do, in fp32
    var64 = x.double().var(1, unbiased=False)
    per_lane, merges = geometry(2, 4099, 100, True)
    bound = 4 * (per_lane + math.ceil(math.log2(merges)) + 4) * EPS * (var64 + EPS * x.double().mean(1) ** 2)
    assert float(((raw.double() - var64).abs() / bound).max()) > 100.0
    print(f"worst error / bound so far: mean {_worst['mean']:.3f}, variance {_worst['var']:.3f}")


def test_column_stats_argument_validation():
    import ctypes

    from vector_quantization import native

    lib = native.load()
    x = torch.zeros((1, 4, 8), device=DEV)
    out = torch.zeros(64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    ws = torch.zeros(int(lib.vq_affine_stats_workspace_bytes(1, 4, 8)) // 4 + 4, device=DEV)
    args = [x.data_ptr(), 8, 32, None, 0, 0, 1, 4, 8, cnt.data_ptr(), out.data_ptr(), out.data_ptr() + 128]
    assert lib.vq_affine_stats_f32(*args, ws.data_ptr(), 16, None) == -1 and b"workspace" in lib.vq_last_error()
    assert lib.vq_affine_stats_f32(*args[:9], None, out.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 4, None) == -1
    bad = list(args)
    bad[8] = 0
    assert lib.vq_affine_stats_f32(*bad, ws.data_ptr(), ws.numel() * 4, None) == -1 and b"size" in lib.vq_last_error()
    stats = [out.data_ptr()] * 4
    assert lib.vq_affine_apply_f32(x.data_ptr(), x.data_ptr(), None, *stats, 1, 4, 8, 1, None) == -1
    assert b"hits" in lib.vq_last_error()
    assert lib.vq_affine_apply_f32(x.data_ptr(), x.data_ptr(), None, *stats, 1, 4, 8, 2, None) == -1
    assert ctypes.c_int64(lib.vq_affine_stats_workspace_bytes(0, 4, 8)).value == 0


def _stats(H, D, gen, offset=0.0):
    cm = torch.randn((H, 1, D), generator=gen, device=DEV) * 0.3
    bm = torch.randn((H, 1, D), generator=gen, device=DEV) + offset
    cv = torch.rand((H, 1, D), generator=gen, device=DEV) + 0.05
    bv = torch.rand((H, 1, D), generator=gen, device=DEV) * 2 + 0.05
    cv[:, :, 0] = 1e-7  # below the clamp
    bv[:, :, -1] = 0.0
    return cm, cv, bm, bv


@pytest.mark.parametrize("H,K,D", [(1, 64, 32), (3, 33, 5), (2, 1024, 256), (1, 7, 1100)])
def test_affine_apply_codes_equals_the_torch_op_sequence(H, K, D):
    from vector_quantization import native

    gen = torch.Generator(device=DEV).manual_seed(K + D)
    codes = torch.randn((H, K, D), generator=gen, device=DEV)
    cm, cv, bm, bv = _stats(H, D, gen, offset=3.0)
    got = native.affine_apply(codes, cm, cv, bm, bv, mode=0)
    want = (codes - cm) * (bv.clamp(min=1e-5).sqrt() / cv.clamp(min=1e-5).sqrt()) + bm
    ulps = (got.view(torch.int32).long() - want.view(torch.int32).long()).abs().max()
    print(f"mode 0 vs the torch op sequence: {int(ulps)} ulp at most")
    assert torch.equal(got, want)
    again = native.affine_apply(codes.clone(), cm, cv, bm, bv, mode=0, out=None)
    assert torch.equal(got, again)


@pytest.mark.parametrize("H,K,D", [(1, 64, 32), (3, 33, 5), (2, 1024, 256)])
def test_affine_apply_sums_against_the_dense_fp64_model(H, K, D):
    """Mode 1 equals summing the transformed rows: checked against fp64 over dense rows, with the bound
    8 * 2^-24 * (r sum|x| + hits (|cm| + |bm r|)): the rounding of the sums handed in, of r (two square roots and a quotient),
    of the two products, of cm - bm r and of the final sum."""
    from vector_quantization import native

    gen = torch.Generator(device=DEV).manual_seed(K * D)
    M = 4 * K + 3
    cm, cv, bm, bv = _stats(H, D, gen, offset=3.0)
    x = torch.randn((H, M, D), generator=gen, device=DEV) * bv.clamp(min=1e-5).sqrt() + bm
    idx = torch.randint(0, K, (H, M), generator=gen, device=DEV)
    idx[:, 0] = K - 1
    onehot = torch.nn.functional.one_hot(idx, K).double()
    hits = onehot.sum(1).float()
    sums = (onehot.transpose(1, 2) @ x.double()).float()  # the per-code sums of the raw rows, rounded once
    got = native.affine_apply(sums, cm, cv, bm, bv, mode=1, hits=hits, out=sums)
    assert got.data_ptr() == sums.data_ptr()
    r = cv.double().clamp(min=1e-5).sqrt() / bv.double().clamp(min=1e-5).sqrt()
    want = onehot.transpose(1, 2) @ ((x.double() - bm.double()) * r + cm.double())
    abs_sums = onehot.transpose(1, 2) @ x.double().abs()
    bound = 8 * EPS * (r * abs_sums + hits.double()[..., None] * (cm.double().abs() + (bm.double() * r).abs()))
    err = (got.double() - want).abs()
    print(f"mode 1: worst error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
