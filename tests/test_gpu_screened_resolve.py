"""GPU: the second pass of the screened Dp = 256 sweep.  Rows the screen cannot bound (candidate overflow of a lane half,
NaN / inf rows, ineligible magnitudes, a flagged codebook) are put on a list by vq_search_persist<256, 8, EUCLID, false, true>
and searched again in full by vq_resolve_rows_kernel, which stores their idx and quantized rows over the provisional ones.
Every call must equal the fp32 sweep (VQ_NO_SCREEN, read per call) bit for bit -- indices and quantized rows viewed as
int32 -- and a row sample, the last 20 rows included, the CPU oracle.

M = 131 073 is the smallest row count at which the persistent kernel is selected at K = 1024, D = 256 on 256 CUs (two row
blocks of 256 rows per CU), and its last block holds one row."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 1024
D = 256
M0 = 131073


def _native():
    from vector_quantization import native

    native.load()
    return native


def _both(x, cb, strided=False):
    """(screened call, fp32-sweep call) of the same plain eval search; no distances requested (the screen's calls).
    strided: out / idx are [H, M, .] views of [M, H * .] tensors (the module's multi-head layout)."""
    native = _native()
    H, M, d = x.shape

    def call():
        if not strided:
            return native.quantize(x, cb, metric=0, want_best=False)
        out = torch.full((M, H * d), -7.0, device=x.device).view(M, H, d).permute(1, 0, 2)
        idx = torch.full((M, H, 1), -7, dtype=torch.int64, device=x.device).permute(1, 0, 2)
        return native.quantize(x, cb, metric=0, want_best=False, out=out, idx=idx)

    a = call()
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        b = call()
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    torch.cuda.synchronize()
    return a, b


def _check(x, cb, oracle, n_sample=200, strided=False):
    a, b = _both(x, cb, strided)
    assert torch.equal(a["idx"], b["idx"])
    assert torch.equal(a["out"].contiguous().view(torch.int32), b["out"].contiguous().view(torch.int32))
    H, M = x.shape[0], x.shape[1]
    rows = torch.cat([torch.randperm(M, generator=torch.Generator().manual_seed(3))[:n_sample], torch.arange(max(0, M - 20), M)])
    for h in range(H):
        ri, _ = oracle.nearest(x[h, rows].cpu().numpy(), cb[h, 0].cpu().numpy(), 0)
        np.testing.assert_array_equal(a["idx"][h, rows, 0].cpu().numpy(), ri)
    return a


@functools.lru_cache(maxsize=None)
def _tied():
    """128 distinct codes, each present 8 times at permuted indices.  The 8 copies of a row's nearest code have the same
    screened value; a lane half holds the codes whose index has the same bit 2, so one half holds at least four of them and
    its third lowest value is the lowest one: no row is certain or complete, every row goes through the list."""
    g = torch.Generator().manual_seed(21)
    base = torch.randn((1, 1, K // 8, D), generator=g)
    perm = torch.randperm(K, generator=g)
    cb = base.repeat(1, 1, 8, 1)[:, :, perm]
    x = torch.randn((1, M0, D), generator=g)
    return x.to(DEV), cb.to(DEV).contiguous(), perm


@functools.lru_cache(maxsize=None)
def _near_a_code(noise):
    """Codes randn * 8, every row a code plus `noise` * randn: the gap between the nearest and the second nearest code is
    ~3e4 in squared distance, far above the screen's bound (delta ~ 10 at these norms)."""
    g = torch.Generator().manual_seed(22)
    cb = torch.randn((1, 1, K, D), generator=g) * 8.0
    pick = torch.randint(0, K, (M0,), generator=g)
    x = cb[0, 0, pick][None] + noise * torch.randn((1, M0, D), generator=g)
    return x.to(DEV), cb.to(DEV), pick


def test_every_row_listed_lowest_tied_copy_wins(oracle):
    """The capacity case: the list holds all H M rows.  Among the 8 tied copies the lowest index wins."""
    x, cb, perm = _tied()
    a = _check(x, cb, oracle)
    # position j of the codebook holds distinct code perm[j] % 128: the winner is the first position of its code
    code_of = (perm % (K // 8)).to(DEV)
    first = torch.full((K // 8,), K, dtype=torch.int64, device=DEV).scatter_reduce(0, code_of, torch.arange(K, device=DEV), "amin")
    idx = a["idx"][0, :, 0]
    assert torch.equal(idx, first[code_of[idx]])


@pytest.mark.parametrize("noise", [1e-3, 0.5])
def test_rows_next_to_a_code(oracle, noise):
    """Huge gaps between the nearest and the second nearest code.  noise = 0.5: the winner's squared distance (~64) is above
    twice the bound, every row is certain, the list stays empty and the second pass finds nothing.  noise = 1e-3: the winner's
    squared distance (~3e-4) is inside the bound, where the screen cannot exclude a clamp to 0, so these rows are listed."""
    x, cb, pick = _near_a_code(noise)
    a = _check(x, cb, oracle)
    assert torch.equal(a["idx"][0, :, 0].cpu(), pick)


def test_mixed_ragged_two_strided_heads(oracle):
    """H = 2 as [H, M, d] views of [M, H * d] tensors (x, out and idx), M = 131 072 + 77 per head, K = 1000, D = 252,
    kaiming-uniform data (near ties: some rows certain, some rescored, some listed), NaN / +inf / -inf rows at the first row,
    in the last (partial) block and in head 1: the head / row decoding of the entries and the strided idx / out stores."""
    H, M, k, d = 2, 131072 + 77, 1000, 252
    g = torch.Generator().manual_seed(23)
    bound = (6.0 / d) ** 0.5
    cb = ((torch.rand((H, 1, k, d), generator=g) * 2 - 1) * bound).to(DEV)
    xf = ((torch.rand((M, H * d), generator=g) * 2 - 1) * bound).to(DEV)
    x = xf.view(M, H, d).permute(1, 0, 2)
    x[0, 0, 7] = float("nan")
    x[0, 131072 + 50, 0] = float("inf")
    x[0, M - 1, 251] = -float("inf")
    x[1, 5, 100] = -float("inf")
    x[1, 70000, 3] = float("nan")
    x[1, 131072 + 3, 17] = float("inf")
    a = _check(x, cb, oracle, strided=True)
    assert a["idx"].stride() == (1, H, 1) and a["out"].stride() == (d, H * d, 1)
    assert int(a["idx"].min()) >= 0 and int(a["idx"].max()) < k  # (every element of the -7-filled views was stored)


def test_flagged_codebook_lists_every_row(oracle):
    """One NaN code flags the codebook: no row is eligible, every row is listed and the non-finite rule decides."""
    g = torch.Generator().manual_seed(24)
    cb = torch.randn((1, 1, K, D), generator=g)
    x = torch.randn((1, M0, D), generator=g)
    cb[0, 0, 100, 9] = float("nan")
    _check(x.to(DEV), cb.to(DEV), oracle, n_sample=100)


def test_two_calls_in_a_row_share_no_entries(oracle):
    """Every row listed, then no row listed, with calls of one shape (the allocator hands the second call the first call's
    workspace block): the count is zeroed per call, so the second call resolves none of the first call's entries."""
    x1, cb1, _ = _tied()
    x2, cb2, pick = _near_a_code(0.5)
    native = _native()
    a1 = native.quantize(x1, cb1, metric=0, want_best=False)
    a2 = native.quantize(x2, cb2, metric=0, want_best=False)
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        b1 = native.quantize(x1, cb1, metric=0, want_best=False)
        b2 = native.quantize(x2, cb2, metric=0, want_best=False)
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    torch.cuda.synchronize()
    for a, b in ((a1, b1), (a2, b2)):
        assert torch.equal(a["idx"], b["idx"])
        assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32))
    assert torch.equal(a2["idx"][0, :, 0].cpu(), pick)
    x3, cb3, _ = _near_a_code(1e-3)
    _check(x3, cb3, oracle, n_sample=20)


def test_a_screened_call_launches_pack_sweep_resolve_in_order():
    from torch.profiler import ProfilerActivity, profile

    native = _native()
    x, cb, _ = _near_a_code(0.5)
    packed = native.pack_codebooks(cb, 0)
    native.quantize(x, cb, packed=packed, want_best=False)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        native.quantize(x, cb, packed=packed, want_best=False)
        torch.cuda.synchronize()
    evs = [ev for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and "vq_" in ev.name]
    if not evs:
        pytest.skip("torch.profiler reported no device activity on this build")
    evs.sort(key=lambda ev: ev.time_range.start)
    names = [ev.name for ev in evs]

    def pos(pred):
        hits = [i for i, n in enumerate(names) if pred(n)]
        assert len(hits) == 1, names
        return hits[0]

    i_pack = pos(lambda n: "vq_pack_scr_kernel" in n)
    i_sweep = pos(lambda n: "vq_search_persist" in n and "true>" in n)
    i_res = pos(lambda n: "vq_resolve_rows_kernel" in n)
    assert i_pack < i_sweep < i_res, names
