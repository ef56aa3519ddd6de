"""GPU: the rescore list of the screened Dp = 256 sweep.  A row whose two lowest screened values are too close to call, but
whose candidates are all among the <= 4 codes its two lane halves track, is put on the rescore list by
vq_search_persist<256, 8, EUCLID, false, true>: its idx element carries the candidate codes (four 16-bit fields) to
vq_resolve_rows_kernel, which runs the exact chain for each of them and stores idx and the quantized row.  Rows with more
candidates than a lane half tracks go on the full-search list, which shares one array with the rescore list (front / back).

Every call must equal the fp32 sweep (VQ_NO_SCREEN, read per call) bit for bit -- indices and quantized rows viewed as int32
-- and a row sample, the last 20 rows included, the CPU oracle; every idx element must be a code (no candidate word
survives).

That a case really takes the list it is about is proven on the host in fp64, for the sampled rows, from the kernel's own
formula delta = 2.5e-4 * 2 |x| max|c| + 1e-4 max|c|^2 + 3e-7 |x|^2 (>= 2.16 delta_0, delta_0 the screen's proven error):
  * the squared distances of the intended candidates lie within 0.1 delta of each other, so their screened values differ
    by < 0.1 delta + 2 delta_0 < 2 delta: the row is uncertain whatever the screen's error;
  * every other code is more than 4 delta further than the furthest candidate, so its screened value is above
    thr = b1 + 2 delta + w (4 delta - 2 delta_0 > 3 delta): with <= 2 candidates per lane half the row is complete (rescored),
    with 3 in one half that half's third lowest value is below thr and the row is searched in full;
  * the nearest candidate's squared distance is above 3 delta: the row is eligible (no clamp to 0 possible).
A lane half holds the codes whose index has the same bit 2.

M = 131 073 is the smallest row count at which the persistent kernel is selected at K = 1024, D = 256 on 256 CUs."""
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
SCALE = 8.0   # codes are randn * SCALE: two unrelated codes are ~2 * 64 * D apart in squared distance (thousands of delta)
NOISE = 0.5   # rows are a code + NOISE * randn: squared distance to it ~ D / 4 (about 6 delta)
EPS = 2e-3    # near copies differ from their original by EPS in one dim: ~2e-3 in squared distance (delta ~ 10), hundreds
              # of fp32 ulps of the distance, so the exact chain and not the index decides most of these rows


def _native():
    from vector_quantization import native

    native.load()
    return native


def _near_copy(cb, src, dst, j=1):
    """cb[dst] = cb[src] with dim (src + j) % d moved by j * EPS (distinct copies for distinct j)."""
    cb[dst] = cb[src]
    cb[dst, (src + j) % cb.shape[1]] += j * EPS


def _twin_codebook(k, d, mask, seed):
    """Every code i with (i & mask) == 0 has a near copy at i ^ mask.  mask = 1: both in one lane half; mask = 4: one in each."""
    cb = torch.randn((k, d), generator=torch.Generator().manual_seed(seed)) * SCALE
    for i in range(k):
        if (i & mask) == 0:
            _near_copy(cb, i, i ^ mask)
    return cb


def _rows(cb, pick, seed):
    return cb[pick] + NOISE * torch.randn((pick.numel(), cb.shape[1]), generator=torch.Generator().manual_seed(seed))


def _sample(m, n=200):
    return torch.cat([torch.randperm(m, generator=torch.Generator().manual_seed(3))[:n], torch.arange(max(0, m - 20), m)])


def _prove(x, cb, cands, full_search=False):
    """The fp64 proof of the module docstring for rows x [n, d] and their intended candidates cands [n, c] (code indices)."""
    x, cb = x.double().numpy(), cb.double().numpy()
    cands = np.asarray(cands)
    xn, cn = (x * x).sum(1), (cb * cb).sum(1)
    delta = 2.5e-4 * 2.0 * np.sqrt(xn) * np.sqrt(cn.max()) + 1e-4 * cn.max() + 3e-7 * xn
    dist = xn[:, None] + cn[None, :] - 2.0 * (x @ cb.T)  # (fp64: exact to ~1e-11 here, against gaps of 1e-3 and more)
    dc = np.take_along_axis(dist, cands, 1)
    rest = dist.copy()
    np.put_along_axis(rest, cands, np.inf, 1)
    assert (dc.max(1) - dc.min(1) < 0.1 * delta).all()
    assert (rest.min(1) - dc.max(1) > 4.0 * delta).all()
    assert (dc.min(1) > 3.0 * delta).all()
    in_half1 = ((cands >> 2) & 1).sum(1)
    per_half = np.maximum(in_half1, cands.shape[1] - in_half1)
    assert (per_half >= 3).all() if full_search else (per_half <= 2).all()


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


def _check(x, cb, oracle, strided=False, a=None):
    """x [H, M, d], cb [H, 1, k, d] on the GPU: the screened call against the fp32 sweep and the oracle sample."""
    if a is None:
        a, b = _both(x, cb, strided)
        assert torch.equal(a["idx"], b["idx"])
        assert torch.equal(a["out"].contiguous().view(torch.int32), b["out"].contiguous().view(torch.int32))
    assert int(a["idx"].min()) >= 0 and int(a["idx"].max()) < cb.shape[2]  # every element: no candidate word survives
    rows = _sample(x.shape[1])
    for h in range(x.shape[0]):
        ri, _ = oracle.nearest(x[h, rows].cpu().numpy(), cb[h, 0].cpu().numpy(), 0)
        np.testing.assert_array_equal(a["idx"][h, rows, 0].cpu().numpy(), ri)
    return a


@functools.lru_cache(maxsize=None)
def _twins(mask):
    cb = _twin_codebook(K, D, mask, seed=40 + mask)
    pick = torch.randint(0, K, (M0,), generator=torch.Generator().manual_seed(31))
    x = _rows(cb, pick, seed=32)
    rows = _sample(M0)
    _prove(x[rows], cb, torch.stack([pick[rows], pick[rows] ^ mask], 1))
    return x[None].to(DEV), cb[None, None].to(DEV)


@pytest.mark.parametrize("mask", [1, 4])
def test_twin_codes_two_candidates(oracle, mask):
    """Every row is next to a code and its near copy: two candidates in one lane half (mask 1: both from one lane) or one in
    each half (mask 4).  Every row is rescored."""
    x, cb = _twins(mask)
    a = _check(x, cb, oracle)
    idx = a["idx"][0, :, 0].cpu()
    won_by_copy = int(((idx & mask) != 0).sum())
    assert 0.2 * M0 < won_by_copy < 0.8 * M0  # both members of the pairs win rows: the exact chains decided, not the index


def test_exact_duplicates_lowest_index_wins(oracle):
    """512 distinct codes, each present twice at permuted indices: both copies of the nearest code are candidates with the
    same exact distance, and the rescored tie goes to the lowest index."""
    g = torch.Generator().manual_seed(51)
    base = torch.randn((K // 2, D), generator=g) * SCALE
    perm = torch.randperm(K, generator=g)
    code_of = perm % (K // 2)   # position j holds distinct code code_of[j]
    cb = base[code_of]
    pick = torch.randint(0, K, (M0,), generator=g)
    x = _rows(cb, pick, seed=52)
    pos = torch.stack([torch.nonzero(code_of == c).flatten() for c in range(K // 2)])  # [512, 2] positions, ascending
    rows = _sample(M0)
    _prove(x[rows], cb, pos[code_of[pick[rows]]])
    a = _check(x[None].to(DEV), cb[None, None].to(DEV), oracle)
    assert torch.equal(a["idx"][0, :, 0].cpu(), pos[code_of[pick], 0])


@functools.lru_cache(maxsize=None)
def _groups_codebook():
    """Groups of 8 consecutive codes (indices 8 g .. 8 g + 3 in lane half 0, 8 g + 4 .. 8 g + 7 in half 1).  Even groups: code
    8 g has near copies at 8 g + 1, + 4, + 5 (four candidates, two per half: rescored).  Odd groups: at 8 g + 1, + 2 (three in
    one half: candidate overflow, searched in full).  The other codes of a group are unrelated."""
    cb = torch.randn((K, D), generator=torch.Generator().manual_seed(61)) * SCALE
    for g in range(K // 8):
        for j, off in enumerate((1, 4, 5) if g % 2 == 0 else (1, 2)):
            _near_copy(cb, 8 * g, 8 * g + off, j + 1)
    return cb


QUAD = torch.tensor([0, 1, 4, 5])
TRIPLE = torch.tensor([0, 1, 2])


@pytest.mark.parametrize("with_certain_rows", [True, False])
def test_both_lists_at_once(oracle, with_certain_rows):
    """Rows next to a four-copy group (rescore list) and rows next to a three-in-one-half group (full-search list) in one
    call.  with_certain_rows: a third of the rows are next to an unrelated code and go on neither list.  Without them every
    row is on one list or the other, about half each: the two-ended array fills to H M entries in total (capacity)."""
    cb = _groups_codebook()
    g = torch.Generator().manual_seed(62 + int(with_certain_rows))
    kind = torch.randint(0, 3 if with_certain_rows else 2, (M0,), generator=g)  # 0: four copies, 1: three copies, 2: unrelated
    grp = torch.randint(0, K // 16, (M0,), generator=g)
    base = 8 * (2 * grp + (kind == 1).long())
    member = torch.randint(0, 3, (M0,), generator=g)  # which of the copies the row starts from
    pick = torch.where(kind == 0, base + QUAD[member], torch.where(kind == 1, base + TRIPLE[member], base + 6 + member % 2))
    x = _rows(cb, pick, seed=64)
    rows = _sample(M0)
    for k, offs in ((0, QUAD), (1, TRIPLE)):
        sel = rows[kind[rows] == k]
        assert sel.numel() > 20
        _prove(x[sel], cb, base[sel, None] + offs[None], full_search=(k == 1))
    a = _check(x[None].to(DEV), cb[None, None].to(DEV), oracle)
    idx = a["idx"][0, :, 0].cpu()
    assert torch.equal(idx[kind == 2], pick[kind == 2])
    assert torch.equal(idx[kind != 2] // 8, pick[kind != 2] // 8)


def test_two_strided_heads_ragged(oracle):
    """H = 2 as [H, M, d] views of [M, H * d] tensors (x, out and idx), M = 131 072 + 77 per head, K = 1000, D = 252, a twin
    codebook per head (one twin in each lane half): rescore entries of head 1 and of the last, partial block; the head / row
    decoding of the entries, the strided idx (candidate words and winners) and out stores, the padded dims."""
    H, M, k, d, mask = 2, 131072 + 77, 1000, 252, 4
    cbs = [_twin_codebook(k, d, mask, seed=70 + h) for h in range(H)]
    pick = torch.randint(0, k, (H, M), generator=torch.Generator().manual_seed(72))
    xf = torch.empty((M, H * d))
    x = xf.view(M, H, d).permute(1, 0, 2)
    rows = _sample(M)
    for h in range(H):
        x[h] = _rows(cbs[h], pick[h], seed=73 + h)
        _prove(x[h, rows], cbs[h], torch.stack([pick[h, rows], pick[h, rows] ^ mask], 1))
    xd = xf.to(DEV).view(M, H, d).permute(1, 0, 2)
    a = _check(xd, torch.stack(cbs)[:, None].to(DEV), oracle, strided=True)
    assert a["idx"].stride() == (1, H, 1) and a["out"].stride() == (d, H * d, 1)
    assert torch.equal(a["idx"][:, :, 0].cpu() | mask, pick | mask)


@functools.lru_cache(maxsize=None)
def _plain():
    """Unrelated codes, rows next to one: every row is certain."""
    g = torch.Generator().manual_seed(81)
    cb = torch.randn((K, D), generator=g) * SCALE
    pick = torch.randint(0, K, (M0,), generator=g)
    return _rows(cb, pick, seed=82)[None].to(DEV), cb[None, None].to(DEV), pick


def test_two_calls_in_a_row_share_no_entries(oracle):
    """Every row rescored, then no uncertain row, with calls of one shape (the allocator hands the second call the first
    call's workspace block): both counts are zeroed per call, so the second call decides none of the first call's entries."""
    x1, cb1 = _twins(4)
    x2, cb2, pick = _plain()
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
    _check(x1, cb1, oracle, a=a1)
    _check(x2, cb2, oracle, a=a2)


def test_graph_replay_on_fresh_inputs(oracle):
    """One screened call captured in a graph (a linear chain: pack, sweep, second pass) and replayed on fresh inputs: the
    counts and the candidate words live on the device only, nothing is read on the host."""
    native = _native()
    mask = 4
    x0, cb = _twins(mask)
    cbh = cb[0, 0].cpu()
    packed = native.pack_codebooks(cb, 0)
    static_x = x0.clone()
    native.quantize(static_x, cb, packed=packed, metric=0, want_best=False)  # warm-up: device info, workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = native.quantize(static_x, cb, packed=packed, metric=0, want_best=False)
    rows = _sample(M0)
    for seed in (91, 92):
        pick = torch.randint(0, K, (M0,), generator=torch.Generator().manual_seed(seed))
        xn = _rows(cbh, pick, seed=seed + 10)
        _prove(xn[rows], cbh, torch.stack([pick[rows], pick[rows] ^ mask], 1))
        static_x.copy_(xn[None])
        g.replay()
        torch.cuda.synchronize()
        a, b = _both(static_x, cb)  # eager: screened and fp32 sweep
        for e in (a, b):
            assert torch.equal(r["idx"], e["idx"])
            assert torch.equal(r["out"].view(torch.int32), e["out"].view(torch.int32))
        _check(static_x, cb, oracle, a=r)
