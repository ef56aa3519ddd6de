"""GPU: the caller-cached screen image of the screened Dp = 256 sweep and the split full searches of its second pass.

A call that is handed the image of ``native.pack_screen`` launches no pack kernel; the image ends in a control block (the two
list counts, an exit ticket, the previous call's counts, a ticket and result slots per split full-search row) that
vq_resolve_rows_kernel leaves clean for the next call.  When the full-search rows are at most half the grid, each row's codes
are split over several workgroups and the last one to finish combines their results.

Every case compares idx and the quantized rows bit for bit among the call with the cached image, the call without one and
the fp32 sweep (VQ_NO_SCREEN, read per call), a row sample (every constructed row included) with the CPU oracle, and reads
the control block back: words 0..2 and every row ticket are zero, words 4 and 5 hold the constructed list lengths -- the
proof that the intended path ran.

The list lengths are steered by construction (tests/test_gpu_screened_rescore.py proves these constructions in fp64): codes
are randn * 8 and an ordinary row is a code + 0.5 * randn, which the screen decides on its own.  A row goes to the full-search
list when it holds a NaN or an inf, or when it sits next to code 0, which has near copies at indices 1 and 2 (three
candidates in one lane half: more than a half tracks); it goes to the rescore list when it sits next to code 8, which has one
near copy at index 9.

M = 131 072 is the smallest row count at which the persistent kernel runs at K = 1024 on 256 CUs."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M0 = 131072
SCALE, NOISE, EPS = 8.0, 0.5, 2e-3
CTRL_BYTES = 16384                 # kScrCtrlBytes
ROW_TICKETS = slice(8, 8 + 160)    # kScrRowTicketWord, kResolveMaxSplitRows


def _native():
    from vector_quantization import native

    native.load()
    return native


def _grid():
    return torch.cuda.get_device_properties(0).multi_processor_count  # workgroups of vq_resolve_rows_kernel


@functools.lru_cache(maxsize=None)
def _base(H, M, K, D):
    """Codebooks [H, 1, K, D] with the near copies, ordinary rows [H, M, D] next to codes 16 .. K - 1, and the image."""
    g = torch.Generator().manual_seed(1000 * H + K + D)
    cb = torch.randn((H, K, D), generator=g) * SCALE
    for h in range(H):
        for src, dst, j in ((0, 1, 1), (0, 2, 2), (8, 9, 1)):
            cb[h, dst] = cb[h, src]
            cb[h, dst, (src + j) % D] += j * EPS
    cb = cb.to(DEV)
    gd = torch.Generator(device=DEV).manual_seed(7)
    pick = torch.randint(16, K, (H, M), generator=gd, device=DEV)
    x = cb[torch.arange(H, device=DEV)[:, None], pick] + NOISE * torch.randn((H, M, D), generator=gd, device=DEV)
    cb4 = cb[:, None].contiguous()
    native = _native()
    packed = native.pack_codebooks(cb4, native.EUCLID)
    screen = native.pack_screen(packed, H, K, D, native.EUCLID)
    assert screen is not None and screen.numel() == native.screen_image_bytes(H, K, D, native.EUCLID)
    return x, cb4, packed, screen


def _rows_for(x, cb4, n_full, n_rescore, limit):
    """A copy of x with n_full full-search rows and n_rescore rescore rows among the first `limit` rows of the heads
    (spread over them), at fixed pseudo-random places.  -> (x, the constructed (head, row) pairs)."""
    H, M, D = x.shape
    x = x.clone()
    g = torch.Generator().manual_seed(n_full * 31 + n_rescore)
    where = torch.randperm(H * limit, generator=g)[:n_full + n_rescore]
    hh, rr = (where // limit).to(DEV), (where % limit).to(DEV)
    gd = torch.Generator(device=DEV).manual_seed(n_full + 3 * n_rescore + 1)
    noise = NOISE * torch.randn((n_full + n_rescore, D), generator=gd, device=DEV)
    kinds = torch.arange(n_full, device=DEV) % 4  # next to the triplicated code, NaN, +inf, -inf
    full = cb4[hh[:n_full], 0, 0] + noise[:n_full]
    full[kinds == 1, 3] = float("nan")
    full[kinds == 2, D - 1] = float("inf")
    full[kinds == 3, 0] = -float("inf")
    x[hh[:n_full], rr[:n_full]] = full
    x[hh[n_full:], rr[n_full:]] = cb4[hh[n_full:], 0, 8] + noise[n_full:]
    return x, (hh.cpu(), rr.cpu())


def _ctrl(screen):
    torch.cuda.synchronize()
    return screen[-CTRL_BYTES:].view(torch.int32).cpu().numpy().view(np.uint32)


def _assert_clean(screen, counts=None):
    c = _ctrl(screen)
    assert (c[0:3] == 0).all(), c[:8]
    assert (c[ROW_TICKETS] == 0).all(), np.nonzero(c[ROW_TICKETS])
    if counts is not None:
        assert (int(c[4]), int(c[5])) == tuple(counts), (c[:8], counts)


def _three_ways(x, cb4, packed, screen):
    native = _native()
    a = native.quantize(x, cb4, packed=packed, screen=screen, want_best=False)
    b = native.quantize(x, cb4, packed=packed, want_best=False)
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        c = native.quantize(x, cb4, packed=packed, want_best=False)
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    for r in (a, b):
        assert torch.equal(r["idx"], c["idx"])
        assert torch.equal(r["out"].view(torch.int32), c["out"].view(torch.int32))
    return a


def _check_oracle(oracle, x, cb4, res, special):
    H, M, _ = x.shape
    hh, rr = special
    keep = torch.randperm(hh.numel(), generator=torch.Generator().manual_seed(5))[:150]
    for h in range(H):
        rows = torch.cat([rr[keep][hh[keep] == h], torch.randperm(M, generator=torch.Generator().manual_seed(3))[:50],
                          torch.arange(M - 5, M)])
        ri, _ = oracle.nearest(x[h, rows].cpu().numpy(), cb4[h, 0].cpu().numpy(), 0)
        np.testing.assert_array_equal(res["idx"][h, rows, 0].cpu().numpy(), ri)


def _list_lengths():
    g = _grid()
    # (full-search rows, rescore rows): none / one / two rows, around half the grid (the split's threshold), more than the
    # grid; batches of 16 rescore rows: 0, 1, 15, 16, 17, thousands; (2, 40 000): too many batches for the free workgroups
    # of a split, so S = 1 although the rows are few; (74, 9 000): the headline call's lengths
    return [(0, 0), (1, 0), (0, 1), (2, 15), (g // 2 - 1, 16), (g // 2, 17), (g // 2 + 1, 5000), (g + 50, 5000), (74, 9000), (2, 40000),
            (1, 3000)]


@pytest.mark.parametrize("case", range(11))
def test_list_lengths_cached_uncached_fp32(oracle, case):
    n_full, n_rescore = _list_lengths()[case]
    x0, cb4, packed, screen = _base(1, M0, 1024, 256)
    x, special = _rows_for(x0, cb4, n_full, n_rescore, M0)
    res = _three_ways(x, cb4, packed, screen)
    _assert_clean(screen, (n_full, n_rescore))
    _check_oracle(oracle, x, cb4, res, special)


def test_unsplit_switch_gives_the_same_rows():
    """VQ_RESOLVE_NO_SPLIT (read per call): one workgroup per full-search row whatever the counts."""
    x0, cb4, packed, screen = _base(1, M0, 1024, 256)
    x, _ = _rows_for(x0, cb4, 74, 9000, M0)
    os.environ["VQ_RESOLVE_NO_SPLIT"] = "1"
    try:
        _three_ways(x, cb4, packed, screen)
    finally:
        os.environ.pop("VQ_RESOLVE_NO_SPLIT", None)
    _assert_clean(screen, (74, 9000))


@pytest.mark.parametrize("H,M,K,D,n_full,n_rescore", [
    (1, M0 + 37, 1030, 132, 3, 40),        # ragged rows (the 37 run as a call of their own), padding codes, D % 32 != 0
    (1, M0 + 37, 1030, 132, 100, 1000),    # K = 1030: three passes per wave unsplit, S = 2 where the grid allows
    (1, M0, 1030, 256, 20, 17),            # few rows at K = 1030: S = 3 (one pass per wave)
    (2, M0 // 2, 1024, 256, 5, 100),       # two heads: entries head * M + row, one image per head, one control block
    (2, M0 // 2 + 37, 1024, 132, 41, 999),
])
def test_shapes(oracle, H, M, K, D, n_full, n_rescore):
    x0, cb4, packed, screen = _base(H, M, K, D)
    x, special = _rows_for(x0, cb4, n_full, n_rescore, M - 37 if M % 256 else M)
    x[:, M - 1, 1] = float("nan")  # the last row of every head (with a ragged M it is not in the screened part)
    res = _three_ways(x, cb4, packed, screen)
    ragged = M % 256 != 0
    _assert_clean(screen, (n_full + (0 if ragged else H), n_rescore))
    _check_oracle(oracle, x, cb4, res, special)


def test_three_calls_on_one_image_long_short_none(oracle):
    """No synchronisation and no other call between them: a count or a ticket that was not cleaned would be the next
    call's."""
    native = _native()
    x0, cb4, packed, screen = _base(1, M0, 1024, 256)
    g = _grid()
    xs = [_rows_for(x0, cb4, nf, nr, M0)[0] for nf, nr in ((g + 50, 5000), (3, 2), (0, 0))]
    got = [native.quantize(x, cb4, packed=packed, screen=screen, want_best=False) for x in xs]
    _assert_clean(screen, (0, 0))
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        want = [native.quantize(x, cb4, packed=packed, want_best=False) for x in xs]
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    for a, b in zip(got, want):
        assert torch.equal(a["idx"], b["idx"])
        assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32))


def test_a_foreign_image_is_an_error():
    native = _native()
    x, cb4, packed, screen = _base(1, M0, 1024, 256)
    with pytest.raises(RuntimeError, match="screen"):
        native.quantize(x, cb4, packed=packed, screen=screen[:-256], want_best=False)
    # calls the screened sweep does not take ignore the image: distances requested, the dot metric's packed image
    a = native.quantize(x, cb4, packed=packed, screen=screen, want_best=True)
    b = native.quantize(x, cb4, packed=packed, want_best=True)
    assert torch.equal(a["idx"], b["idx"]) and torch.equal(a["best"].view(torch.int32), b["best"].view(torch.int32))
    _assert_clean(screen)


# ------------------------------------------------------------------------------------------------ the module
def _module(seed=11):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    mod = vq.VectorQuantize(dim=256, codebook_params=CodebookParams(dim=256, codebook_size=1024))
    with torch.no_grad():
        mod._codebook.embeddings.copy_(torch.randn(mod._codebook.embeddings.shape, generator=torch.Generator().manual_seed(seed)))
    return mod.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _batch():
    return torch.randn((128, 1024, 256), generator=torch.Generator(device=DEV).manual_seed(12), device=DEV)


def _reference(mod, x):
    """The module's forward with the fp32 sweep."""
    os.environ["VQ_NO_SCREEN"] = "1"
    try:
        with torch.no_grad():
            q, i, _ = mod(x)
    finally:
        os.environ.pop("VQ_NO_SCREEN", None)
    return q.clone(), i.clone()


def _same(got, want):
    return torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


def test_module_repeats_and_follows_in_place_weights():
    mod, x = _module(), _batch()
    want = _reference(mod, x)
    with torch.no_grad():
        for _ in range(3):
            q, i, _ = mod(x)
            assert _same((q, i), want)
    book = mod._codebook
    assert len(book._screen) == 1 and next(iter(book._screen.values())) is not None
    first = next(iter(book._screen.values()))
    with torch.no_grad():
        book.embeddings.copy_(torch.randn(book.embeddings.shape, generator=torch.Generator().manual_seed(13)).to(DEV))
        q, i, _ = mod(x)
    want2 = _reference(mod, x)
    assert _same((q, i), want2) and not torch.equal(want2[1], want[1])
    assert next(iter(book._screen.values())) is not first  # the image was rebuilt from the new codes
    _assert_clean(next(iter(book._screen.values())))


def test_module_two_streams_two_images():
    mod, x = _module(), _batch()
    want = _reference(mod, x)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    got = []
    with torch.no_grad():
        for s in streams:
            with torch.cuda.stream(s):
                q, i, _ = mod(x)
                got.append((q, i))
    torch.cuda.synchronize()
    images = [mod._codebook._screen[s.cuda_stream] for s in streams]  # (the current stream is the key)
    assert images[0].data_ptr() != images[1].data_ptr()
    assert all(_same(g, want) for g in got)
    for img in images:
        _assert_clean(img)


def test_graphed_forward_reads_the_weights_of_its_replay():
    from vector_quantization.graphs import GraphedForward

    mod, x = _module(), _batch()
    fast = GraphedForward(mod, x)
    with torch.no_grad():
        mod._codebook.embeddings.copy_(torch.randn(mod._codebook.embeddings.shape, generator=torch.Generator().manual_seed(14)).to(DEV))
    q, i, _ = fast(x)
    torch.cuda.synchronize()
    got = (q.clone(), i.clone())
    assert _same(got, _reference(mod, x))
    with torch.no_grad():  # and the eager module beside the graph
        q, i, _ = mod(x)
    assert _same((q, i), got)


def test_second_eval_forward_launches_no_pack_kernel():
    from torch.profiler import ProfilerActivity, profile

    mod, x = _module(), _batch()
    with torch.no_grad():
        mod(x)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            mod(x)
            torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and "vq_" in ev.name]
    if not names:
        pytest.skip("torch.profiler reported no device activity on this build")
    assert not any("vq_pack" in n for n in names), names
    assert sum("vq_search_persist" in n and "true>" in n for n in names) == 1, names
    assert sum("vq_resolve_rows_kernel" in n for n in names) == 1, names
