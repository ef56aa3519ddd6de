"""Diagnostic: where the waves of the persistent Dp = 256 kernel (vq_search_persist) spend their lives, per row block
(in-kernel s_memtime stamps: block start, prologue end, sweep end, resolve end; the open finalize's end once per wave).

Build the diagnostic library first, as ONE translation unit (the multi-part build keeps a copy of the stamp array per part
and the read-back would return the all-zero copy of part 0):
    VQ_BUILD_SINGLE=1 VQ_EXTRA_FLAGS=-DVQ_EXP_STAMPS VQ_LIB_OUT=lib/stamps.so ./build.sh
then  VQ_MI355X_LIB=.../lib/stamps.so python tools/stamps_persist.py [M,K,D]
Without an argument the data is bench.py's headline workload (cfg2: 262144 x 256 rows of seed 1234, 1024 codes of seed 4321);
with one, randn of seed 0.  VQ_NO_SCREEN=1 in the environment stamps the fp32 sweep of the same kernel.
The screened sweep also stamps, per wave, six sub-tiles (12 .. 17) of row block 2: barrier release, start and end of the
epilogue, barrier arrival.  Reported for waves 0-3 and 4-7 (SIMD partners w, w + 4): epilogue and sub-tile lengths and how
much the partners' epilogue intervals overlap.  VQ_NO_STAGGER=1 puts all eight waves' epilogues at the same place.
"""
import sys, os, ctypes, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-quantization-by-ml_amd")]
import torch, numpy as np
from vector_quantization import native
dev = torch.device("cuda:0")
if len(sys.argv) > 1:
    M, K, D = [int(v) for v in sys.argv[1].split(",")]
    g = torch.Generator().manual_seed(0)
    x = torch.randn((1, M, D), generator=g).to(dev); cb = torch.randn((1, 1, K, D), generator=g).to(dev)
else:
    M, K, D = 262144, 1024, 256
    x = torch.randn((256, 1024, 256), generator=torch.Generator().manual_seed(1234)).reshape(1, M, D).to(dev)
    cb = torch.randn((1, K, D), generator=torch.Generator().manual_seed(4321)).reshape(1, 1, K, D).to(dev)
packed = native.pack_codebooks(cb, 0)
t_s = time.perf_counter()
while time.perf_counter() - t_s < 0.1:  # the stamps of the LAST call are read: by then the clock has settled
    for _ in range(5):
        native.quantize(x, cb, packed=packed, want_best=False)
    torch.cuda.synchronize()
lib = native.load()
NST, NB = 64, 8
buf = (ctypes.c_uint64 * (8192 * NST))()
lib.vq_debug_read_stamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
rc = lib.vq_debug_read_stamps(buf, 8192 * NST)
st = np.frombuffer(buf, dtype=np.uint64).reshape(8192, NST).astype(np.int64)
st = st[st[:, 57] > 0]
if rc != 0 or len(st) == 0 or len(st) % 8:
    sys.exit(f"rc {rc}, {len(st)} stamped waves: not a VQ_EXP_STAMPS single-unit build, or the persistent kernel did not run")
nb = np.minimum(st[:, 57], NB)
print(f"M,K,D = {M},{K},{D}   waves {len(st)}   workgroups {len(st) // 8}   blocks per workgroup min/median/max "
      f"{st[:, 57].min()}/{int(np.median(st[:, 57]))}/{st[:, 57].max()}")


def row(name, a):
    a = np.asarray(a, dtype=np.float64)
    print(f"{name:34s} median {np.median(a):9.0f}  p10 {np.percentile(a, 10):9.0f}  p90 {np.percentile(a, 90):9.0f}  max {a.max():9.0f}")
    return np.median(a)


print("cycles per wave and row block (shader clock):")
ph = {"prologue": [], "sweep": [], "resolve": []}
for it in range(int(nb.max())):
    s = st[nb > it][:, 4 * it:4 * it + 4]
    ph["prologue"].append(s[:, 1] - s[:, 0]); ph["sweep"].append(s[:, 2] - s[:, 1]); ph["resolve"].append(s[:, 3] - s[:, 2])
    row(f"  block {it}: prologue", ph["prologue"][-1]); row(f"  block {it}: sweep", ph["sweep"][-1])
    row(f"  block {it}: resolve", ph["resolve"][-1])
sweep_med = 0.0
for k in ("prologue", "sweep", "resolve"):
    m = row(f"all blocks: {k}", np.concatenate(ph[k]))
    if k == "sweep":
        sweep_med = m
last = st[np.arange(len(st)), 4 * (nb - 1) + 3]
row("open finalize (last resolve -> end)", st[:, 56] - last)
# a workgroup's life: first start to last end over its 8 waves
wg = st.reshape(-1, 8, NST)
life = wg[:, :, 56].max(axis=1) - wg[:, :, 0].min(axis=1)
med = row("workgroup life (first start -> last end)", life)
print(f"slowest workgroup trails the median by {life.max() - med:.0f} cycles = {100.0 * (life.max() - med) / med:.2f} % of the median life")
print(f"workgroups whose life exceeds the median by more than one sweep ({sweep_med:.0f} cycles): {int((life > med + sweep_med).sum())}"
      f"   by more than 3 %: {int((life > 1.03 * med).sum())}")
wres = np.zeros(len(wg))
for it in range(int(nb.max())):
    ok = (wg[:, 0, 57] > it)
    wres[ok] += (wg[ok][:, :, 4 * it + 3] - wg[ok][:, :, 4 * it + 2]).max(axis=1)
row("per workgroup: sum over blocks of its slowest wave's resolve", wres)
# screened sweep, sub-tiles 12 .. 17 of block 2: barrier release, epilogue start / end, barrier arrival per wave (slots 32 ..)
sub = wg[(wg[:, :, 57].min(axis=1) > 2) & (wg[:, :, 32:56].min(axis=(1, 2)) > 0)][:, :, 32:56].reshape(-1, 8, 6, 4)
if len(sub):
    print(f"sub-tiles 12..17 of block 2, {len(sub)} workgroups (VQ_NO_STAGGER {'set' if os.environ.get('VQ_NO_STAGGER') else 'unset'}):")
    for name, ws in (("waves 0-3", slice(0, 4)), ("waves 4-7", slice(4, 8))):
        s = sub[:, ws]
        row(f"  {name}: epilogue length", s[..., 2] - s[..., 1])
        row(f"  {name}: release -> epilogue start", s[..., 1] - s[..., 0])
        row(f"  {name}: epilogue end -> arrival", s[..., 3] - s[..., 2])
        row(f"  {name}: release -> arrival", s[..., 3] - s[..., 0])
        row(f"  {name}: sub-tile (release to release)", s[:, :, 1:, 0] - s[:, :, :-1, 0])
    # SIMD partners w and w + 4: how much of one's epilogue interval lies inside the other's
    a, b = sub[:, 0:4], sub[:, 4:8]
    ov = np.maximum(0, np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 1], b[..., 1]))
    row("  partners' epilogues overlap (cycles)", ov)
    row("  ... in % of the early half's epilogue", 100.0 * ov / np.maximum(a[..., 2] - a[..., 1], 1))
    row("  ... in % of the late half's epilogue", 100.0 * ov / np.maximum(b[..., 2] - b[..., 1], 1))
    row("  barrier wait (arrival -> next release)", sub[:, :, 1:, 0] - sub[:, :, :-1, 3])
rt = (st[:, 61] - st[:, 60]).astype(np.float64)
clk = np.median((st[:, 56] - st[:, 0]) / np.maximum(rt, 1.0)) * 100.0
print(f"wave life: median {np.median(rt) / 100:.1f} us, max {rt.max() / 100:.1f} us; first start .. last end of the launch: "
      f"{(st[:, 61].max() - st[:, 60].min()) / 100:.1f} us; s_memtime ticks per us: {clk:.0f}")
