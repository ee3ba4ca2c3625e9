#!/usr/bin/env python3
"""kernel-level perf of the apply entries (mxa_ld_window_apply: Y = T_w(R) X without the rows) over last[i] = min(i + window, snps - 1), term r2, n in
{1, 16, 64}, both engines, in one process on synthetic device data with device X / Y.  HIP events around the kernels (mxa_profile_get: products, tile kernel,
finish) and around the whole call (torch events).  Two comparison legs, alternating with the apply calls:
  scores   mxa_ld_window_scores (n = 1, X = 1: the same information by the fused epilogue);
  rows     mxa_ld_window_rows (kind r2) to a device buffer, then a device band product of the rows with the same X in torch: per chunk of 1024 rows the band is
           skewed into a dense 1024 x (1024 + window) block (one strided copy) and multiplied from both sides (two fp64 GEMMs) -- what a user does today.
Model printed beside the numbers: one product per window tile, as the pairs entry; 256 KiB of counts per tile slot written once and read ceil(n / 16) times;
4 * 65536 * n flop per full tile; the rows route writes (and reads back) 8 bytes per window element.
usage: perf_ld_apply.py snps indiv window [reps]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import miraculix_amd as mx
from miraculix_amd.crossproduct import ld_window_tiles, LD_APPLY_NC
from bench import synth_plink_device

snps, indiv, window = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
NS = (1, 16, 64)
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr


def timed(fn):
    """(library kernel ms, whole ms by torch events) of one call"""
    L.mxa_profile_reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    la, ms = ctypes.c_int(0), ctypes.c_double(0)
    L.mxa_profile_get(ctypes.byref(la), ctypes.byref(ms))
    return ms.value, e0.elapsed_time(e1)


X = synth_plink_device(torch, snps, (indiv + 3) // 4, 7, dev)
f = torch.rand(snps, dtype=torch.float64, device=dev) * 0.4 + 0.1
last = np.minimum(np.arange(snps) + window, snps - 1).astype(np.int32)
entries = int((last.astype(np.int64) - np.arange(snps) + 1).sum())
ntiles = len(ld_window_tiles(last))
d_last = torch.from_numpy(last).to(dev)
rows = torch.empty(entries, dtype=torch.float64, device=dev)
scores = torch.empty(snps, dtype=torch.float64, device=dev)
nmax = max(NS)
B = torch.randn(nmax, snps, dtype=torch.float64, device=dev)          # column-major snps x nmax
B[0] = 1.0                                                            # column 0 of ones: the scores
Y = torch.empty(nmax, snps, dtype=torch.float64, device=dev)
print(f"apply {snps} SNPs x {indiv} indiv, window {window}: {ntiles} window tiles, {entries} window elements; the rows route writes {8 * entries / 1e9:.2f} GB; "
      f"model: {ntiles * 262144 / 1e9:.2f} GB of counts written once, read ceil(n / {LD_APPLY_NC}) times; {4 * 65536 * ntiles / 1e9:.2f} GFLOP per column", flush=True)


def apply_call(n):
    assert L.mxa_ld_window_apply(P(X), snps, indiv, P(d_last), 1, P(B), snps, n, P(Y), snps, 1, P(f)) == 0, mx.lib.last_error()


def scores_call():
    assert L.mxa_ld_window_scores(P(X), snps, indiv, P(d_last), P(scores), 0, 1, P(f)) == 0, mx.lib.last_error()


def rows_call():
    assert L.mxa_ld_window_rows(P(X), snps, indiv, P(d_last), P(rows), 1, 1, P(f)) == 0, mx.lib.last_error()


CH = 1024
w1 = window + 1
full_rows = snps - window                                             # rows 0 .. full_rows - 1 hold window + 1 entries
Dbuf = torch.zeros(CH * (CH + window), dtype=torch.float64, device=dev)
tail_last = torch.from_numpy(last.astype(np.int64)).to(dev)


def band_product(n):
    """Y (snps x n) = the window's rows (ragged, kind r2) times B[:n]^T, both sides of the diagonal"""
    Xr = torch.zeros(snps + window, n, dtype=torch.float64, device=dev)
    Xr[:snps] = B[:n].t()
    Yr = torch.zeros(snps + window, n, dtype=torch.float64, device=dev)
    for i0 in range(0, snps, CH):
        c = min(CH, snps - i0)
        Lw = c + window
        if i0 + c <= full_rows:
            chunk = rows[i0 * w1: (i0 + c) * w1].view(c, w1)
        else:                                                         # the ragged tail: padded with zeros
            i = torch.arange(i0, i0 + c, device=dev)
            mask = torch.arange(w1, device=dev)[None, :] <= (tail_last[i0: i0 + c] - i)[:, None]
            chunk = torch.zeros(c, w1, dtype=torch.float64, device=dev)
            start = i0 * w1 if i0 <= full_rows else full_rows * w1 + sum(int(last[k]) - k + 1 for k in range(full_rows, i0))
            chunk[mask] = rows[start: start + int(mask.sum())]
        D = Dbuf[: c * Lw]
        D.zero_()
        skew = D.as_strided((c, w1), (Lw + 1, 1))                     # skew[i, d] = D[i, i + d]
        skew.copy_(chunk)
        Dm = D.view(c, Lw)
        Yr[i0: i0 + c] += Dm @ Xr[i0: i0 + Lw]                        # j >= i
        skew[:, 0] = 0.0                                              # the diagonal counts once
        Yr[i0: i0 + Lw] += Dm.t() @ Xr[i0: i0 + c]                    # j < i: the pair (j, i)
    return Yr[:snps]


def med(v):
    k = sorted(v)
    return k[len(k) // 2], k[0], k[-1]


for engine in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = engine
    legs = {f"apply n={n}": (lambda n=n: apply_call(n)) for n in NS}
    legs["scores"] = scores_call
    legs["rows"] = rows_call
    for n in NS:
        legs[f"rows + band product n={n}"] = (lambda n=n: (rows_call(), band_product(n)))
    for fn in legs.values():
        timed(fn)                                                     # warm-up: code objects, allocator
    res = {k: [] for k in legs}
    for _ in range(reps):                                             # alternating
        for k, fn in legs.items():
            res[k].append(timed(fn))
    m = {}
    for k in legs:
        km, kmin, kmax = med([r[0] for r in res[k]])
        wm, wmin, wmax = med([r[1] for r in res[k]])
        m[k] = (km, wm)
        print(f"{engine} {k}: library kernels {km:.2f} ms median of {reps} (min {kmin:.2f}, max {kmax:.2f}); whole {wm:.2f} ms (min {wmin:.2f}, max {wmax:.2f}); "
              f"{km / ntiles * 1e3:.2f} us per tile", flush=True)
    print(f"{engine}: apply n=1 / scores: kernels {m['apply n=1'][0] / m['scores'][0]:.3f}, whole {m['apply n=1'][1] / m['scores'][1]:.3f}", flush=True)
    for n in NS:
        print(f"{engine}: apply n={n} / (rows + band product n={n}): whole {m[f'apply n={n}'][1] / m[f'rows + band product n={n}'][1]:.3f}; "
              f"apply at {4 * 65536 * ntiles * n / m[f'apply n={n}'][0] / 1e9:.2f} TFLOP/s of the model's flop", flush=True)
# the two routes agree (kind r2, the last engine's results): column 0 against the scores, all columns against the band product
apply_call(nmax)
torch.cuda.synchronize()
Yb = band_product(nmax)
scores_call()
torch.cuda.synchronize()
scale = float(Yb.abs().max())
print(f"agreement: max |apply - band product| / max |Y| = {float((Y.t() - Yb).abs().max()) / scale:.2e}; max |apply column 0 - scores| / max = "
      f"{float((Y[0] - scores).abs().max() / scores.abs().max()):.2e}", flush=True)
