#!/usr/bin/env python3
"""kernel-level perf of the windowed LD entries over a window given as data (mxa_ld_window_rows / mxa_ld_window_scores) against the fixed entries
(mxa_ld_band / mxa_ld_scores) of the same build, in one process, on synthetic device data with device results.  HIP events around the tile launches and the
tail / finish kernel (mxa_profile_get); the calls alternate.  Both engines.
 1. last[i] = min(i + window, snps - 1): the same tiles as the fixed entries; the difference is two cached loads per stored row.  Per entry median, min and max,
    so that the difference can be read against the run-to-run spread of the fixed entries in this run.
 2. a synthetic density profile -- positions whose local spacing varies smoothly by 1 : 25, max_dist searched so that the mean reach is `window` (the
    largest about four times that): tiles, stored entries, and the time per tile against 1.
usage: perf_ld_window_var.py snps indiv window [reps]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import miraculix_amd as mx
from miraculix_amd.crossproduct import ld_band_tiles, ld_window_bounds, ld_window_tiles
from bench import synth_plink_device

snps, indiv, window = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr


def kernel_ms(fn):
    L.mxa_profile_reset()
    assert fn() == 0, mx.lib.last_error()
    torch.cuda.synchronize()
    la, ms = ctypes.c_int(0), ctypes.c_double(0)
    L.mxa_profile_get(ctypes.byref(la), ctypes.byref(ms))
    return ms.value


def density_window():
    """positions with a smoothly varying density; max_dist by bisection on the mean reach"""
    i = np.arange(snps, dtype=np.float64)
    dens = 0.2 + 4.8 * (0.5 + 0.5 * np.sin(2.0 * np.pi * i / 60000.0)) ** 6
    pos = np.cumsum(1.0 / dens)
    lo, hi = 0.0, float(pos[-1])
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        last, _ = ld_window_bounds(pos, None, max_dist=mid)
        if (last - np.arange(snps)).mean() < window:
            lo = mid
        else:
            hi = mid
    return ld_window_bounds(pos, None, max_dist=hi)


X = synth_plink_device(torch, snps, (indiv + 3) // 4, 7, dev)
f = torch.rand(snps, dtype=torch.float64, device=dev) * 0.4 + 0.1
fixed_last = np.minimum(np.arange(snps) + window, snps - 1).astype(np.int32)
fixed_total = int((fixed_last.astype(np.int64) - np.arange(snps) + 1).sum())
var_last, var_rowptr = density_window()
reach = var_last - np.arange(snps)
nt_fixed, nt_var = len(ld_band_tiles(snps, window)), len(ld_window_tiles(var_last))
assert len(ld_window_tiles(fixed_last)) == nt_fixed
print(f"windowed LD over last[] {snps} SNPs x {indiv} indiv: fixed window {window}: {nt_fixed} tiles, {fixed_total} entries; density profile: reach mean {reach.mean():.0f} "
      f"min {reach.min()} max {reach.max()}, {nt_var} tiles, {int(var_rowptr[-1])} entries", flush=True)
band = torch.empty((snps, window + 1), dtype=torch.float64, device=dev)
rows = torch.empty(max(fixed_total, int(var_rowptr[-1])), dtype=torch.float64, device=dev)
scores = torch.empty(snps, dtype=torch.float64, device=dev)
d_fixed, d_var = torch.from_numpy(fixed_last).to(dev), torch.from_numpy(var_last).to(dev)
calls = {
    "mxa_ld_band r": (lambda: L.mxa_ld_band(P(X), snps, indiv, window, P(band), window + 1, 0, 1, P(f)), nt_fixed),
    "mxa_ld_window_rows r, fixed last": (lambda: L.mxa_ld_window_rows(P(X), snps, indiv, P(d_fixed), P(rows), 0, 1, P(f)), nt_fixed),
    "mxa_ld_window_rows r, density profile": (lambda: L.mxa_ld_window_rows(P(X), snps, indiv, P(d_var), P(rows), 0, 1, P(f)), nt_var),
    "mxa_ld_scores": (lambda: L.mxa_ld_scores(P(X), snps, indiv, window, P(scores), 0, 1, P(f)), nt_fixed),
    "mxa_ld_window_scores, fixed last": (lambda: L.mxa_ld_window_scores(P(X), snps, indiv, P(d_fixed), P(scores), 0, 1, P(f)), nt_fixed),
    "mxa_ld_window_scores, density profile": (lambda: L.mxa_ld_window_scores(P(X), snps, indiv, P(d_var), P(scores), 0, 1, P(f)), nt_var),
}
names = list(calls)
for engine in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = engine
    for fn, _ in calls.values():
        kernel_ms(fn)                                                    # warm-up: code objects, allocator
    res = {n: [] for n in names}
    for _ in range(reps):                                                # alternating
        for n in names:
            res[n].append(kernel_ms(calls[n][0]))
    med = {}
    for n in names:
        k = sorted(res[n])
        med[n] = k[len(k) // 2]
        print(f"{engine} {n}: kernel {med[n]:.2f} ms median of {reps} (min {k[0]:.2f}, max {k[-1]:.2f}); {med[n] / calls[n][1] * 1e3:.2f} us per tile", flush=True)
    for base in (0, 3):
        a, b, c = names[base], names[base + 1], names[base + 2]
        print(f"{engine} ratio {b} / {a}: {med[b] / med[a]:.3f};  per tile {c} / {b}: {(med[c] / calls[c][1]) / (med[b] / calls[b][1]):.3f}", flush=True)
