#!/usr/bin/env python3
"""kernel-level perf of the pairwise-complete windowed LD entries (mxa_ld_band_pairwise / mxa_ld_scores_pairwise) against mxa_ld_band / mxa_ld_scores of the same
build, in one process, on synthetic device data with device results: the pairwise entries on genotypes with `missing` of the fields set to the missing code
01 (six products per band tile) and on the same genotypes without it (fast path: one product), the plain entries on the genotypes without it.  The calls
alternate; per entry the kernel time (HIP events around the tile launches, combines and tail / finish kernel: mxa_profile_get) and the call's wall time
(staging included), then the ratios pairwise / plain.  Both engines.
usage: perf_ld_pairwise.py snps indiv window [reps] [missing]"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import miraculix_amd as mx
from miraculix_amd.crossproduct import ld_band_tiles, ld_pairwise_group_rows
from bench import synth_plink_device

snps, indiv, window = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
missing = float(sys.argv[5]) if len(sys.argv) > 5 else 0.05
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr


def with_missing(X, frac, seed):
    """a copy of X in which every field is replaced by 01 with probability frac (padding fields of the last byte excluded); in chunks"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = X.clone()
    rb = X.shape[1]
    chunk = max(1, (64 << 20) // max(1, rb))
    for r0 in range(0, X.shape[0], chunk):
        b = out[r0:r0 + chunk]
        for q in range(4):
            m = torch.rand(b.shape, device=dev, generator=g) < frac
            if indiv % 4 and q >= indiv % 4:
                m[:, -1] = False
            b[:] = torch.where(m, (b & (0xFF ^ (3 << (2 * q)))) | (1 << (2 * q)), b)
    return out


def timed(fn):
    """one call: (kernel ms by the library's events, wall ms)"""
    L.mxa_profile_reset()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    assert fn() == 0, mx.lib.last_error()
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    la, ms = ctypes.c_int(0), ctypes.c_double(0)
    L.mxa_profile_get(ctypes.byref(la), ctypes.byref(ms))
    return ms.value, wall * 1e3


X = synth_plink_device(torch, snps, (indiv + 3) // 4, 7, dev)
if indiv % 4:
    X[:, -1] &= (1 << (2 * (indiv % 4))) - 1
Xm = with_missing(X, missing, 8)
f = torch.rand(snps, dtype=torch.float64, device=dev) * 0.4 + 0.1
band = torch.empty((snps, window + 1), dtype=torch.float64, device=dev)
scores = torch.empty(snps, dtype=torch.float64, device=dev)
ntiles = len(ld_band_tiles(snps, window))
nb = (snps + 255) // 256
rows6, rows1 = ld_pairwise_group_rows(snps, window), ld_pairwise_group_rows(snps, window, pairs=1)
print(f"pairwise-complete windowed LD {snps} SNPs x {indiv} indiv, window {window}, {missing:.0%} missing: {ntiles} band tiles; six products: {-(-nb // rows6)} groups of "
      f"{rows6} tile rows, {6 * ntiles * 262144 * 2 / 1e9:.1f} GB of counts written and read; fast path: {-(-nb // rows1)} group(s)", flush=True)
calls = {
    "mxa_ld_band r (no missing)": lambda: L.mxa_ld_band(P(X), snps, indiv, window, P(band), window + 1, 0, 1, P(f)),
    f"mxa_ld_band_pairwise r ({missing:.0%} missing)": lambda: L.mxa_ld_band_pairwise(P(Xm), snps, indiv, window, P(band), window + 1, 0),
    "mxa_ld_band_pairwise r (no missing)": lambda: L.mxa_ld_band_pairwise(P(X), snps, indiv, window, P(band), window + 1, 0),
    "mxa_ld_scores (no missing)": lambda: L.mxa_ld_scores(P(X), snps, indiv, window, P(scores), 0, 1, P(f)),
    f"mxa_ld_scores_pairwise ({missing:.0%} missing)": lambda: L.mxa_ld_scores_pairwise(P(Xm), snps, indiv, window, P(scores), 0),
    "mxa_ld_scores_pairwise (no missing)": lambda: L.mxa_ld_scores_pairwise(P(X), snps, indiv, window, P(scores), 0),
}
names = list(calls)
for engine in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = engine
    for fn in calls.values():
        timed(fn)                                                        # warm-up: code objects, allocator
    res = {n: [] for n in names}
    for _ in range(reps):                                                # alternating
        for n in names:
            res[n].append(timed(calls[n]))
    med = {}
    for n in names:
        k, w = sorted(r[0] for r in res[n]), sorted(r[1] for r in res[n])
        med[n] = k[len(k) // 2]
        print(f"{engine} {n}: kernel {med[n]:.2f} ms median of {reps} (min {k[0]:.2f}, max {k[-1]:.2f}); call wall {w[len(w) // 2]:.1f} ms median", flush=True)
    for base in (0, 3):
        print(f"{engine} ratio {names[base + 1]} / {names[base]}: {med[names[base + 1]] / med[names[base]]:.2f};  {names[base + 2]} / {names[base]}: "
              f"{med[names[base + 2]] / med[names[base]]:.2f}", flush=True)
