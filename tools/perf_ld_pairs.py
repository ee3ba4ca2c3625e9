#!/usr/bin/env python3
"""kernel-level perf of the CSR entries (mxa_ld_window_pairs / mxa_ld_window_pairs_pairwise: the pairs with r^2 >= min_r2, compacted on the device) against the
rows entries (mxa_ld_window_rows / mxa_ld_window_rows_pairwise) over the same last[i] = min(i + window, snps - 1), in one process, on synthetic device data with
device results.  HIP events around the products plus the selection (mxa_profile_get); the calls alternate.  Both engines.  Three data sets: the plain route;
the pairwise route with 5 % missing (six products per window tile); the pairwise route without a missing code (one product plus per-SNP sums).
Model printed beside the numbers: one product per window tile plus 256 KiB per tile slot, written once and read twice (count pass, write pass; the count-only
call reads it once); the rows entry writes 8 bytes per window element.
usage: perf_ld_pairs.py snps indiv window min_r2 [reps]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import miraculix_amd as mx
from miraculix_amd.crossproduct import ld_window_tiles
from bench import synth_plink_device

snps, indiv, window, min_r2 = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4])
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
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


def with_missing(X, frac):
    """code 01 in `frac` of the fields"""
    out = X.clone()
    for q in range(4):
        hit = torch.rand(X.shape, device=dev) < frac
        out = torch.where(hit, (out & ~(3 << (2 * q))) | (1 << (2 * q)), out)
    return out


def no_missing(X):
    """every 01 field becomes 00"""
    out = X.clone()
    for q in range(4):
        f = (out >> (2 * q)) & 3
        out = torch.where(f == 1, out & ~(3 << (2 * q)), out)
    return out


X = synth_plink_device(torch, snps, (indiv + 3) // 4, 7, dev)
data = {"plain": X, "pairwise, 5 % missing": with_missing(no_missing(X), 0.05), "pairwise, no missing code": no_missing(X)}
f = torch.rand(snps, dtype=torch.float64, device=dev) * 0.4 + 0.1
last = np.minimum(np.arange(snps) + window, snps - 1).astype(np.int32)
entries = int((last.astype(np.int64) - np.arange(snps) + 1).sum())
ntiles = len(ld_window_tiles(last))
d_last = torch.from_numpy(last).to(dev)
rows = torch.empty(entries, dtype=torch.float64, device=dev)
rowptr = torch.empty(snps + 1, dtype=torch.int64, device=dev)
total = ctypes.c_long(0)
print(f"pairs as CSR {snps} SNPs x {indiv} indiv, window {window}, min_r2 {min_r2}: {ntiles} window tiles, {entries} window elements; the rows entry writes "
      f"{8 * entries / 1e9:.2f} GB; the count scratch moves {ntiles * 262144 / 1e9:.2f} GB per product slot, written once and read twice", flush=True)


def pairs_call(name, Xd, col, val, cap):
    if name == "plain":
        return L.mxa_ld_window_pairs(P(Xd), snps, indiv, P(d_last), min_r2, 1, P(rowptr), P(col), P(val), cap, ctypes.byref(total), 1, P(f))
    return L.mxa_ld_window_pairs_pairwise(P(Xd), snps, indiv, P(d_last), min_r2, 1, P(rowptr), P(col), P(val), cap, ctypes.byref(total))


def rows_call(name, Xd):
    if name == "plain":
        return L.mxa_ld_window_rows(P(Xd), snps, indiv, P(d_last), P(rows), 1, 1, P(f))
    return L.mxa_ld_window_rows_pairwise(P(Xd), snps, indiv, P(d_last), P(rows), 1)


for engine in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = engine
    for name, Xd in data.items():
        assert pairs_call(name, Xd, None, None, 0) == 0, mx.lib.last_error()          # the total of this data set (and the warm-up of the count pass)
        kept = total.value
        col, val = torch.empty(max(kept, 1), dtype=torch.int32, device=dev), torch.empty(max(kept, 1), dtype=torch.float64, device=dev)
        calls = {"rows": lambda: rows_call(name, Xd), "pairs, count only": lambda: pairs_call(name, Xd, None, None, 0), "pairs, filling": lambda: pairs_call(name, Xd, col, val, kept)}
        for fn in calls.values():
            kernel_ms(fn)                                                              # warm-up: code objects, allocator
        res = {n: [] for n in calls}
        for _ in range(reps):                                                          # alternating
            for n, fn in calls.items():
                res[n].append(kernel_ms(fn))
        med = {}
        for n in calls:
            k = sorted(res[n])
            med[n] = k[len(k) // 2]
            print(f"{engine} {name}: {n}: kernel {med[n]:.2f} ms median of {reps} (min {k[0]:.2f}, max {k[-1]:.2f}); {med[n] / ntiles * 1e3:.2f} us per tile", flush=True)
        print(f"{engine} {name}: {kept} pairs kept ({100.0 * kept / max(entries - snps, 1):.3f} % of the candidates, {12 * kept / 1e6:.1f} MB of col / val); "
              f"filling / rows {med['pairs, filling'] / med['rows']:.3f}, count only / rows {med['pairs, count only'] / med['rows']:.3f}", flush=True)
        del col, val
