#!/usr/bin/env python3
"""kernel-level perf of the windowed LD entries mxa_ld_band / mxa_ld_scores on synthetic device data (device results).  Prints per entry the kernel time
(HIP events around the tile launch and its tail / finish kernel: mxa_profile_get), the tiles launched, the bytes written and the time divided by the
tile-rate model of crossprod_any (tiles x K stages x tile_stage_ms / 256 CUs: 0.66 us per stage FP4, 1.0 us int8) so that the cost of the epilogues shows.
--vs-full: also mxa_ld into a snps x snps device result, alternating band / full calls (A/B in one process).
usage: perf_ld_band.py snps indiv window [reps] [--vs-full]      (MXA_XPROD_ENGINE=i8 for the int8 engine)"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import miraculix_amd as mx
from miraculix_amd.crossproduct import ld_band_tiles
from bench import synth_plink_device

args = [a for a in sys.argv[1:] if not a.startswith("--")]
snps, indiv, window = int(args[0]), int(args[1]), int(args[2])
reps = int(args[3]) if len(args) > 3 else 3
vs_full = "--vs-full" in sys.argv
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr
engine = "int8" if os.environ.get("MXA_XPROD_ENGINE") == "i8" else "FP4"
stage_ms = 1.0e-3 if engine == "int8" else 0.66e-3
nslabs = (indiv + 127) // 128


def kernel_ms(fn):
    """one call: (kernel ms by the library's events, wall ms)"""
    L.mxa_profile_reset()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    assert fn() == 0, mx.lib.last_error()
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    la, ms = ctypes.c_int(0), ctypes.c_double(0)
    L.mxa_profile_get(ctypes.byref(la), ctypes.byref(ms))
    return ms.value, wall * 1e3


X = synth_plink_device(torch, snps, (indiv + 3) // 4, 7, dev)           # SNP-major: snps rows x indiv / 4 bytes
f = torch.rand(snps, dtype=torch.float64, device=dev) * 0.4 + 0.1
band = torch.empty((snps, window + 1), dtype=torch.float64, device=dev)
scores = torch.empty(snps, dtype=torch.float64, device=dev)
ntiles = len(ld_band_tiles(snps, window)) if snps <= 2_000_000 else -1
model = ntiles * nslabs * stage_ms / 256.0
in_band = (window + 1) * snps - window * (window + 1) // 2               # elements R(i, i + d) with i + d < snps
ndiag = (window + 255) // 256
calls = {
    "mxa_ld_band r": (lambda: L.mxa_ld_band(P(X), snps, indiv, window, P(band), window + 1, 0, 1, P(f)), 8 * (window + 1) * snps),
    "mxa_ld_band r2": (lambda: L.mxa_ld_band(P(X), snps, indiv, window, P(band), window + 1, 1, 1, P(f)), 8 * (window + 1) * snps),
    "mxa_ld_scores": (lambda: L.mxa_ld_scores(P(X), snps, indiv, window, P(scores), 0, 1, P(f)), 8 * (2 * ntiles - (snps + 255) // 256) * 256 + 8 * snps),
}
print(f"windowed LD {snps} SNPs x {indiv} indiv, window {window}, {engine} engine: {ntiles} tiles x {nslabs} K stages, tile-rate model {model:.2f} ms; "
      f"{in_band} band elements ({8 * in_band / 1e9:.2f} GB)", flush=True)
for name, (fn, nbytes) in calls.items():
    kernel_ms(fn)                                                        # warm-up: code objects, allocator
    res = [kernel_ms(fn) for _ in range(reps)]
    k = sorted(r[0] for r in res)
    print(f"{name}: kernel {k[len(k) // 2]:.2f} ms median of {reps} (min {k[0]:.2f}, max {k[-1]:.2f}) = {k[len(k) // 2] / model:.2f} x model; {ntiles} tiles launched, "
          f"{nbytes / 1e9:.3f} GB written; call wall {min(r[1] for r in res):.1f} ms", flush=True)
if vs_full:
    R = torch.empty((snps, snps), dtype=torch.float64, device=dev)
    full = lambda: L.mxa_ld(P(X), snps, indiv, P(R), 1, P(f))
    kernel_ms(full)
    a, b = [], []
    for _ in range(reps):                                                # A/B, alternating
        a.append(kernel_ms(calls["mxa_ld_band r"][0]))
        b.append(kernel_ms(full))
    nb = (snps + 255) // 256
    for name, r, nt in (("mxa_ld_band r", a, ntiles), (f"mxa_ld (full {8 * snps * snps / 1e9:.1f} GB result)", b, nb * (nb + 1) // 2)):
        k, w = sorted(x[0] for x in r), sorted(x[1] for x in r)
        print(f"A/B {name}: kernel {k[len(k) // 2]:.2f} ms median of {reps} (min {k[0]:.2f}, max {k[-1]:.2f}), call wall {w[len(w) // 2]:.1f} ms median, {nt} tiles", flush=True)
    # the band of the full result equals the band (spot check, first and last SNPs)
    for i in (0, 1000, snps - 1):
        hi = min(snps, i + window + 1)
        assert torch.equal(band[i, : hi - i], R[i, i:hi]), i
    print("band == band of the full result at the sampled SNPs (bit for bit)")
