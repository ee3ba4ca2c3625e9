#!/usr/bin/env python3
"""perf of the mixed-model scan (miraculix_amd.mixed.assoc_mixed): device operands, one process, one whole call after a small warm-up call.
  data     genotypes drawn on the device with allele frequencies U(0.05, 0.5) per SNP (Hardy-Weinberg, no missing calls, unrelated individuals); one Gaussian
           trait with q = 3 covariates and a polygenic part from 200 SNPs (every 50th of the first 10 000); `blocks` chromosome blocks of equal size, LOCO, h2 by Haseman-Elston
  split    HIP events (torch, default stream) around every Kinship.apply -- the mxa_gram_matvec_device calls of all blocks plus their sum -- and around every
           assoc_score call; "everything else" is the whole call minus the two: torch vector operations, decodes, the small products with the covariates,
           staging of the kinship objects and host waits
  trace    `perf_assoc_mixed.py snps indiv blocks trace` makes the warm-up call and ONE call, for a run of its own under rocprofv3 --kernel-trace
           (tools/profile.sh assoc-mixed); `perf_assoc_mixed.py summarize kernel_trace.csv` prints the kernel time by class -- library kernels of the scan
           (k_assoc*), the other library kernels (the products of the kinship operator and its staging), everything that is not the library's (torch, rocBLAS)
           -- and the time of the span in which no kernel ran
The split decides whether a device-side solver (the vector updates fused, no host read per iteration) is worth building: it is when "everything else" is a
large share of the call.
usage: perf_assoc_mixed.py snps indiv [blocks [trace]]   |   perf_assoc_mixed.py summarize kernel_trace.csv"""
import csv, os, re, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(path):
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))]
    rows.sort()
    cls = {"scan (k_assoc*)": [0, 0.0], "library, other (kinship products, staging)": [0, 0.0], "not the library's (torch, rocBLAS)": [0, 0.0]}
    busy_end, idle, first = None, 0.0, None
    for s, e, name in rows:
        short = re.sub(r"^.*?mxa::(\(anonymous namespace\)::)?", "", name).split("(")[0].split("<")[0] if "mxa::" in name else None
        key = "not the library's (torch, rocBLAS)" if short is None else "scan (k_assoc*)" if short.startswith("k_assoc") else "library, other (kinship products, staging)"
        cls[key][0] += 1
        cls[key][1] += (e - s) / 1e6
        if first is None:
            first = s
        if busy_end is not None and s > busy_end:
            idle += (s - busy_end) / 1e6
        busy_end = e if busy_end is None else max(busy_end, e)
    span = (busy_end - first) / 1e6
    print(f"kernel trace of the warm-up call and one call: span {span:.1f} ms, no kernel running for {idle:.1f} ms of it ({100 * idle / span:.1f} %)")
    for key, (count, ms) in cls.items():
        print(f"  {key}: {ms:.1f} ms in {count} launches")


if len(sys.argv) > 2 and sys.argv[1] == "summarize":
    summarize(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch
import miraculix_amd as mx
from miraculix_amd import mixed

snps, indiv = int(sys.argv[1]), int(sys.argv[2])
blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 5
trace = len(sys.argv) > 4 and sys.argv[4] == "trace"
assert indiv % 4 == 0 and snps % (4 * blocks) == 0, "indiv needs to be a multiple of 4 and snps one of 4 blocks here"
dev = torch.device("cuda", 0)
mx.load_shared_library()
mx.dgemm_compressed.set_options(use_gpu=True, not_center=False, verbose=0)
bps = indiv // 4
Q_COV = 3


def genotypes():
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    X = torch.empty((snps, bps), dtype=torch.uint8, device=dev)
    chunk = max(4, ((64 << 20) // indiv) // 4 * 4)
    for r0 in range(0, snps, chunk):
        rows = min(chunk, snps - r0)
        f = 0.05 + 0.45 * torch.rand((rows, 1), device=dev, generator=g)
        u = torch.rand((rows, indiv), device=dev, generator=g)
        p0 = (1 - f) ** 2
        code = (u >= p0).to(torch.uint8) + (u >= p0 + 2 * f * (1 - f)).to(torch.uint8)
        field = torch.where(code == 0, code, code + 1).reshape(rows, bps, 4)
        X[r0:r0 + rows] = field[:, :, 0] | (field[:, :, 1] << 2) | (field[:, :, 2] << 4) | (field[:, :, 3] << 6)
    return X


X = genotypes()
g = torch.Generator(device=dev)
g.manual_seed(9)
W = torch.randn((indiv, Q_COV), dtype=torch.float64, device=dev, generator=g)
causal, _ = mixed.decode_imputed(X[::50][:200].contiguous(), indiv)
causal = causal - causal.mean(0, keepdim=True)
poly = causal @ torch.randn((causal.shape[1], 1), dtype=torch.float64, device=dev, generator=g)
Y = 0.6 * poly / poly.std() + 0.8 * torch.randn((indiv, 1), dtype=torch.float64, device=dev, generator=g) + W @ torch.tensor([[0.3], [-0.2], [0.1]], dtype=torch.float64, device=dev)
del causal, poly
Wh = W.cpu().numpy()
bounds = [b * (snps // blocks) for b in range(blocks)] + [snps]

pairs = {"gram": [], "scan": []}


def bracket(kind, fn):
    def run(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **k)
        e1.record()
        pairs[kind].append((e0, e1))
        return out
    return run


mixed.Kinship.apply = bracket("gram", mixed.Kinship.apply)
mixed._assoc.assoc_score = bracket("scan", mixed._assoc.assoc_score)

# warm-up on the first rows: workspace growth, first launches, torch's lazily loaded kernels
ws = min(snps, 4 * 2048)
mixed.assoc_mixed(X[:ws], ws, indiv, Y, Wh, chrom_bounds=[0, ws // 2, ws], h2=0.3, calib_snps=8, tol=1e-6)
torch.cuda.synchronize()
print("data drawn, warm-up call done", flush=True)
for v in pairs.values():
    v.clear()
t0 = time.perf_counter()
res = mixed.assoc_mixed(X, snps, indiv, Y, Wh, chrom_bounds=bounds)
torch.cuda.synchronize()
wall = (time.perf_counter() - t0) * 1e3
if trace:
    sys.exit(0)
ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in pairs.items()}
other = wall - ms["gram"] - ms["scan"]
z = res.zstat[:, 0]
lam = float(torch.median(z[torch.isfinite(z)] ** 2)) / 0.4549
print(f"{snps} SNPs x {indiv} individuals, n = 1, q = {Q_COV}, {blocks} blocks, LOCO, calib_snps 200, no exact stage, device operands, one call, ms", flush=True)
print(f"assoc_mixed whole call: {wall:.1f}; h2 {res.h2[0]:.4f}, calibration factors {np.array2string(res.gamma[:, 0], precision=4)}, lambda_GC {lam:.3f}")
print(f"  Kinship.apply (mxa_gram_matvec_device per block + the sum): {ms['gram']:.1f} in {len(pairs['gram'])} calls = {100 * ms['gram'] / wall:.1f} %")
print(f"  assoc_score (the scan): {ms['scan']:.1f} in {len(pairs['scan'])} calls = {100 * ms['scan'] / wall:.1f} %")
print(f"  everything else (torch vector operations, decodes, staging of the kinship objects, host waits): {other:.1f} = {100 * other / wall:.1f} %")
