#!/usr/bin/env python3
"""perf of the set tests (mxa_assoc_set) beside mxa_assoc_score on the same operands, device operands, one process, HIP events (torch) around whole calls,
alternating legs, median of `reps`.
  data     genotypes drawn on the device with a minor allele frequency per SNP from {0.005, 0.01, 0.02, 0.05} (no missing calls); one Gaussian trait with q = 3
           covariates: R = residual / s^2, Wt = 1 / s^2, H = W C L^-T (kh = 4); sets of `size` neighbouring SNPs (32, then 8 and 256), unit weights
  legs     mxa_assoc_score; mxa_assoc_set (stat only, no scan results) for each set size; and the route a user has without the entry: gather the rows of a batch
           of sets, decode them to fp64 in torch and take torch.bmm of (X diag(w)) X^T -- timed over the first TORCH_SETS sets of 32 and scaled to all of them
Kernel times come from a run of its own under rocprofv3 --kernel-trace (tools/profile.sh assoc-set-kernels): `perf_assoc_set.py snps indiv trace` makes two
calls of mxa_assoc_set per set size and nothing else of the library; `perf_assoc_set.py summarize kernel_trace.csv` prints the time of every library kernel of
each second call by name (a call begins with k_assoc_pack).
usage: perf_assoc_set.py snps indiv [reps | trace]   |   perf_assoc_set.py summarize kernel_trace.csv"""
import csv, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (32, 8, 256)
TORCH_SETS, TORCH_BATCH = 64, 16


def summarize(path):
    rows = [r for r in csv.DictReader(open(path)) if "mxa::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        name = re.sub(r"^.*?mxa::(\(anonymous namespace\)::)?", "", r["Kernel_Name"]).split("(")[0].split("<")[0]
        if name == "k_assoc_pack":
            calls.append([])
        if calls:
            calls[-1].append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    assert len(calls) == 2 * len(SIZES), (len(calls), "calls in the trace")
    for e, size in enumerate(SIZES):
        call = calls[2 * e + 1]
        order, tot = [], {}
        for name, ms in call:
            if name not in tot:
                order.append(name)
                tot[name] = [0, 0.0]
            tot[name][0] += 1
            tot[name][1] += ms
        print(f"sets of {size}, second call: library kernels {sum(ms for _, ms in call):.2f} ms in {len(call)} launches: " +
              ", ".join(f"{nm} {tot[nm][1]:.2f} ms" + (f" ({tot[nm][0]})" if tot[nm][0] > 1 else "") for nm in order), flush=True)


if sys.argv[1] == "summarize":
    summarize(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch
import miraculix_amd as mx

snps, indiv = int(sys.argv[1]), int(sys.argv[2])
trace = len(sys.argv) > 3 and sys.argv[3] == "trace"
reps = int(sys.argv[3]) if len(sys.argv) > 3 and not trace else 7
assert indiv % 4 == 0, "indiv needs to be a multiple of 4 here (the rows are packed on the device without padding fields)"
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr
bps = indiv // 4
Q_COV = 3


def genotypes():
    """snps x bps packed rows on the device, row s at the minor allele frequency MAFS[s % 4], Hardy-Weinberg, no missing calls"""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    X = torch.empty((snps, bps), dtype=torch.uint8, device=dev)
    mafs = torch.tensor([0.005, 0.01, 0.02, 0.05], device=dev)
    chunk = max(4, ((64 << 20) // indiv) // 4 * 4)
    for r0 in range(0, snps, chunk):
        rows = min(chunk, snps - r0)
        f = mafs[(torch.arange(r0, r0 + rows, device=dev) % 4)][:, None]
        u = torch.rand((rows, indiv), device=dev, generator=g)
        p0 = (1 - f) ** 2
        code = (u >= p0).to(torch.uint8) + (u >= p0 + 2 * f * (1 - f)).to(torch.uint8)          # the allele count
        field = torch.where(code == 0, code, code + 1).reshape(rows, bps, 4)                     # 00, 10, 11
        X[r0:r0 + rows] = field[:, :, 0] | (field[:, :, 1] << 2) | (field[:, :, 2] << 4) | (field[:, :, 3] << 6)
    return X


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


X = genotypes()
rng = np.random.default_rng(3)
C = np.column_stack([np.ones(indiv), rng.standard_normal((indiv, Q_COV))])
y = 0.5 * C[:, 1] + rng.standard_normal(indiv)
res = y - C @ np.linalg.lstsq(C, y, rcond=None)[0]
s2 = res @ res / (indiv - Q_COV - 1)
w = np.full(indiv, 1 / s2)
H = (w[:, None] * C) @ np.linalg.inv(np.linalg.cholesky(C.T @ (w[:, None] * C))).T
kh = Q_COV + 1
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
Rd, Wd, Hd = to_dev(res / s2), to_dev(w), to_dev(H.T)
out = [torch.empty(snps, dtype=torch.float64, device=dev) for _ in range(3)]
nobs = torch.empty(snps, dtype=torch.int32, device=dev)


def score():
    assert L.mxa_assoc_score(P(X), snps, indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, 1, kh, P(out[0]), P(out[1]), P(out[2]), snps, P(nobs)) == 0, mx.lib.last_error()


def set_leg(size):
    nsets = snps // size
    ptr = np.arange(nsets + 1, dtype=np.int64) * size
    idx = np.arange(nsets * size, dtype=np.int32)
    stat = torch.empty((6, nsets), dtype=torch.float64, device=dev)

    def run():
        assert L.mxa_assoc_set(P(X), snps, indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, 1, kh, nsets, P(ptr), P(idx), None, None, None, None, snps, None, P(stat),
                               nsets, None) == 0, mx.lib.last_error()
    run.nsets = nsets
    return run


def torch_gram(size, first, count):
    """S of the sets [first, first + count) of `size` neighbouring SNPs: gather, decode to fp64 (0, 1, 2; no missing calls here), bmm"""
    rows = X[first * size:(first + count) * size]                                   # neighbouring SNPs: the gather is a slice
    f = torch.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(count, size, indiv)
    x = torch.where(f == 0, f, f - 1).to(torch.float64)
    return torch.bmm(x * Wd[None, None, :], x.transpose(1, 2))


legs = {f"set size {s}": set_leg(s) for s in SIZES}
if trace:
    for run in legs.values():
        run()
        run()
    torch.cuda.synchronize()
    sys.exit(0)

print(f"{snps} SNPs x {indiv} individuals, n = 1, kh = {kh}, device operands, median of {reps}, ms", flush=True)
for fn in [score] + list(legs.values()):
    fn()                                                                           # first calls: not timed
times = {"score": []}
times.update({k: [] for k in legs})
for _ in range(reps):
    times["score"].append(timed(score))
    for k, fn in legs.items():
        times[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in times.items()}
print(f"mxa_assoc_score: {med['score']:.1f} (min {min(times['score']):.1f}, max {max(times['score']):.1f})", flush=True)
for k, fn in legs.items():
    stage = med[k] - med["score"]
    size = int(k.split()[-1])
    flop = fn.nsets * (size // 16) * (size // 16 + 1) / 2 * 2 * 256 * indiv if size >= 16 else fn.nsets * 2 * 256 * indiv
    print(f"mxa_assoc_set, {fn.nsets} sets of {size}: {med[k]:.1f} (min {min(times[k]):.1f}, max {max(times[k]):.1f}) = {med[k] / med['score']:.2f} x mxa_assoc_score; "
          f"the stage {stage:.1f} = {stage / fn.nsets * 1e3:.1f} us per set; {flop / 1e12:.2f} TFLOP of 16 x 16 tiles = {flop / stage / 1e9:.1f} TFLOP/s over the whole stage",
          flush=True)
# the torch route at sets of 32
torch_gram(32, 0, TORCH_BATCH)
tt = []
for _ in range(reps):
    tt.append(timed(lambda: [torch_gram(32, b, TORCH_BATCH) for b in range(0, TORCH_SETS, TORCH_BATCH)]))
per_set = statistics.median(tt) / TORCH_SETS
n32 = legs["set size 32"].nsets
stage32 = med["set size 32"] - med["score"]
print(f"torch route (decode to fp64 + bmm), sets of 32, {TORCH_SETS} sets in batches of {TORCH_BATCH}: {per_set * 1e3:.1f} us per set = {per_set * n32:.1f} ms scaled to {n32} sets; "
      f"the whole set stage takes {stage32 / (per_set * n32):.3f} of that ({per_set * n32 / stage32:.1f} x faster)", flush=True)
S = torch_gram(32, 0, 1)[0]
print(f"torch S[0, :2, :2] of set 0: {S[:2, :2].flatten().tolist()}", flush=True)
