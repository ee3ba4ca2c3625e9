#!/usr/bin/env python3
"""perf of the score test with saddlepoint p-values (mxa_assoc_score_spa) beside mxa_assoc_score, device operands, one process, HIP events (torch) around
whole calls, alternating legs.
  data     genotypes drawn on the device with a minor allele frequency per SNP from {0.005, 0.01, 0.05, 0.2} (no missing calls); one 0 / 1 trait with
           5 % cases from a logistic model in q = 3 covariates; the null fitted by mxa_assoc_logistic_null (host), P = y - r
  legs     mxa_assoc_score; mxa_assoc_score_spa at z_cutoff = 1.96 (about 5 % of the SNPs under the null) and at z_cutoff = inf (the stage without any item:
           the classification, the list and the one host wait)
Kernel times come from a run of its own under rocprofv3 --kernel-trace (tools/profile.sh assoc-spa-kernels): `perf_assoc_spa.py snps indiv trace` makes two
calls of the entry and nothing else of the library; `perf_assoc_spa.py summarize kernel_trace.csv` prints the time of every library kernel of the second
call by name (a call begins with k_assoc_pack).
Model: items x 2 sides x evaluations x indiv terms of about 100 fp64 operations, and as many reads of 16 bytes (g and p).
usage: perf_assoc_spa.py snps indiv [reps | trace]   |   perf_assoc_spa.py summarize kernel_trace.csv"""
import csv, math, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    assert len(calls) == 2, (len(calls), "calls in the trace")
    order, tot = [], {}
    for name, ms in calls[1]:
        if name not in tot:
            order.append(name)
            tot[name] = [0, 0.0]
        tot[name][0] += 1
        tot[name][1] += ms
    print(f"second call: library kernels {sum(ms for _, ms in calls[1]):.2f} ms in {len(calls[1])} launches: " +
          ", ".join(f"{nm} {tot[nm][1]:.2f} ms" + (f" ({tot[nm][0]})" if tot[nm][0] > 1 else "") for nm in order), flush=True)


if sys.argv[1] == "summarize":
    summarize(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch
import miraculix_amd as mx

snps, indiv = int(sys.argv[1]), int(sys.argv[2])
trace = len(sys.argv) > 3 and sys.argv[3] == "trace"
reps = int(sys.argv[3]) if len(sys.argv) > 3 and not trace else 5
assert indiv % 4 == 0, "indiv needs to be a multiple of 4 here (the rows are packed on the device without padding fields)"
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr
bps = indiv // 4
Q_COV, Z_CUTOFF = 3, 1.96


def genotypes():
    """snps x bps packed rows on the device, row s at the minor allele frequency MAFS[s % 4], Hardy-Weinberg, no missing calls"""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    X = torch.empty((snps, bps), dtype=torch.uint8, device=dev)
    mafs = torch.tensor([0.005, 0.01, 0.05, 0.2], device=dev)
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
W = rng.standard_normal((indiv, Q_COV))
eta = math.log(0.05 / 0.95) + 0.3 * (W @ rng.standard_normal(Q_COV))
y = (rng.random(indiv) < 1 / (1 + np.exp(-eta))).astype(np.float64)
fit = mx.assoc_logistic_null(y, W)
kh = Q_COV + 1
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
Pd, Rd, Wd, Hd = to_dev(y - fit.r), to_dev(fit.r), to_dev(fit.w), to_dev(fit.H.T)
out = [torch.empty(snps, dtype=torch.float64, device=dev) for _ in range(4)]
flag = torch.empty(snps, dtype=torch.int32, device=dev)
nobs = torch.empty(snps, dtype=torch.int32, device=dev)


def score():
    assert L.mxa_assoc_score(P(X), snps, indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, 1, kh, P(out[0]), P(out[1]), P(out[2]), snps, P(nobs)) == 0, mx.lib.last_error()


def spa(z_cutoff):
    assert L.mxa_assoc_score_spa(P(X), snps, indiv, P(Pd), indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, 1, kh, z_cutoff, 2.0 ** -30, 50, P(out[0]), P(out[1]), P(out[2]),
                                 P(out[3]), snps, P(flag), P(nobs)) == 0, mx.lib.last_error()


if trace:
    for _ in range(2):
        spa(Z_CUTOFF)
    torch.cuda.synchronize()
    sys.exit(0)

legs = {"score": score, "score_spa z_cutoff=1.96": (lambda: spa(Z_CUTOFF)), "score_spa z_cutoff=inf": (lambda: spa(math.inf))}
for fn in legs.values():
    timed(fn)                                                                 # warm-up: code objects, allocator
res = {k: [] for k in legs}
for _ in range(reps):
    for k, fn in legs.items():
        res[k].append(timed(fn))
spa(Z_CUTOFF)
counts = torch.bincount(flag, minlength=4).tolist()
items = counts[1] + counts[2]
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}          # (a call now and then pays hundreds of ms for its allocations: the median, with min and max beside it)
print(f"assoc_spa {snps} SNPs x {indiv} indiv, n = 1, q = {Q_COV}, {int(y.sum())} cases ({100 * y.mean():.1f} %): raw matrix {snps * bps / 1e9:.2f} GB; flags 0/1/2/3 = {counts}, "
      f"{items} items ({100.0 * items / snps:.1f} % of the SNPs)", flush=True)
for k, v in res.items():
    print(f"{k}: whole call {med[k]:.2f} ms median of {reps} (min {min(v):.2f}, max {max(v):.2f})", flush=True)
extra = med["score_spa z_cutoff=1.96"] - med["score"]
print(f"the correction: {extra:.2f} ms beyond mxa_assoc_score ({med['score_spa z_cutoff=1.96'] / med['score']:.2f} x the scan), {extra / max(items, 1) * 1e3:.1f} us per item; "
      f"the empty stage {med['score_spa z_cutoff=inf'] - med['score']:.2f} ms; model at 8 evaluations a side: {items * 2 * 8 * indiv:.3g} terms, "
      f"{items * 2 * 8 * indiv * 16 / 1e9:.1f} GB of g and p", flush=True)
