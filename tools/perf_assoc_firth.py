#!/usr/bin/env python3
"""perf of the score test with effect sizes (mxa_assoc_score_firth, penalty 0 and 1) beside mxa_assoc_score and mxa_assoc_score_spa, device operands, one process,
HIP events (torch) around whole calls, alternating legs.
  data     genotypes drawn on the device with a minor allele frequency per SNP from {0.005, 0.01, 0.05, 0.2} (no missing calls); one 0 / 1 trait with
           5.5 % cases from a logistic model in q = 3 covariates; the null fitted by mxa_assoc_logistic_null (host), P = y - r
  legs     mxa_assoc_score; mxa_assoc_score_spa; mxa_assoc_score_firth with penalty 0 and with penalty 1; all at z_cutoff = 1.96: the same items
Kernel times come from a run of its own under rocprofv3 --kernel-trace (tools/profile.sh assoc-firth-kernels): `perf_assoc_firth.py snps indiv trace` makes two
calls of each of the three entries with a stage and nothing else of the library, then counts the evaluations of every item -- the header's Newton loops in
float64 on torch, outside the trace's library kernels: the library does not return them -- and prints them as a `counts:` line;
`perf_assoc_firth.py summarize kernel_trace.csv run.log` prints the time of every library kernel of each entry's second call by name (a call begins with
k_assoc_pack), and for k_assoc_spa and k_assoc_firth the time per item and per (item, evaluation).  An evaluation is one pass over g and p that sums K', K'', ...
or, at the accepted point, K and K''; the first pass of a workgroup (c0, A, G+, G-) is not counted.  k_assoc_spa runs two workgroups an item (the two sides),
k_assoc_firth one.
usage: perf_assoc_firth.py snps indiv [reps | trace]   |   perf_assoc_firth.py summarize kernel_trace.csv run.log"""
import csv, json, math, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENTRIES = ("score_spa", "score_firth penalty=0", "score_firth penalty=1")


def summarize(path, log):
    counts = json.loads(re.search(r"^counts: (.*)$", open(log).read(), flags=re.M).group(1))
    rows = [r for r in csv.DictReader(open(path)) if "mxa::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        name = re.sub(r"^.*?mxa::(\(anonymous namespace\)::)?", "", r["Kernel_Name"]).split("(")[0].split("<")[0]
        if name == "k_assoc_pack":
            calls.append([])
        if calls:
            calls[-1].append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    assert len(calls) == 2 * len(ENTRIES) + 1, (len(calls), "calls in the trace")          # (the last one: the mxa_assoc_score of the count)
    items = counts["items"]
    print(f"{items} items of {counts['indiv']} individuals", flush=True)
    per_eval = {}
    for e, entry in enumerate(ENTRIES):
        call = calls[2 * e + 1]
        order, tot = [], {}
        for name, ms in call:
            if name not in tot:
                order.append(name)
                tot[name] = [0, 0.0]
            tot[name][0] += 1
            tot[name][1] += ms
        print(f"{entry}, second call: library kernels {sum(ms for _, ms in call):.2f} ms in {len(call)} launches: " +
              ", ".join(f"{nm} {tot[nm][1]:.2f} ms" + (f" ({tot[nm][0]})" if tot[nm][0] > 1 else "") for nm in order), flush=True)
        solve = "k_assoc_spa" if e == 0 else "k_assoc_firth"
        ms, evals = tot[solve][1], counts["evaluations"][entry]
        per_eval[entry] = ms / evals * 1e6
        print(f"  {solve}: {ms:.2f} ms = {ms / items * 1e3:.1f} us per item; {evals} evaluations ({evals / items:.2f} an item) = {per_eval[entry]:.1f} ns per (item, evaluation) "
              f"= {per_eval[entry] / counts['indiv'] * 1e3:.2f} ps per term", flush=True)
    for entry in ENTRIES[1:]:
        print(f"{entry}: {per_eval[entry] / per_eval[ENTRIES[0]]:.2f} x k_assoc_spa's time per (item, evaluation)", flush=True)


if sys.argv[1] == "summarize":
    summarize(sys.argv[2], sys.argv[3])
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
Q_COV, Z_CUTOFF, TOL, MAX_ITER = 3, 1.96, 2.0 ** -30, 50


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
eta = math.log(0.05 / 0.95) + 0.3 * (W @ rng.standard_normal(Q_COV))          # (the data of tools/perf_assoc_spa.py: 5.5 % cases)
y = (rng.random(indiv) < 1 / (1 + np.exp(-eta))).astype(np.float64)
fit = mx.assoc_logistic_null(y, W)
kh = Q_COV + 1
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
Pd, Rd, Wd, Hd = to_dev(y - fit.r), to_dev(fit.r), to_dev(fit.w), to_dev(fit.H.T)
out = [torch.empty(snps, dtype=torch.float64, device=dev) for _ in range(7)]
flag = torch.empty(snps, dtype=torch.int32, device=dev)
nobs = torch.empty(snps, dtype=torch.int32, device=dev)


def score():
    assert L.mxa_assoc_score(P(X), snps, indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, 1, kh, P(out[0]), P(out[1]), P(out[2]), snps, P(nobs)) == 0, mx.lib.last_error()


def spa():
    assert L.mxa_assoc_score_spa(P(X), snps, indiv, P(Pd), indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, 1, kh, Z_CUTOFF, TOL, MAX_ITER, P(out[0]), P(out[1]), P(out[2]),
                                 P(out[3]), snps, P(flag), P(nobs)) == 0, mx.lib.last_error()


def firth(penalty):
    assert L.mxa_assoc_score_firth(P(X), snps, indiv, P(Pd), indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, 1, kh, Z_CUTOFF, penalty, TOL, MAX_ITER, P(out[0]), P(out[1]),
                                   P(out[2]), P(out[3]), P(out[4]), P(out[5]), P(out[6]), snps, P(flag), P(nobs)) == 0, mx.lib.last_error()


def newton_evaluations(G, p, c0, q, penalty, live):
    """the evaluations (the one at the accepted point included) of the header's Newton loop on every row of G that is live, rows at once: f = K' - q, with the
    penalty the further terms; penalty None: the saddlepoint entry's loop"""
    rows = G.shape[0]
    b, lo, hi = (torch.zeros(rows, dtype=torch.float64, device=dev), torch.full((rows,), -math.inf, dtype=torch.float64, device=dev),
                 torch.full((rows,), math.inf, dtype=torch.float64, device=dev))
    evals = torch.zeros(rows, dtype=torch.int64, device=dev)
    live = live.clone()
    for it in range(1, MAX_ITER + 1):
        if not bool(live.any()):
            break
        x = b[:, None] * G
        e = torch.exp(-x.abs())
        pos = x >= 0
        al, be = torch.where(pos, p, 1 - p), torch.where(pos, 1 - p, p)
        d = al + be * e
        pi = torch.where(pos, p / d, p * e / d)
        om = al * be * e / (d * d)
        K1, K2 = (G * pi).sum(1) - c0, (G * G * om).sum(1)
        f, fp = K1 - q, K2
        if penalty:
            r3 = (G ** 3 * om * (1 - 2 * pi)).sum(1) / K2
            f = f - 0.5 * r3
            alt = K2 - 0.5 * ((G ** 4 * om * (1 - 6 * om)).sum(1) / K2 - r3 * r3)
            fp = torch.where(alt > 0, alt, K2)
        evals += live
        lo, hi = torch.where(live & (f < 0), b, lo), torch.where(live & ~(f < 0), b, hi)
        bn = b - f / fp
        done = live & torch.isfinite(bn) & ((bn - b).abs() <= TOL * bn.abs())
        evals += done                                            # the evaluation of K and K'' at the accepted point
        inside = (bn > lo) & (bn < hi)
        bn = torch.where(inside, bn, 0.5 * (lo + hi))
        live = live & ~done & torch.isfinite(bn) & (it < MAX_ITER)
        b = torch.where(live, bn, b)
    return evals


def count_evaluations():
    """items and the evaluations of the three entries over them, from the scan's own U and z (no missing calls: x = the allele count, a_j = sum_i x_i h_ji)"""
    score()
    U, z = out[0].clone(), out[2].clone()
    marked = torch.nonzero(torch.isfinite(z) & (z.abs() >= Z_CUTOFF)).flatten()
    tau = Hd / Wd[None, :]
    total = {k: 0 for k in ENTRIES}
    step = max(1, (1 << 25) // indiv)
    for i0 in range(0, len(marked), step):
        rows = marked[i0:i0 + step]
        byte = X[rows].to(torch.int64)
        code = torch.stack([(byte >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(len(rows), indiv)
        G = torch.where(code == 0, code, code - 1).to(torch.float64)
        a = G @ Hd.T
        for j in range(kh):
            G = G - a[:, j:j + 1] * tau[j][None, :]
        c0, A, u = (G * Pd).sum(1), G.abs().sum(1), U[rows]
        gp, gm = G.clamp(min=0).sum(1), G.clamp(max=0).sum(1)
        for sigma in (1.0, -1.0):
            q = sigma * u.abs()
            inside = sigma * ((gp if sigma > 0 else gm) - c0 - q) > 2.0 ** -30 * A
            total[ENTRIES[0]] += int(newton_evaluations(G, Pd, c0, q, None, inside).sum())
        observed = torch.where(u >= 0, gp - c0 - u, -(gm - c0 - u)) > 2.0 ** -30 * A
        total[ENTRIES[1]] += int(newton_evaluations(G, Pd, c0, u, 0, observed).sum())
        total[ENTRIES[2]] += int(newton_evaluations(G, Pd, c0, u, 1, torch.ones_like(observed)).sum())
    return int(len(marked)), total


if trace:
    for fn in (spa, lambda: firth(0), lambda: firth(1)):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    items, total = count_evaluations()
    print("counts: " + json.dumps({"items": items, "indiv": indiv, "evaluations": total}), flush=True)
    sys.exit(0)

legs = {"score": score, "score_spa": spa, "score_firth penalty=0": (lambda: firth(0)), "score_firth penalty=1": (lambda: firth(1))}
for fn in legs.values():
    timed(fn)                                                                 # warm-up: code objects, allocator
res = {k: [] for k in legs}
for _ in range(reps):
    for k, fn in legs.items():
        res[k].append(timed(fn))
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}          # (a call now and then pays hundreds of ms for its allocations: the median, with min and max beside it)
print(f"assoc_firth {snps} SNPs x {indiv} indiv, n = 1, q = {Q_COV}, {int(y.sum())} cases ({100 * y.mean():.1f} %), z_cutoff = {Z_CUTOFF}: raw matrix "
      f"{snps * bps / 1e9:.2f} GB", flush=True)
for k, fn in legs.items():
    if k == "score":
        print(f"{k}: whole call {med[k]:.2f} ms median of {reps} (min {min(res[k]):.2f}, max {max(res[k]):.2f})", flush=True)
        continue
    fn()
    counts = torch.bincount(flag, minlength=4).tolist()
    items, extra = counts[1] + counts[2], med[k] - med["score"]
    print(f"{k}: whole call {med[k]:.2f} ms median of {reps} (min {min(res[k]):.2f}, max {max(res[k]):.2f}); flags 0/1/2/3 = {counts}, {items} items "
          f"({100.0 * items / snps:.1f} % of the SNPs); {extra:.2f} ms beyond mxa_assoc_score ({med[k] / med['score']:.2f} x the scan), "
          f"{extra / max(items, 1) * 1e3:.1f} us per item", flush=True)
