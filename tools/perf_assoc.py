#!/usr/bin/env python3
"""perf of the association scan (mxa_assoc_linear), device operands, one process, HIP events (torch) around whole calls, alternating legs:
  shapes   n = 1, k = 15 and n = 16, k = 16 (both 16 columns or 32: one and two passes of the scan);
  data     random PLINK bytes without the missing code, and the same with 5 % of the fields set to 01;
  beside   mxa_dgemm_compressed_device('T') with n + k columns on a RESIDENT object of the same matrix (uncentred): the bare product the scan is built on.
The whole call includes what a resident object has paid before: the allocations, the recode pass that packs the one-shot object, the phenotype preparation.
Kernel times come from a run of its own under rocprofv3 --kernel-trace (tools/profile.sh assoc-kernels): `perf_assoc.py snps indiv trace` makes two calls per
data set and shape and nothing else of the library; `perf_assoc.py summarize kernel_trace.csv` prints, for the second call of each, the time of every library
kernel by name in dispatch order of first appearance (a call ends with k_assoc_finish).
Model: the 'T' product of n + k columns + ceil((n + k) / 16) reads of the raw matrix at the 7.0 TB/s read ceiling + O(snps (n + k)) epilogue bytes.
The score test (mxa_assoc_score) is the same script with `score` in front (tools/profile.sh assoc-score, assoc-score-kernels): shapes n = 1, q = 15
and n = 4, q = 15 (kh = q + 1 projection columns per trait: 18 and 72 columns of B), beside mxa_assoc_linear at n = 1, k = 15 and the bare 'T' product of the same
column counts, in column chunks of at most 32 as the entry itself multiplies.  Its summary puts the weight kernel (k_assoc_weights: E = the weights summed over
the 11 fields) beside its model -- one read of the raw matrix at 7.0 TB/s plus snps x indiv masked adds per pass, one pass per trait -- and beside k_assoc_scan.
usage: perf_assoc.py [score] snps indiv [reps | trace]   |   perf_assoc.py summarize kernel_trace.csv   |   perf_assoc.py summarize-score kernel_trace.csv"""
import csv, ctypes, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import miraculix_amd as mx
from bench import synth_plink_device



SCORE_SHAPES = ((1, 15), (4, 15))


def summarize(path, last="k_assoc_finish", shapes=((1, 15), (16, 16)), second="k"):
    rows = [r for r in csv.DictReader(open(path)) if "mxa::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], []
    for r in rows:
        name = re.sub(r"^.*?mxa::(\(anonymous namespace\)::)?", "", r["Kernel_Name"]).split("(")[0].split("<")[0]
        cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
        if name == last:
            calls.append(cur)
            cur = []
    labels = [f"{d}, n={n} {second}={k}" for d in ("no missing", "5 % missing") for n, k in shapes]
    assert len(calls) == 2 * len(labels), (len(calls), "calls in the trace")
    for i, label in enumerate(labels):
        call, order, tot = calls[2 * i + 1], [], {}
        for name, ms in call:
            if name not in tot:
                order.append(name)
                tot[name] = [0, 0.0]
            tot[name][0] += 1
            tot[name][1] += ms
        print(f"{label}: library kernels {sum(ms for _, ms in call):.2f} ms in {len(call)} launches: " +
              ", ".join(f"{nm} {tot[nm][1]:.2f} ms" + (f" ({tot[nm][0]})" if tot[nm][0] > 1 else "") for nm in order), flush=True)


if sys.argv[1] == "summarize":
    summarize(sys.argv[2])
    sys.exit(0)
if sys.argv[1] == "summarize-score":
    summarize(sys.argv[2], "k_assoc_score_finish", SCORE_SHAPES, "q")
    sys.exit(0)
score = sys.argv[1] == "score"
if score:
    del sys.argv[1]
snps, indiv = int(sys.argv[1]), int(sys.argv[2])
trace = len(sys.argv) > 3 and sys.argv[3] == "trace"
reps = int(sys.argv[3]) if len(sys.argv) > 3 and not trace else 5
SHAPES = ((1, 15), (16, 16))
READ_CEILING, MFMA_PEAK = 7.0e12, 78.6e12
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr
dg = mx.dgemm_compressed
bps = (indiv + 3) // 4


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def med(v):
    k = sorted(v)
    return k[len(k) // 2], k[0], k[-1]


def alternate(legs, reps):
    for fn in legs.values():
        timed(fn)                                                         # warm-up: code objects, allocator
    res = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            res[k].append(timed(fn))
    return {k: med(v) for k, v in res.items()}


def with_missing(X, frac, seed):
    """a copy of X with `frac` of the fields set to 01, in chunks"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = X.clone()
    chunk = max(1, (256 << 20) // bps)
    for r0 in range(0, snps, chunk):
        b = out[r0:r0 + chunk]
        for q in range(4):
            m = torch.rand(b.shape, device=dev, generator=g) < frac
            b[m] = (b[m] & (0xFF ^ (3 << (2 * q)))) | (1 << (2 * q))
    return out


print(f"assoc {snps} SNPs x {indiv} indiv: raw matrix {snps * bps / 1e9:.2f} GB, one scan pass {snps * bps / READ_CEILING * 1e3:.2f} ms at {READ_CEILING / 1e12:.1f} TB/s", flush=True)
data = {"no missing": synth_plink_device(torch, snps, bps, 7, dev)}
data["5 % missing"] = with_missing(data["no missing"], 0.05, 8)
dg.set_options(use_gpu=True, not_center=True, verbose=0)
nmax = max(n + k for n, k in SHAPES)
rng = np.random.default_rng(3)
W = rng.standard_normal((indiv, max(k for _, k in SHAPES)))
Qh = mx.assoc_basis(W)
Yd = (100.0 + torch.randn(max(n for n, _ in SHAPES), indiv, dtype=torch.float64, device=dev))
Qd = torch.from_numpy(np.ascontiguousarray(Qh.T)).to(dev)
Bd = torch.randn(nmax, indiv, dtype=torch.float64, device=dev)
Cd = torch.empty(nmax, snps, dtype=torch.float64, device=dev)
out = [torch.empty(16, snps, dtype=torch.float64, device=dev) for _ in range(3)]
nobs = torch.empty(snps, dtype=torch.int32, device=dev)



def score_legs():
    """the score test: whole calls beside mxa_assoc_linear at n = 1, k = 15 and the bare 'T' products, alternating; or, for the trace, two calls per shape"""
    nt = max(n for n, _ in SCORE_SHAPES)
    kh = max(q for _, q in SCORE_SHAPES) + 1
    Rd = torch.randn(nt, indiv, dtype=torch.float64, device=dev)
    Wd = 0.25 * torch.rand(nt, indiv, dtype=torch.float64, device=dev)
    Hd = torch.randn(nt * kh, indiv, dtype=torch.float64, device=dev) / indiv ** 0.5
    Bs = torch.randn(32, indiv, dtype=torch.float64, device=dev)
    Cs = torch.empty(32, snps, dtype=torch.float64, device=dev)

    def scan(X, n, q):
        assert L.mxa_assoc_score(P(X), snps, indiv, P(Rd), indiv, P(Wd), indiv, P(Hd), indiv, n, q + 1, P(out[0]), P(out[1]), P(out[2]), snps, P(nobs)) == 0, mx.lib.last_error()

    for name, X in data.items():
        if trace:
            for n, q in SCORE_SHAPES:
                for _ in range(2):
                    scan(X, n, q)
            torch.cuda.synchronize()
            continue
        obj = ctypes.c_void_p(None)
        assert L.mxa_plink2compressed_begin(snps, indiv, 32, ctypes.byref(obj)) == 0, mx.lib.last_error()
        assert L.mxa_plink2compressed_rows(obj, P(X), 0, snps, None) == 0 and L.mxa_plink2compressed_end(obj) == 0, mx.lib.last_error()

        def linear():
            assert L.mxa_assoc_linear(P(X), snps, indiv, P(Yd), indiv, 1, P(Qd), indiv, 15, P(out[0]), P(out[1]), P(out[2]), snps, P(nobs), None) == 0, mx.lib.last_error()

        def product(cols):                                                  # in column chunks of at most 32, as the entries multiply
            for c0 in range(0, cols, 32):
                assert L.mxa_dgemm_compressed_device(b"T", obj, min(32, cols - c0), P(Bs), indiv, P(Cs), snps, None, 1) == 0, mx.lib.last_error()

        legs = {"assoc_linear n=1 k=15": linear, "'T' product 16 columns": (lambda: product(16))}
        for n, q in SCORE_SHAPES:
            legs[f"score n={n} q={q}"] = (lambda n=n, q=q: scan(X, n, q))
            legs[f"'T' product {n * (q + 3)} columns"] = (lambda c=n * (q + 3): product(c))
        m = alternate(legs, reps)
        lin, p16 = m["assoc_linear n=1 k=15"], m["'T' product 16 columns"]
        print(f"{name}: assoc_linear n=1 k=15 whole call {lin[0]:.2f} ms median of {reps} (min {lin[1]:.2f}, max {lin[2]:.2f}); bare 'T' product of 16 columns "
              f"{p16[0]:.2f} ms", flush=True)
        for n, q in SCORE_SHAPES:
            cols = n * (q + 3)
            a, lo, hi = m[f"score n={n} q={q}"]
            p, plo, phi = m[f"'T' product {cols} columns"]
            passes, epasses = (cols + 15) // 16, n
            adds = snps * indiv * epasses
            print(f"{name}, n={n} q={q} ({cols} columns): score whole call {a:.2f} ms median of {reps} (min {lo:.2f}, max {hi:.2f}); bare 'T' product of {cols} columns on a "
                  f"resident object {p:.2f} ms (min {plo:.2f}, max {phi:.2f}) = {2.0 * snps * indiv * cols / p / 1e9:.1f} TFLOP/s; ratio to the product {a / p:.2f}, to "
                  f"assoc_linear n=1 k=15 {a / lin[0]:.2f}; model of the kernels: product + {passes} scan pass(es) + {epasses} weight pass(es) of "
                  f"{snps * bps / READ_CEILING * 1e3:.2f} ms each + {adds:.3g} masked adds = {p + (passes + epasses) * snps * bps / READ_CEILING * 1e3:.2f} ms + the adds",
                  flush=True)
        freed = ctypes.c_void_p(obj.value)
        L.free_compressed(ctypes.byref(freed))


if score:
    score_legs()
    sys.exit(0)

for name, X in data.items():
    if trace:                                                             # two calls per shape, nothing else: what the kernel trace is cut into
        for n, k in SHAPES:
            for _ in range(2):
                assert L.mxa_assoc_linear(P(X), snps, indiv, P(Yd), indiv, n, P(Qd), indiv, k, P(out[0]), P(out[1]), P(out[2]), snps, P(nobs), None) == 0, mx.lib.last_error()
        torch.cuda.synchronize()
        continue
    obj = ctypes.c_void_p(None)
    assert L.mxa_plink2compressed_begin(snps, indiv, nmax, ctypes.byref(obj)) == 0, mx.lib.last_error()
    assert L.mxa_plink2compressed_rows(obj, P(X), 0, snps, None) == 0 and L.mxa_plink2compressed_end(obj) == 0, mx.lib.last_error()

    def assoc(n, k):
        assert L.mxa_assoc_linear(P(X), snps, indiv, P(Yd), indiv, n, P(Qd), indiv, k, P(out[0]), P(out[1]), P(out[2]), snps, P(nobs), None) == 0, mx.lib.last_error()

    def product(cols):
        assert L.mxa_dgemm_compressed_device(b"T", obj, cols, P(Bd), indiv, P(Cd), snps, None, 1) == 0, mx.lib.last_error()

    legs = {}
    for n, k in SHAPES:
        legs[f"assoc n={n} k={k}"] = (lambda n=n, k=k: assoc(n, k))
        legs[f"'T' product {n + k} columns"] = (lambda c=n + k: product(c))
    m = alternate(legs, reps)
    for n, k in SHAPES:
        a, lo, hi = m[f"assoc n={n} k={k}"]
        p, plo, phi = m[f"'T' product {n + k} columns"]
        passes = (n + k + 15) // 16
        flop = 2.0 * snps * indiv * (n + k)
        print(f"{name}, n={n} k={k}: assoc whole call {a:.2f} ms median of {reps} (min {lo:.2f}, max {hi:.2f}); bare 'T' product of {n + k} columns on a resident object "
              f"{p:.2f} ms (min {plo:.2f}, max {phi:.2f}) = {flop / p / 1e9:.1f} TFLOP/s, {flop / p / 1e9 / (MFMA_PEAK / 1e12):.3f} of the fp64 MFMA peak; ratio {a / p:.2f}; "
              f"model of the kernels: product + {passes} scan pass(es) = "
              f"{p + passes * snps * bps / READ_CEILING * 1e3:.2f} ms", flush=True)
    freed = ctypes.c_void_p(obj.value)
    L.free_compressed(ctypes.byref(freed))
