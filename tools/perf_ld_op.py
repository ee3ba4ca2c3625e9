#!/usr/bin/env python3
"""perf of the LD operator object (mxa_ld_op_*) over last[i] = min(i + window, snps - 1), kind r2, device operands, one process, HIP events (torch) around
whole calls, alternating legs:
  creation   mxa_ld_op_create against mxa_ld_window_rows to a device buffer, both engines;
  apply      mxa_ld_op_apply at n in {1, 16, 64} against the whole call of mxa_ld_window_apply (term r2) at the same n, with the byte model beside it:
             8 (2 entries - snps) bytes of mirrored rows over the 7.0 TB/s read ceiling of DESIGN.md 7;
  solve      mxa_ld_op_solve held to 50 iterations (a tolerance no residual reaches) at n in {1, 16} against 50 times the mxa_ld_window_apply call.
usage: perf_ld_op.py snps indiv window [reps]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import miraculix_amd as mx
from bench import synth_plink_device

snps, indiv, window = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
NS = (1, 16, 64)
READ_CEILING = 7.0e12
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr


def timed(fn):
    pre = getattr(fn, "pre", None)
    if pre:
        pre()                                                             # outside the timed span
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


X = synth_plink_device(torch, snps, (indiv + 3) // 4, 7, dev)
f = torch.empty(snps, dtype=torch.float64, device=dev)                  # the data's own frequencies: r is a correlation, T + I positive definite
assert L.mxa_allele_freq(P(X), snps, indiv, P(f)) == 0, mx.lib.last_error()
last = np.minimum(np.arange(snps) + window, snps - 1).astype(np.int32)
entries, nbytes = mx.crossproduct.ld_op_bytes(last)
d_last = torch.from_numpy(last).to(dev)
model_ms = 8 * (2 * entries - snps) / READ_CEILING * 1e3
print(f"ld-op {snps} SNPs x {indiv} indiv, window {window}, kind r2: {entries} upper entries, object {nbytes / 1e9:.2f} GB ({8 * (2 * entries - snps) / 1e9:.2f} GB of "
      f"mirrored rows), upper rows during creation {8 * entries / 1e9:.2f} GB; byte model of one pass {model_ms:.2f} ms at {READ_CEILING / 1e12:.1f} TB/s", flush=True)
rows = torch.empty(entries, dtype=torch.float64, device=dev)
handle = ctypes.c_void_p(None)


def release():
    L.mxa_ld_op_free(ctypes.byref(handle))


def create():
    assert L.mxa_ld_op_create(P(X), snps, indiv, P(d_last), 1, 1, P(f), ctypes.byref(handle)) == 0, mx.lib.last_error()


create.pre = release                                                      # the previous object goes before the clock starts: creation alone is timed


def rows_call():
    assert L.mxa_ld_window_rows(P(X), snps, indiv, P(d_last), P(rows), 1, 1, P(f)) == 0, mx.lib.last_error()


for engine in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = engine
    m = alternate({"create": create, "rows": rows_call}, reps)
    for k, (a, lo, hi) in m.items():
        print(f"{engine} {k}: whole {a:.2f} ms median (min {lo:.2f}, max {hi:.2f})", flush=True)
    print(f"{engine}: create / rows to a device buffer: {m['create'][0] / m['rows'][0]:.3f}", flush=True)
os.environ.pop("MXA_XPROD_ENGINE")
del rows
torch.cuda.empty_cache()

nmax = max(NS)
B = torch.randn(nmax, snps, dtype=torch.float64, device=dev)              # column-major snps x nmax
Y = torch.empty(nmax, snps, dtype=torch.float64, device=dev)
Y2 = torch.empty(nmax, snps, dtype=torch.float64, device=dev)


def op_apply(n):
    assert L.mxa_ld_op_apply(handle, 0.0, P(B), snps, n, P(Y), snps) == 0, mx.lib.last_error()


def window_apply(n):
    assert L.mxa_ld_window_apply(P(X), snps, indiv, P(d_last), 1, P(B), snps, n, P(Y2), snps, 1, P(f)) == 0, mx.lib.last_error()


legs = {}
for n in NS:
    legs[f"op apply n={n}"] = (lambda n=n: op_apply(n))
    legs[f"window apply n={n}"] = (lambda n=n: window_apply(n))
m = alternate(legs, reps)
for k, (a, lo, hi) in m.items():
    print(f"{k}: whole {a:.3f} ms median of {reps} (min {lo:.3f}, max {hi:.3f})", flush=True)
for n in NS:
    a, w = m[f"op apply n={n}"][0], m[f"window apply n={n}"][0]
    passes = (n + 15) // 16
    print(f"n={n}: op apply / window apply = {a / w:.4f} ({w / a:.1f} times faster); {passes} pass(es) over the object: byte model {passes * model_ms:.2f} ms, "
          f"reached {passes * model_ms / a:.3f} of it ({passes * 8 * (2 * entries - snps) / a / 1e9:.2f} TB/s)", flush=True)
op_apply(nmax)
window_apply(nmax)
torch.cuda.synchronize()
print(f"agreement: max |op apply - window apply| / max |Y| = {float((Y - Y2).abs().max() / Y2.abs().max()):.2e}", flush=True)

ITER = 50
Xs = torch.empty(16, snps, dtype=torch.float64, device=dev)
Bs = B[:16] * 1e60                                                        # T + I is well conditioned: the residual falls by orders of magnitude per iteration, and
                                                                          # |b|^2 of 1e126 keeps r.r and p.Ap of the fiftieth iteration far above the smallest double
iters, status = np.zeros(16, np.int32), np.zeros(16, np.int32)


def solve(n):
    assert L.mxa_ld_op_solve(handle, 1.0, P(Bs), snps, n, P(Xs), snps, 1e-300, ITER, P(iters), None, P(status)) == 0, mx.lib.last_error()


sm = alternate({f"solve n={n}": (lambda n=n: solve(n)) for n in (1, 16)}, max(3, reps // 2))
for n in (1, 16):
    solve(n)
    a, lo, hi = sm[f"solve n={n}"]
    w = m[f"window apply n={n}"][0]
    ran = int(iters[:n].max())                                            # the loop runs until the last column stops: the iterations that were timed
    note = "" if ran == ITER and set(status[:n].tolist()) == {1} else f" -- NOT the {ITER} iterations asked for: the figures below are for {ran}"
    print(f"solve n={n}: {ran} iterations run (iters {iters[:n].min()} .. {iters[:n].max()}, status {sorted(set(status[:n].tolist()))}){note}; whole {a:.2f} ms median "
          f"(min {lo:.2f}, max {hi:.2f}), {a / max(ran, 1):.3f} ms per iteration; {ran} mxa_ld_window_apply calls at their median: {ran * w:.1f} ms; "
          f"ratio {a / (max(ran, 1) * w):.4f}", flush=True)
L.mxa_ld_op_free(ctypes.byref(handle))
