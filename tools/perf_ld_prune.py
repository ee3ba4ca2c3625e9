#!/usr/bin/env python3
"""perf of the selection entries (mxa_ld_window_prune / mxa_ld_prune_csr: LD pruning and clumping on the device) in one process, on synthetic device data WITH LD
structure (independent SNPs have no pair above the cutoff): founders form a chain, each a copy of its predecessor with 30 % of the bytes redrawn, and every SNP is
a copy of the founder of its block of `block` SNPs with a per-SNP share of {0, 2, 10, 30} % of the bytes redrawn.  Plain route, both engines for the products.
HIP events throughout:
  products + select   the count-only and the filling call of mxa_ld_window_pairs (mxa_profile_get: the events inside the library), what the window entry runs
                      twice, the second time without val (the library's own timing of both passes of mxa_ld_window_prune is printed beside it);
  rounds, owner pass  events around mxa_ld_prune_csr on the device CSR, without and with owner (the owner pass = the difference), per priority: random, -MAF,
                      NULL; per round = the time without owner / rounds;
  the whole call      events around mxa_ld_window_prune.
For comparison the route that existed before these entries: ld_pairs() on the device, col / val / rowptr to the host, and the sequential walk in numpy / Python
(wall clock; the walk is the definition's, so the results are compared too).
usage: perf_ld_prune.py snps indiv window min_r2 [reps] [block]"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import miraculix_amd as mx
from miraculix_amd import crossproduct as cp

snps, indiv, window, min_r2 = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4])
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
block = int(sys.argv[6]) if len(sys.argv) > 6 else 12
dev = torch.device("cuda", 0)
L = mx.load_shared_library()
P = mx.lib.ptr


def random_bytes(n, row_bytes, g):
    """PLINK bytes without the missing code 01"""
    b = torch.randint(0, 256, (n, row_bytes), dtype=torch.uint8, device=dev, generator=g)
    return b ^ ((b & 0x55) & ~((b >> 1) & 0x55))


def synth_ld(snps, row_bytes, block, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nf = (snps + block - 1) // block
    F = random_bytes(nf, row_bytes, g)
    for k in range(1, nf):                                                             # the chain of founders
        F[k] = torch.where(torch.rand(row_bytes, device=dev, generator=g) < 0.3, F[k], F[k - 1])
    rate = torch.tensor([0.0, 0.02, 0.1, 0.3], device=dev)[torch.randint(0, 4, (snps,), device=dev, generator=g)]
    X = torch.empty((snps, row_bytes), dtype=torch.uint8, device=dev)
    chunk = max(block, ((128 << 20) // row_bytes) // block * block)
    for r0 in range(0, snps, chunk):
        r1 = min(snps, r0 + chunk)
        own = F[torch.arange(r0, r1, device=dev) // block]
        X[r0:r1] = torch.where(torch.rand((r1 - r0, row_bytes), device=dev, generator=g) < rate[r0:r1, None], random_bytes(r1 - r0, row_bytes, g), own)
    return X


def library_ms(fn):
    L.mxa_profile_reset()
    assert fn() == 0, mx.lib.last_error()
    torch.cuda.synchronize()
    la, ms = ctypes.c_int(0), ctypes.c_double(0)
    L.mxa_profile_get(ctypes.byref(la), ctypes.byref(ms))
    return ms.value


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert fn() == 0, mx.lib.last_error()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(fn, timer):
    timer(fn)                                                                          # warm-up: code objects, allocator
    k = sorted(timer(fn) for _ in range(reps))
    return k[len(k) // 2], k[0], k[-1]


def walk(n, rowptr, col, priority):
    """the sequential walk of the definition on the host (keep, owner)"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    a, b = np.concatenate([rows, col]), np.concatenate([col.astype(np.int64), rows])
    o = np.argsort(a, kind="stable")
    nb, start = b[o], np.concatenate([[0], np.cumsum(np.bincount(a, minlength=n))])
    order = np.arange(n) if priority is None else np.lexsort((np.arange(n), priority))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    keep, owner = np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int32)
    for v in order:
        m = nb[start[v]: start[v + 1]]
        kept = m[keep[m]]
        if kept.size == 0:
            keep[v], owner[v] = True, v
        else:
            owner[v] = kept[np.argmin(rank[kept])]
    return keep, owner


row_bytes = (indiv + 3) // 4
X = synth_ld(snps, row_bytes, block, 7)
f = torch.empty(snps, dtype=torch.float64, device=dev)
for r0 in range(0, snps, 4096):                                                        # the data's own frequency: 0, 1, 2 copies in the fields 00, 10, 11
    b = X[r0: r0 + 4096]
    fields = torch.stack([(b >> (2 * q)) & 3 for q in range(4)], dim=-1).reshape(b.shape[0], -1)[:, :indiv]
    f[r0: r0 + 4096] = torch.clamp(fields.to(torch.int16) - 1, min=0).sum(dim=1, dtype=torch.int64).to(torch.float64) / (2 * indiv)
last = np.minimum(np.arange(snps) + window, snps - 1).astype(np.int32)
d_last = torch.from_numpy(last).to(dev)
maf = torch.minimum(f, 1 - f)
g = torch.Generator(device=dev)
g.manual_seed(11)
priorities = {"random": torch.rand(snps, dtype=torch.float64, device=dev, generator=g), "-MAF": -maf, "NULL": None}
rowptr = torch.empty(snps + 1, dtype=torch.int64, device=dev)
keep, owner = torch.empty(snps, dtype=torch.uint8, device=dev), torch.empty(snps, dtype=torch.int32, device=dev)
total, n_kept, rounds = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_int(0)
print(f"LD prune {snps} SNPs x {indiv} indiv, window {window}, min_r2 {min_r2}, LD blocks of {block} on a founder chain, medians of {reps}", flush=True)


def pairs_call(col, val, cap):
    return L.mxa_ld_window_pairs(P(X), snps, indiv, P(d_last), min_r2, 1, P(rowptr), P(col), P(val), cap, ctypes.byref(total), 1, P(f))


def window_call(prio, with_owner):
    return L.mxa_ld_window_prune(P(X), snps, indiv, P(d_last), min_r2, P(prio), P(keep), P(owner) if with_owner else None, ctypes.byref(n_kept), ctypes.byref(rounds), 1, P(f))


def csr_call(col, prio, with_owner):
    return L.mxa_ld_prune_csr(snps, P(rowptr), P(col), P(prio), P(keep), P(owner) if with_owner else None, ctypes.byref(n_kept), ctypes.byref(rounds))


for engine in ("f4", "i8"):
    os.environ["MXA_XPROD_ENGINE"] = engine
    assert pairs_call(None, None, 0) == 0, mx.lib.last_error()
    pairs = total.value
    col, val = torch.empty(max(pairs, 1), dtype=torch.int32, device=dev), torch.empty(max(pairs, 1), dtype=torch.float64, device=dev)
    cnt, fill = median(lambda: pairs_call(None, None, 0), library_ms), median(lambda: pairs_call(col, val, pairs), library_ms)
    both = median(lambda: window_call(None, False), library_ms)
    print(f"{engine}: {pairs} pairs ({pairs / snps:.1f} per SNP); products + select, library events: count-only call {cnt[0]:.2f} ms (min {cnt[1]:.2f}, max {cnt[2]:.2f}), "
          f"filling call with val {fill[0]:.2f} ms (min {fill[1]:.2f}, max {fill[2]:.2f}), the two passes of mxa_ld_window_prune (col only) {both[0]:.2f} ms "
          f"(min {both[1]:.2f}, max {both[2]:.2f})", flush=True)
    if engine == "i8":
        break                                                                          # the graph step does not depend on the engine
    assert pairs_call(col, val, pairs) == 0
    for name, prio in priorities.items():
        no_owner, with_owner = median(lambda: csr_call(col, prio, False), event_ms), median(lambda: csr_call(col, prio, True), event_ms)
        r, k = rounds.value, n_kept.value
        whole = median(lambda: window_call(prio, True), event_ms)
        assert (rounds.value, n_kept.value) == (r, k)
        print(f"priority {name}: kept {k} of {snps}, rounds {r}; graph step without owner {no_owner[0]:.2f} ms (min {no_owner[1]:.2f}, max {no_owner[2]:.2f}) = "
              f"{1e3 * no_owner[0] / r:.1f} us per round; with owner {with_owner[0]:.2f} ms: owner pass {with_owner[0] - no_owner[0]:.2f} ms; "
              f"mxa_ld_window_prune with owner, whole call {whole[0]:.2f} ms (min {whole[1]:.2f}, max {whole[2]:.2f})", flush=True)
        if name == "NULL":
            continue                                                                   # the host route is timed under two priorities
        d_keep, d_owner = keep.cpu().numpy().astype(bool), owner.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_rowptr, h_col, h_val = cp.ld_pairs(X, snps, indiv, last=d_last, min_r2=min_r2, kind="r2", is_plink_format=True, allele_freq=f)
        h_rowptr, h_col, h_val = h_rowptr.cpu().numpy(), h_col.cpu().numpy(), h_val.cpu().numpy()
        t1 = time.perf_counter()
        h_keep, h_owner = walk(snps, h_rowptr, h_col, prio.cpu().numpy())
        t2 = time.perf_counter()
        same = bool(np.array_equal(h_keep, d_keep) and np.array_equal(h_owner, d_owner))
        print(f"priority {name}: the host route: ld_pairs + {12 * len(h_col) / 1e6:.1f} MB to the host {1e3 * (t1 - t0):.1f} ms, the walk in numpy / Python {1e3 * (t2 - t1):.1f} ms, "
              f"together {1e3 * (t2 - t0):.1f} ms = {1e3 * (t2 - t0) / whole[0]:.1f} x the device call; same keep and owner: {same}", flush=True)
        assert same
