#!/usr/bin/env python3
"""Emit tests/golden/ld_entries_digests.json: sha256 digests of what the general-window LD entries return on small seeded inputs, as THIS library computes
them on an MI355X -- mxa_ld_window_rows / _scores / _pairs / _apply / _prune (plain and _pairwise), mxa_ld_prune_csr and the operator object (mxa_ld_op_create
(_pairwise), _rows, _apply, _solve).  make_golden_ld_window.py pins the four fixed-window entries; this file pins the entries that go through the int32 count
scratch and the ones built on them, which the other tests hold only to bounds and to identities between entries.  tests/test_ld_entries_golden_gpu.py
recomputes every case and compares, so a change of one bit of a value, a position in a CSR, a kept SNP or an iteration count is reported.

One case = (shape, route, missing fraction, window, engine, variant); per case five digests, one per family of results: `rs` (rows kind 0 / 1, scores adjust
0 / 1), `pairs`, `apply`, `prune`, `op`.  A digest runs over the labelled bytes of every result of its family in the order computed, sentinel-filled padding
included (ldx / ldy = snps + 3, two entries behind every flat result).  Windows: last[i] = min(i + w, snps - 1) for w in WINDOWS, and `dist`: from
mxa_ld_window_bounds over seeded positions on two chromosomes (the generator asserts that the chromosome end is no multiple of 256, that an inner SNP has
last[i] = i, and -- where snps allows it -- that a row reaches beyond 256 SNPs, i.e. a second tile diagonal).  Variants: device pointers on VARIANTS,
MXA_LD_PAIRWISE_SCRATCH_MB=1 on GROUPS (one tile row per group), MXA_LD_PAIRWISE_DENSE=1 on the missing-free pairwise cases of VARIANTS; both engines throughout.
`recorded_at` names the tree that was run (see make_golden_ld_window.py); the digests of the inputs are stored and asserted first.  Fixtures are data only.

usage: make_golden_ld_entries.py [COMMIT]          write the golden file (needs the GPU)
       make_golden_ld_entries.py --emit OUT.json   the child process: its digests as JSON"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden_ld_window import make_inputs, sha, tree_id  # noqa: E402

GOLDEN = os.path.join(HERE, "ld_entries_digests.json")
SENTINEL = -12345.678
ISENTINEL = -77

SHAPES = ((200, 131), (777, 203), (1024, 160))   # below one tile; four ragged tile rows; exactly four tiles
VARIANTS = (777, 203)                            # device pointers, the dense switch
GROUPS = (1024, 160)                             # the scratch cap of 1 MiB: one tile row per group, four groups
WINDOWS = (0, 100, 300)
ENGINES = (None, "i8")
ROUTES = (("plain", 0.0), ("pw", 0.0), ("pw", 0.05))
MIN_R2 = (0.0, 0.02)
FAMILIES = ("rs", "pairs", "apply", "prune", "op")


def distance_window(L, P, snps):
    """(pos, chrom, last) of a window by distance on two chromosomes: a dense cluster whose rows reach across it, an isolated SNP, Poisson gaps elsewhere"""
    rng = np.random.default_rng([snps, 7])
    cend = (3 * snps) // 5                                    # first SNP of the second chromosome
    cend += cend % 256 == 0
    gaps = rng.exponential(1.0, snps)
    dense = slice(10, min(410, cend - 20))
    gaps[dense] *= 0.05
    iso = cend + 5
    gaps[iso] = gaps[iso + 1] = 1000.0
    pos = np.cumsum(gaps)
    chrom = np.where(np.arange(snps) < cend, 1, 2).astype(np.int32)
    last = np.full(snps, ISENTINEL, np.int32)
    rc = L.mxa_ld_window_bounds(snps, P(pos), P(chrom), 40.0, -1, P(last), None)
    assert rc == 0
    reach = last - np.arange(snps)
    assert cend % 256 != 0 and last[cend - 1] == cend - 1 and (last[:cend] < cend).all()
    assert last[iso] == iso
    assert snps < 512 or reach.max() > 256
    return pos, chrom, last


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, label, a):
        self.h.update(label.encode() + b"\0")
        self.h.update(np.ascontiguousarray(a).tobytes())

    def hex(self):
        return self.h.hexdigest()


def emit():
    """every case: (digests of the inputs, digests of the results)"""
    sys.path.insert(0, ROOT)
    import torch
    import miraculix_amd as mx
    L = mx.load_shared_library()
    P = mx.lib.ptr
    dev = torch.device("cuda", 0)
    inputs, results = {}, {}

    def setenv(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value

    def case(key, d, snps, indiv, last, pairwise, device, solve):
        up = (lambda a: torch.from_numpy(a).to(dev)) if device else (lambda a: a)
        down = (lambda a: a.cpu().numpy()) if device else (lambda a: a)
        X, f, lastp = up(d["plink"]), up(d["f"]), up(last)
        sfx = "_pairwise" if pairwise else ""
        tail = () if pairwise else (1, P(f))
        head = (P(X), snps, indiv, P(lastp))
        entries = int((last - np.arange(snps) + 1).sum())
        rng = np.random.default_rng([snps, indiv, 11])

        def ok(rc, what):
            assert rc == 0, (key, what, mx.lib.last_error())

        def full(n, value, dtype):
            return up(np.full(n, value, dtype))

        def put(D, family):
            assert f"{key}|{family}" not in results
            results[f"{key}|{family}"] = D.hex()

        # rows and scores
        D = Digest()
        for kind in (0, 1):
            out = full(entries + 2, SENTINEL, np.float64)
            ok(getattr(L, "mxa_ld_window_rows" + sfx)(*head, P(out), kind, *tail), "rows")
            D.add(f"rows {kind}", down(out))
        for adjust in (0, 1):
            out = full(snps, SENTINEL, np.float64)
            ok(getattr(L, "mxa_ld_window_scores" + sfx)(*head, P(out), adjust, *tail), "scores")
            D.add(f"scores {adjust}", down(out))
        put(D, "rs")

        # pairs: count only, filled, and filled with half the capacity (error 25)
        D = Digest()
        pairs = getattr(L, "mxa_ld_window_pairs" + sfx)
        csr = None
        for kind in (0, 1):
            for min_r2 in MIN_R2:
                total = ctypes.c_long(ISENTINEL)
                rowptr = full(snps + 1, ISENTINEL, np.int64)
                ok(pairs(*head, min_r2, kind, P(rowptr), None, None, 0, ctypes.byref(total), *tail), "pairs count")
                D.add(f"count {kind} {min_r2}", down(rowptr))
                D.add("total", np.int64(total.value))
                want = total.value
                for cap in (want, want // 2):
                    total = ctypes.c_long(ISENTINEL)
                    rowptr = full(snps + 1, ISENTINEL, np.int64)
                    col, val = full(cap + 2, ISENTINEL, np.int32), full(cap + 2, SENTINEL, np.float64)
                    rc = pairs(*head, min_r2, kind, P(rowptr), P(col), P(val), cap, ctypes.byref(total), *tail)
                    assert total.value == want
                    if want > cap:
                        assert rc == 1 and mx.lib.last_error()[0] == 25, (key, rc, mx.lib.last_error())
                        D.add(f"short {kind} {min_r2}", down(rowptr))
                        D.add("col", down(col)[:cap])
                        D.add("val", down(val)[:cap])
                    else:
                        ok(rc, "pairs fill")
                        D.add(f"fill {kind} {min_r2}", down(rowptr))
                        D.add("col", down(col))
                        D.add("val", down(val))
                        if kind == 0 and min_r2 == MIN_R2[1] and cap == want:
                            csr = (down(rowptr).copy(), down(col)[:want].copy())
                    D.add("total", np.int64(total.value))
        put(D, "pairs")

        # apply
        D = Digest()
        ld = snps + 3
        for term in (0, 1, 2):
            for n in (1, 17):
                Xm = up(rng.standard_normal((n, ld)))
                Y = full(n * ld, SENTINEL, np.float64)
                ok(getattr(L, "mxa_ld_window_apply" + sfx)(*head, term, P(Xm), ld, n, P(Y), ld, *tail), "apply")
                D.add(f"apply {term} {n}", down(Y))
        put(D, "apply")

        # prune: the window entry and the graph step on the pairs of min_r2 = MIN_R2[1], three priorities
        D = Digest()
        maf = np.minimum(d["f"], 1.0 - d["f"])
        for name, prio in (("none", None), ("seeded", rng.random(snps)), ("maf", -np.round(maf, 2))):
            pr = None if prio is None else up(prio)
            for which in ("window", "csr"):
                keep, owner = full(snps + 2, 99, np.uint8), full(snps + 2, ISENTINEL, np.int32)
                n_kept, rounds = ctypes.c_long(ISENTINEL), ctypes.c_int(ISENTINEL)
                if which == "window":
                    rc = getattr(L, "mxa_ld_window_prune" + sfx)(*head, MIN_R2[1], P(pr), P(keep), P(owner), ctypes.byref(n_kept), ctypes.byref(rounds), *tail)
                else:
                    rp, cl = up(csr[0]), up(csr[1])
                    rc = L.mxa_ld_prune_csr(snps, P(rp), P(cl), P(pr), P(keep), P(owner), ctypes.byref(n_kept), ctypes.byref(rounds))
                ok(rc, "prune " + which)
                D.add(f"{which} {name} keep", down(keep))
                D.add("owner", down(owner))
                D.add("n_kept rounds", np.array([n_kept.value, rounds.value], np.int64))
        put(D, "prune")

        # the operator object
        D = Digest()
        for kind in (0, 1):
            op = ctypes.c_void_p()
            if pairwise:
                ok(L.mxa_ld_op_create_pairwise(*head, kind, ctypes.byref(op)), "op create")
            else:
                ok(L.mxa_ld_op_create(*head, kind, 1, P(f), ctypes.byref(op)), "op create")
            out = full(entries + 2, SENTINEL, np.float64)
            ok(L.mxa_ld_op_rows(op, P(out)), "op rows")
            D.add(f"op rows {kind}", down(out))
            for shift in (0.0, 0.5):
                Xm = up(rng.standard_normal((3, ld)))
                Y = full(3 * ld, SENTINEL, np.float64)
                ok(L.mxa_ld_op_apply(op, shift, P(Xm), ld, 3, P(Y), ld), "op apply")
                D.add(f"op apply {shift}", down(Y))
            if kind == 1 and solve:
                B = up(rng.standard_normal((2, ld)))
                Xs = full(2 * ld, SENTINEL, np.float64)
                iters, relres, status = np.full(2, ISENTINEL, np.int32), np.full(2, SENTINEL), np.full(2, ISENTINEL, np.int32)
                ok(L.mxa_ld_op_solve(op, 2.0, P(B), ld, 2, P(Xs), ld, 1e-10, 500, P(iters), P(relres), P(status)), "op solve")
                D.add("op solve X", down(Xs))
                D.add("iters", iters)
                D.add("relres", relres)
                D.add("status", status)
            L.mxa_ld_op_free(ctypes.byref(op))
        put(D, "op")
        if device:
            torch.cuda.synchronize()

    for snps, indiv in SHAPES:
        pos, chrom, dist_last = distance_window(L, P, snps)
        inputs[f"{snps} pos"], inputs[f"{snps} chrom"], inputs[f"{snps} dist last"] = sha(pos), sha(chrom), sha(dist_last)
        lasts = [(f"w={w}", np.minimum(np.arange(snps) + w, snps - 1).astype(np.int32)) for w in WINDOWS] + [("dist", dist_last)]
        for route, miss in ROUTES:
            d = make_inputs(snps, indiv, miss)
            inputs[f"{snps}x{indiv} miss={miss} plink"] = sha(d["plink"])
            if miss == 0.0:
                inputs[f"{snps}x{indiv} f"] = sha(d["f"])
            pairwise = route == "pw"
            for wname, last in lasts:
                for engine in ENGINES:
                    setenv("MXA_XPROD_ENGINE", engine)
                    base = f"{snps}x{indiv} {route} m={miss} {wname} {engine or 'f4'}"
                    solve = wname == "w=100"
                    case(base + " host", d, snps, indiv, last, pairwise, False, solve)
                    if (snps, indiv) == VARIANTS:
                        case(base + " dev", d, snps, indiv, last, pairwise, True, solve)
                        if pairwise and miss == 0.0:
                            setenv("MXA_LD_PAIRWISE_DENSE", "1")
                            case(base + " dense", d, snps, indiv, last, pairwise, False, solve)
                            setenv("MXA_LD_PAIRWISE_DENSE", None)
                    if (snps, indiv) == GROUPS:
                        setenv("MXA_LD_PAIRWISE_SCRATCH_MB", "1")
                        case(base + " scratch1", d, snps, indiv, last, pairwise, False, solve)
                        setenv("MXA_LD_PAIRWISE_SCRATCH_MB", None)
    setenv("MXA_XPROD_ENGINE", None)
    return dict(inputs=inputs, results=results)


def collect(tmpdir):
    """the cases in one fresh child process, the environment switches cleared; returns its dict"""
    env = dict(os.environ)
    for k in ("MXA_XPROD_ENGINE", "MXA_XPROD_GANG", "MXA_LD_PAIRWISE_DENSE", "MXA_LD_PAIRWISE_SCRATCH_MB"):
        env.pop(k, None)
    path = os.path.join(tmpdir, "ld_entries.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--emit", path], check=True, env=env, timeout=900)
    with open(path) as fh:
        return json.load(fh)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--emit":
        with open(sys.argv[2], "w") as fh:
            json.dump(emit(), fh)
    else:
        import tempfile
        stamp = sys.argv[1] if len(sys.argv) > 1 else tree_id()
        if not stamp:
            sys.exit("this tree is no git checkout: name the commit it was exported from (make_golden_ld_entries.py COMMIT)")
        with tempfile.TemporaryDirectory() as tmp:
            out = collect(tmp)
        out["recorded_at"] = stamp
        with open(GOLDEN, "w") as fh:
            json.dump(out, fh, indent=0, sort_keys=True)
            fh.write("\n")
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(out["results"]), "results")
