#!/usr/bin/env python3
"""Emit tests/golden/dgemm_digests.json: sha256 digests of what the fp64 product entries return on seeded inputs, as THIS library computes them on an
MI355X -- dgemm_compressed (host and device operands), mxa_dgemm_compressed_device, mxa_gram_matvec(_device) -- on every route of the host driver
(mxa_product.cpp: gemm_device, gemm_host_pipelined, gemm_any, gram_any): the guarded int8 route (n <= 6), the column peel (n = 4q + r), the plain fp64 tile, the
pair tables (K < 128), both stored-orientation policies, MXA_GEMM_TR=0, MXA_I8_TN=1, engines 1 / 3 / 4, host operands, the range fallback of the
denormal-operand mode (one pass and grouped), grouped K splits (MXA_P_BUDGET_MB), the host pipeline (K ranges for 'N', row ranges for 'T') and one sharded
object.  tests/test_dgemm_golden_digests_gpu.py recomputes every case and compares, so a change of one bit of C or of the route a product takes is reported.

One case = (group, shape, object, variant, n, 'N' / 'T', centred); one digest per case over the bytes of C -- the whole n x ldc buffer, i.e. the rows [m, ldc)
that the entries zero-fill, plus two sentinel entries behind it -- followed by mxa_last_path and the six mxa_last_geometry fields; the same seven integers are
stored next to the digest (`route`), and the generator asserts from them that the case took the route it is meant to pin.  (The sharded object's digest is over C
alone: its shards write the geometry from their worker threads.)  B carries 1e300 in its leading-dimension padding.  Operands: ldb = k + 3, ldc = m + 5.
`recorded_at` names the tree that was run (see make_golden_ld_window.py); the digests of the inputs are stored and asserted first.  Fixtures are data only.

usage: make_golden_dgemm.py [COMMIT]          write the golden file (needs the GPU)
       make_golden_dgemm.py --emit OUT.json   the child process: its digests as JSON"""
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

GOLDEN = os.path.join(HERE, "dgemm_digests.json")
SENTINEL = -12345.678
POISON = 1e300

SMALL = ((200, 131), (777, 203), (1024, 640), (300, 100))   # (300, 100): 'T' has K = 100 < 128, the fp64 / pair-table route
BOTH = ((777, 203), (1024, 640))                            # shapes that also get the two-copy object
VARIANTS = (777, 203)
SMALL_N = (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 8, 32)           # guarded | peel r = 3, 1, 2, 3 | plain tile
GROUPED = ((40_000, 3_000, 32), (30_011, 2_051, 20))        # the shapes of test_grouped_splits_bit_identical
PIPE = (140_003, 3_001)                                     # the shape of test_host_pipeline_gpu.py
PIPE_N = (32, 34)
KNOBS = ("MXA_SINGLE_ORIENTATION", "MXA_GEMM_TR", "MXA_I8_TN", "MXA_P_BUDGET_MB", "MXA_ENGINE", "MXA_WARMUP", "MXA_FORCE_MULTI", "MIRACULIX_NUM_GPUS", "MXA_DIAG",
         "PRINT_LEVEL")
GROUPS = ("small", "variant", "fallback", "grouped", "pipeline", "multi")


def make_big(snps, indiv):
    """dict(plink, f) of a large seeded matrix without missing codes, drawn bytewise (00 / 10 / 11 with probabilities 1/2, 1/4, 1/4)"""
    rng = np.random.default_rng([snps, indiv, 99])
    bps = (indiv + 3) // 4
    b = rng.integers(0, 256, (snps, bps), dtype=np.uint8)
    b ^= b & 0x55 & ~(b >> 1)                                 # a missing 01 becomes 00
    if indiv % 4:
        b[:, -1] &= (1 << (2 * (indiv % 4))) - 1              # clean padding bits
    alleles = np.array([sum((0, 0, 1, 2)[(v >> s) & 3] for s in (0, 2, 4, 6)) for v in range(256)], np.uint8)
    f = alleles[b].sum(axis=1, dtype=np.int64) / (2.0 * indiv)
    return dict(plink=np.ascontiguousarray(b), f=f)


def make_B(k, n, ldb, seed, kind=None):
    """n columns of k entries (row-major n x ldb = column-major ldb x n), magnitudes over six decades, 1e300 in the padding; kind: `span` = the last column spans
    more than 800 binades, `inf` = it holds an inf"""
    rng = np.random.default_rng(seed)
    B = np.full((n, ldb), POISON)
    B[:, :k] = rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    if kind == "span":
        B[n - 1, 0:k:3] *= 1e-150
        B[n - 1, 1:k:3] *= 1e+120
        nz = np.abs(B[n - 1, :k])
        assert np.log2(nz.max() / nz[nz > 0].min()) > 800
    elif kind == "inf":
        B[n - 1, 5] = np.inf
    return B


def expected_paths(single, trans, n, k, engine, fallback):
    """(allowed mxa_last_path values, columns the recorded geometry describes) by the rules of gemm_device.  Paths: 0 k_gemm, 1 pair tables, 2 int8, 3 the fp64
    kernels behind the int8 route's guard.  The opt-in int8 engines may decline 'N' of a one-copy object (transposed-operand form) to the fp64 tile."""
    small_ok = (engine == 0 or (engine == 4 and n <= 2)) and k >= 128
    no_plain = single and not trans
    if small_ok and n <= 6:
        return ({3} if fallback else {2}), n
    if engine == 4 and k >= 128 and n > 2 and not fallback:
        return {2} | ({0} if no_plain else set()), n
    if engine == 1:
        return {2} | ({0} if no_plain else set()), n
    n_geo = n
    if small_ok and n > 6 and n & 3:
        n_geo = n - (n & 3)
    return ({1} if n_geo <= 2 and not no_plain else {0}), n_geo


def emit():
    """every case: (digests of the inputs, digest and route of every result)"""
    sys.path.insert(0, ROOT)
    import torch
    import miraculix_amd as mx
    L = mx.load_shared_library()
    P = mx.lib.ptr
    dg = mx.dgemm_compressed
    dev = torch.device("cuda", 0)
    inputs, results, wrong = {}, {}, []

    def setenv(**kv):
        for name, value in kv.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = str(value)

    def create(d, snps, indiv, max_n, single, **env):
        setenv(MXA_SINGLE_ORIENTATION=1 if single else 0, **env)
        obj = ctypes.c_void_p()
        L.plink2compressed(P(d["plink"]), None, snps, indiv, P(d["f"]), max_n, ctypes.byref(obj))
        setenv(MXA_SINGLE_ORIENTATION=None, **{k: None for k in env})
        assert obj.value and L.mxa_last_error() == 0, mx.lib.last_error()
        if "MIRACULIX_NUM_GPUS" not in env:
            assert L.mxa_single_orientation(obj) == (1 if single else 0)
        return obj

    def route():
        m, k, splits = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
        n, a, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.mxa_last_geometry(ctypes.byref(m), ctypes.byref(k), ctypes.byref(n), ctypes.byref(splits), ctypes.byref(a), ctypes.byref(c))
        return [L.mxa_last_path(), m.value, k.value, n.value, splits.value, a.value, c.value]

    def put(key, C, r):
        h = hashlib.sha256()
        h.update(np.ascontiguousarray(C).tobytes())
        if r is not None:
            h.update(np.array(r, np.int64).tobytes())
        assert key not in results, key
        results[key] = dict(sha=h.hexdigest(), route=r)

    def product(key, obj, snps, indiv, single, n, trans, centered, device, kind=None, engine=0, expect=True, seed=0):
        """one dgemm_compressed; returns the route"""
        k, m = (indiv, snps) if trans else (snps, indiv)
        ldb, ldc = k + 3, m + 5
        B = make_B(k, n, ldb, [snps, indiv, n, trans, seed], kind)
        C = np.full(n * ldc + 2, SENTINEL)
        dg.set_options(use_gpu=True, not_center=not centered, verbose=0)
        t = b"T" if trans else b"N"
        if device:
            Bd, Cd = torch.from_numpy(B).to(dev), torch.from_numpy(C).to(dev)
            rc = L.mxa_dgemm_compressed_device(t, obj, n, P(Bd), ldb, P(Cd), ldc, None, 1)
            assert rc == 0
            r = route()
            C = Cd.cpu().numpy()
        else:
            L.dgemm_compressed(t, obj, n, P(B), ldb, P(C), ldc)
            r = route()
        assert L.mxa_last_error() == 0, (key, mx.lib.last_error())
        assert (C[n * ldc:] == SENTINEL).all() and (C[:n * ldc].reshape(n, ldc)[:, m:] == 0.0).all(), key
        if expect is None:
            put(key, C, None)
            return r
        paths, n_geo = expected_paths(single, trans, n, k, engine, kind is not None)
        if r[0] not in paths or r[1:3] != [m, k] or r[3] != n_geo:
            wrong.append((key, r, sorted(paths), n_geo))
        put(key, C, r)
        return r

    def sweep(group, label, obj, snps, indiv, single, ns, device, **kw):
        out = []
        for n in ns:
            for trans in (0, 1):
                for centered in (0, 1):
                    key = f"{group}|{snps}x{indiv} {label} n={n} {'T' if trans else 'N'} c={centered}"
                    out.append(product(key, obj, snps, indiv, single, n, trans, centered, device, **kw))
        return out

    def free(obj):
        L.free_compressed(ctypes.byref(obj))

    # ---- small shapes: device operands, every column count; the variants at one shape
    for snps, indiv in SMALL:
        d = make_inputs(snps, indiv, 0.02)
        inputs[f"{snps}x{indiv} plink"], inputs[f"{snps}x{indiv} f"] = sha(d["plink"]), sha(d["f"])
        for single in ((True, False) if (snps, indiv) in BOTH else (True,)):
            oname = "one-copy" if single else "two-copy"
            obj = create(d, snps, indiv, 32, single)
            sweep("small", oname + " dev", obj, snps, indiv, single, SMALL_N, True)
            if (snps, indiv) in BOTH and not single:
                setenv(MXA_GEMM_TR=0)
                sweep("variant", oname + " tr=0 dev", obj, snps, indiv, single, (8, 10), True)
                setenv(MXA_GEMM_TR=None, MXA_I8_TN=1)
                sweep("variant", oname + " i8tn=1 dev", obj, snps, indiv, single, (1, 2), True)
                setenv(MXA_I8_TN=None)
            if (snps, indiv) == VARIANTS:
                for engine in (1, 3, 4):
                    assert L.mxa_set_engine(engine) == 0
                    sweep("variant", f"{oname} engine={engine} dev", obj, snps, indiv, single, (2, 5, 10), True, engine=engine)
                    assert L.mxa_set_engine(0) == engine
                sweep("variant", oname + " host", obj, snps, indiv, single, (5, 10, 32), False)
                for n in (1, 10):                                  # gram: out = Zc (Zc^T V), the intermediate stays on the device
                    for centered in (0, 1):
                        for device in (False, True):
                            ldv, ldo = indiv + 3, indiv + 5
                            V = make_B(indiv, n, ldv, [snps, indiv, n, 7])
                            out = np.full(n * ldo + 2, SENTINEL)
                            dg.set_options(use_gpu=True, not_center=not centered, verbose=0)
                            if device:
                                Vd, Od = torch.from_numpy(V).to(dev), torch.from_numpy(out).to(dev)
                                rc = L.mxa_gram_matvec_device(obj, n, P(Vd), ldv, P(Od), ldo, 1)
                                out = Od.cpu().numpy()
                            else:
                                rc = L.mxa_gram_matvec(obj, n, P(V), ldv, P(out), ldo)
                            key = f"variant|{snps}x{indiv} {oname} gram {'dev' if device else 'host'} n={n} c={centered}"
                            assert rc == 0 and (out[n * ldo:] == SENTINEL).all(), (key, mx.lib.last_error())
                            put(key, out, route())
                for kind in ("span", "inf"):                       # range fallback, one pass and under the 1 MB budget
                    for mb in (None, 1):
                        setenv(MXA_P_BUDGET_MB=mb)
                        rs = sweep("fallback", f"{oname} {kind} mb={mb} dev", obj, snps, indiv, single, (3, 8), True, kind=kind)
                        assert L.mxa_last_range_fallback(obj) == 1     # (the last product: n = 8, the flag of the denormal-operand mode)
                        setenv(MXA_P_BUDGET_MB=None)
            free(obj)

    # ---- grouped K splits: budgets of 1 MB and of about 2.5 splits, and the range fallback through the groups
    for snps, indiv, n in GROUPED:
        d = make_big(snps, indiv)
        inputs[f"{snps}x{indiv} plink"], inputs[f"{snps}x{indiv} f"] = sha(d["plink"]), sha(d["f"])
        for single in (True, False):
            oname = "one-copy" if single else "two-copy"
            obj = create(d, snps, indiv, n, single)
            most = 0
            for trans in (0, 1):
                m = snps if trans else indiv
                one_split_mb = 8.0 * n * (m + 512) / 2 ** 20
                for centered in (0, 1):
                    for mb in (None,) + tuple(sorted({1, int(2.5 * one_split_mb) + 1})):      # (the short side's 2.5 splits can be the 1 MB again)
                        setenv(MXA_P_BUDGET_MB=mb)
                        key = f"grouped|{snps}x{indiv} {oname} mb={mb} dev n={n} {'T' if trans else 'N'} c={centered}"
                        r = product(key, obj, snps, indiv, single, n, trans, centered, True)
                        most = max(most, r[4])
                setenv(MXA_P_BUDGET_MB=1)
                key = f"grouped|{snps}x{indiv} {oname} span mb=1 dev n=8 {'T' if trans else 'N'} c=1"
                product(key, obj, snps, indiv, single, 8, trans, 1, True, kind="span")
                assert L.mxa_last_range_fallback(obj) == 1
                setenv(MXA_P_BUDGET_MB=None)
            assert most >= 3, (snps, indiv, most)                  # the product along the long dimension has several K splits to group
            free(obj)

    # ---- host pipeline: host B and C beyond the 32 MB threshold; n = 34 peels two columns ahead of it
    snps, indiv = PIPE
    d = make_big(snps, indiv)
    inputs[f"{snps}x{indiv} plink"], inputs[f"{snps}x{indiv} f"] = sha(d["plink"]), sha(d["f"])
    for single in (True, False):
        oname = "one-copy" if single else "two-copy"
        obj = create(d, snps, indiv, 40, single)
        for r in sweep("pipeline", oname + " host", obj, snps, indiv, single, PIPE_N, False, expect=True):
            assert r[0] == 0 and r[3] == 32, r
        free(obj)

    # ---- sharded object: two SNP blocks behind one handle on this device (virtual shards), host operands
    snps, indiv = VARIANTS
    d = make_inputs(snps, indiv, 0.02)
    obj = create(d, snps, indiv, 32, True, MIRACULIX_NUM_GPUS=2)
    assert L.mxa_num_shards(obj) == 2
    sweep("multi", "2 shards host", obj, snps, indiv, True, (5, 10), False, expect=None)
    free(obj)
    torch.cuda.synchronize()
    return dict(inputs=inputs, results=results), wrong


def collect(tmpdir):
    """the cases in one fresh child process, the environment switches cleared; returns its dict"""
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    path = os.path.join(tmpdir, "dgemm.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--emit", path], check=True, env=env, timeout=900)
    with open(path) as fh:
        return json.load(fh)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--emit":
        out, wrong = emit()
        with open(sys.argv[2], "w") as fh:
            json.dump(out, fh)
        assert not wrong, f"{len(wrong)} cases left their route (key, route, allowed paths, columns): {wrong[:20]}"
    else:
        import tempfile
        stamp = sys.argv[1] if len(sys.argv) > 1 else tree_id()
        if not stamp:
            sys.exit("this tree is no git checkout: name the commit it was exported from (make_golden_dgemm.py COMMIT)")
        with tempfile.TemporaryDirectory() as tmp:
            out = collect(tmp)
        out["recorded_at"] = stamp
        with open(GOLDEN, "w") as fh:
            json.dump(out, fh, indent=0, sort_keys=True)
            fh.write("\n")
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(out["results"]), "results")
