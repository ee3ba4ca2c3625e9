#!/usr/bin/env python3
"""Emit tests/golden/ld_window_digests.json: the sha256 of every result of the four windowed LD entries (mxa_ld_band, mxa_ld_scores, mxa_ld_band_pairwise,
mxa_ld_scores_pairwise) on small seeded inputs, as THIS library computes them on an MI355X.  The committed file was recorded at commit e43c170, before the
two copies of the window epilogue and the two host drivers became one: tests/test_ld_window_golden_gpu.py recomputes every case and compares, so that a change
of a single bit of a band entry or a score -- a summation order, a slot of the partial buffer, a window test -- is reported.  `recorded_at` in the file names
the tree that was run: the COMMIT argument, or `git rev-parse` of this checkout (marked -dirty with uncommitted changes); without either nothing is written.  The digests of the inputs are stored too and
asserted first (a numpy whose generator draws other numbers is then reported as such).  Fixtures are data only.

MXA_XPROD_GANG is read once per process, so the cases run in two child processes: `default` (every case) and `gang2` (MXA_XPROD_GANG=2, the cases of the
one shape whose band has at least 512 tiles, i.e. the gang-synchronised kernels).
usage: make_golden_ld_window.py [COMMIT]   write the golden file (needs the GPU); COMMIT: what a tree exported without its .git was exported from
       make_golden_ld_window.py --emit default|gang2 OUT.json    one child: its digests as JSON"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "ld_window_digests.json")
SENTINEL = -12345.678

# (snps, indiv): below one tile, not a multiple of 256, a multiple of 256; windows: 0, not a multiple of 256, a tile edge, snps - 1
SMALL = {(200, 131): (0, 100, 199), (777, 203): (0, 100, 256, 776), (1024, 160): (0, 300, 512, 1023)}
VARIANTS = (777, 203)                 # the shape that also runs device results, the raw format, a wide host band, the dense switch
GROUPS = (1024, 160)                  # ... and the scratch cap of 1 MiB: one tile row per group, four groups
GANG = ((35700, 200), 520)            # 140 tile rows x 4 diagonals - 6 = 554 band tiles >= 512: gang_order_tiles takes the list
ENGINES = (None, "i8")
MISSING = (0.0, 0.05, 0.3)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_inputs(snps, indiv, missing_frac):
    """dict(plink, raw: uint8 (snps, ceil(indiv / 4)); f: the allele frequencies of the complete data) from numpy.random.default_rng"""
    rng = np.random.default_rng([snps, indiv, int(round(100 * missing_frac))])
    p = rng.uniform(0.1, 0.9, snps)
    g = rng.binomial(2, p[:, None], size=(snps, indiv)).astype(np.uint8)
    assert (g.min(axis=1) < g.max(axis=1)).all()              # no constant SNP: every sigma is positive
    miss = rng.random((snps, indiv)) < missing_frac if missing_frac > 0 else np.zeros((snps, indiv), bool)
    code = np.where(miss, 1, np.array([0, 2, 3], np.uint8)[g]).astype(np.uint8)      # PLINK: 00, 10, 11; 01 = missing

    def pack(fields):
        pad = (-indiv) % 4
        x = np.pad(fields, ((0, 0), (0, pad))).reshape(snps, -1, 4)
        return np.ascontiguousarray(x[..., 0] | (x[..., 1] << 2) | (x[..., 2] << 4) | (x[..., 3] << 6)).astype(np.uint8)

    return dict(plink=pack(code), raw=pack(g), f=g.sum(axis=1, dtype=np.int64) / (2.0 * indiv))


def emit(mode):
    """every case of one child process: (digests of the inputs, digests of the results)"""
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

    def run(name, entry, X, snps, indiv, window, flag, device, extra, ldb_pad=0):
        """one call of a C entry; the result's bytes (a host band with ldb_pad > 0 keeps the sentinel beyond the window) -> results[name]"""
        scores = "scores" in entry
        shape = (snps,) if scores else (snps, window + 1 + ldb_pad)
        if device:
            Xa = torch.from_numpy(X).to(dev)
            out = torch.full(shape, SENTINEL, dtype=torch.float64, device=dev)
            extra = tuple(torch.from_numpy(e).to(dev) if isinstance(e, np.ndarray) else e for e in extra)
        else:
            Xa, out = X, np.full(shape, SENTINEL, dtype=np.float64)
        args = [P(Xa), snps, indiv, window, P(out)] + ([] if scores else [window + 1 + ldb_pad]) + [flag] + [P(e) if not isinstance(e, int) else e for e in extra]
        rc = getattr(L, entry)(*args)
        assert rc == 0, (name, mx.lib.last_error())
        if device:
            torch.cuda.synchronize()
            out = out.cpu().numpy()
        assert name not in results, name
        results[name] = sha(out)

    def plain(tag, X, f, fmt, snps, indiv, window, device, ldb_pad=0):
        for kind in (0, 1):
            run(f"{tag} band kind={kind}", "mxa_ld_band", X, snps, indiv, window, kind, device, (fmt, f), ldb_pad)
        if not ldb_pad:
            for adjust in (0, 1):
                run(f"{tag} scores adjust={adjust}", "mxa_ld_scores", X, snps, indiv, window, adjust, device, (fmt, f))

    def pairwise(tag, X, snps, indiv, window, device, ldb_pad=0):
        for kind in (0, 1):
            run(f"{tag} band kind={kind}", "mxa_ld_band_pairwise", X, snps, indiv, window, kind, device, (), ldb_pad)
        if not ldb_pad:
            for adjust in (0, 1):
                run(f"{tag} scores adjust={adjust}", "mxa_ld_scores_pairwise", X, snps, indiv, window, adjust, device, ())

    def data(snps, indiv, miss):
        d = make_inputs(snps, indiv, miss)
        for k, v in d.items():
            if miss == 0.0 or k == "plink":
                inputs[f"{snps}x{indiv} miss={miss} {k}"] = sha(v)
        return d

    if mode == "default":
        for (snps, indiv), windows in SMALL.items():
            for miss in MISSING:
                d = data(snps, indiv, miss)
                for window in windows:
                    for engine in ENGINES:
                        setenv("MXA_XPROD_ENGINE", engine)
                        base = f"{snps}x{indiv} w={window} engine={engine or 'default'}"
                        if miss == 0.0:
                            plain(f"plain {base} plink host", d["plink"], d["f"], 1, snps, indiv, window, False)
                            if (snps, indiv) == VARIANTS:
                                plain(f"plain {base} plink device", d["plink"], d["f"], 1, snps, indiv, window, True)
                                plain(f"plain {base} raw host", d["raw"], d["f"], 0, snps, indiv, window, False)
                                plain(f"plain {base} plink host ldb+3", d["plink"], d["f"], 1, snps, indiv, window, False, ldb_pad=3)
                        pw = f"pairwise {base} miss={miss}"
                        pairwise(f"{pw} host", d["plink"], snps, indiv, window, False)
                        if (snps, indiv) == VARIANTS:
                            if miss == 0.05:
                                pairwise(f"{pw} device", d["plink"], snps, indiv, window, True)
                                pairwise(f"{pw} host ldb+3", d["plink"], snps, indiv, window, False, ldb_pad=3)
                            if miss == 0.0:
                                setenv("MXA_LD_PAIRWISE_DENSE", "1")
                                pairwise(f"{pw} host dense=1", d["plink"], snps, indiv, window, False)
                                setenv("MXA_LD_PAIRWISE_DENSE", None)
                        if (snps, indiv) == GROUPS and miss != 0.3:
                            setenv("MXA_LD_PAIRWISE_SCRATCH_MB", "1")
                            pairwise(f"{pw} host scratch=1MiB", d["plink"], snps, indiv, window, False)
                            setenv("MXA_LD_PAIRWISE_SCRATCH_MB", None)
    # the shape with >= 512 band tiles, device results: classic kernels in the `default` child, the gang instantiations under MXA_XPROD_GANG=2
    (snps, indiv), window = GANG
    for miss in (0.0, 0.05):
        d = data(snps, indiv, miss)
        for engine in ENGINES:
            setenv("MXA_XPROD_ENGINE", engine)
            base = f"{snps}x{indiv} w={window} engine={engine or 'default'} gang={mode}"
            if miss == 0.0:
                plain(f"plain {base} plink device", d["plink"], d["f"], 1, snps, indiv, window, True)
            else:
                pairwise(f"pairwise {base} miss={miss} device", d["plink"], snps, indiv, window, True)
    return dict(inputs=inputs, results=results)


def run_child(mode, path):
    """a fresh process per setting of MXA_XPROD_GANG; returns its dict"""
    env = dict(os.environ)
    for k in ("MXA_XPROD_ENGINE", "MXA_XPROD_GANG", "MXA_LD_PAIRWISE_DENSE", "MXA_LD_PAIRWISE_SCRATCH_MB"):
        env.pop(k, None)
    if mode == "gang2":
        env["MXA_XPROD_GANG"] = "2"
    subprocess.run([sys.executable, os.path.abspath(__file__), "--emit", mode, path], check=True, env=env, timeout=900)
    with open(path) as fh:
        return json.load(fh)


def collect(tmpdir):
    inputs, results = {}, {}
    for mode in ("default", "gang2"):
        d = run_child(mode, os.path.join(tmpdir, f"ld_window_{mode}.json"))
        assert all(inputs.get(k, v) == v for k, v in d["inputs"].items())
        inputs.update(d["inputs"])
        assert not set(results) & set(d["results"])
        results.update(d["results"])
    return dict(inputs=inputs, results=results)


def tree_id():
    """the commit of this checkout, -dirty if it has uncommitted changes; None where git cannot tell"""
    git = lambda *a: subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True)
    if git("rev-parse", "--show-toplevel").stdout.strip() != os.path.realpath(ROOT):
        return None
    head, dirty = git("rev-parse", "--short", "HEAD"), git("status", "--porcelain", "--untracked-files=no")
    if head.returncode or dirty.returncode:
        return None
    return head.stdout.strip() + ("-dirty" if dirty.stdout.strip() else "")


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--emit":
        with open(sys.argv[3], "w") as fh:
            json.dump(emit(sys.argv[2]), fh)
    else:
        import tempfile
        stamp = sys.argv[1] if len(sys.argv) > 1 else tree_id()
        if not stamp:
            sys.exit("this tree is no git checkout: name the commit it was exported from (make_golden_ld_window.py COMMIT)")
        with tempfile.TemporaryDirectory() as tmp:
            out = collect(tmp)
        out["recorded_at"] = stamp
        with open(GOLDEN, "w") as fh:
            json.dump(out, fh, indent=0, sort_keys=True)
            fh.write("\n")
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(out["results"]), "results")
