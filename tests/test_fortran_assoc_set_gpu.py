"""The Fortran interface blocks of mxa_assoc_set and mxa_assoc_skat_pvalue (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by
examples/fortran/assoc_set_check.f90: the null models, the set tests and the SKAT p-values are called from Fortran on raw binary inputs, and the checksums it
prints -- the exclusive or of the 64-bit patterns of stat, phi, the p-values and score, which no order can change, and the sum of nobs -- must equal those of the
same entries called from Python on the same seeded input.  Built by __graft_entry__.build() (make -C examples/fortran) where a Fortran compiler exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_spa_ref as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "assoc_set_check.out")


def _xor(a):
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(a).view(np.uint64).ravel()))


def test_the_fortran_calls_give_the_checksums_of_the_python_entries(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, n, q = 301, 203, 2, 3
    codes, Y, W = sp.rare_case(indiv, snps, n, q, seed=13)
    P = sp.pack(codes)
    rng = np.random.default_rng(5)
    sets = [np.arange(0, 20), rng.integers(0, snps, 37), np.array([300]), np.zeros(0, np.int64), np.arange(100, 117), np.array([8, 8, 3])]
    weights = [rng.uniform(0.5, 3.0, len(s)) for s in sets]
    ptr = np.zeros(len(sets) + 1, np.int64)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    idx, wt = np.concatenate(sets).astype(np.int32), np.concatenate(weights)
    for name, a in (("plink.bin", P), ("y.bin", Y.T), ("w.bin", W.T), ("setptr.bin", ptr), ("setidx.bin", idx), ("setwt.bin", wt)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(n), str(q), str(len(sets)), str(idx.size)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    got = re.search(" ".join(r"%s ([0-9A-Fa-f]{16})" % k for k in ("stat", "phi", "pval", "score")) + r" nobs (\d+) PASS", p.stdout).groups()
    out = dict(score=np.zeros((snps, n), order="F"), nobs=np.zeros(snps, np.int32))
    fits = [mx.assoc_logistic_null(Y[:, c], W) for c in range(n)]
    R = np.asfortranarray(np.stack([f.r for f in fits], axis=1))
    Wt = np.asfortranarray(np.stack([f.w for f in fits], axis=1))
    H = np.asfortranarray(np.concatenate([f.H for f in fits], axis=1))
    res = mx.assoc_set(P, snps, indiv, R, Wt, H, sets, weights, out=out, want_phi=True)
    live = res.c2 > 0
    assert np.isfinite(res.skat).all() and np.all((res.skat_p[live] > 0) & (res.skat_p[live] <= 1)) and int((~live).sum()) == n
    stat = np.stack([res.burden, res.burden_var, res.skat, res.c1, res.c2, res.c4])
    want = (_xor(stat), _xor(np.concatenate([b.ravel() for b in res.phi])), _xor(res.skat_p), _xor(out["score"]), int(out["nobs"].sum()))
    assert tuple(int(g, 16) for g in got[:4]) + (int(got[4]),) == want, (got, [hex(v) for v in want[:4]], want[4])
