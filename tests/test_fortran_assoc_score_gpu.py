"""The Fortran interface blocks of the score test (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by examples/fortran/assoc_score_check.f90:
mxa_assoc_logistic_null and mxa_assoc_score are called from Fortran on raw binary inputs, and the checksums it prints -- the exclusive or of the 64-bit patterns
of score, var and z, which no order can change, the sum of nobs and the sum of the Newton steps -- must equal those of the same entries called from Python on the
same seeded input.  Built by __graft_entry__.build() (make -C examples/fortran) where a Fortran compiler exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_score_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "assoc_score_check.out")


def _xor(a):
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(a).view(np.uint64).ravel()))


def test_the_fortran_calls_give_the_checksums_of_the_python_entries(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, n, q = 301, 203, 2, 3
    codes, Y, W = sr.binary_case(indiv, snps, n, q, seed=13)
    P = sr.pack(codes)
    for name, a in (("plink.bin", P), ("y.bin", Y.T), ("w.bin", W.T)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(n), str(q)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    got = re.search(r"score ([0-9A-Fa-f]{16}) var ([0-9A-Fa-f]{16}) z ([0-9A-Fa-f]{16}) nobs (\d+) iters (\d+) PASS", p.stdout).groups()
    iters = sum(mx.assoc_logistic_null(Y[:, c], W).iters for c in range(n))
    res = mx.assoc_logistic(P, snps, indiv, Y, covariates=W)
    assert np.isfinite(res.z).all()
    want = (_xor(res.score), _xor(res.var), _xor(res.z), int(res.nobs.sum()), iters)
    assert (int(got[0], 16), int(got[1], 16), int(got[2], 16), int(got[3]), int(got[4])) == want, (got, [hex(v) for v in want[:3]])
