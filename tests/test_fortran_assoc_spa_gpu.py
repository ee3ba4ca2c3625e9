"""The Fortran interface block of mxa_assoc_score_spa (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by examples/fortran/assoc_spa_check.f90:
the null models and the scan with its saddlepoint correction are called from Fortran on raw binary inputs, and the checksums it prints -- the exclusive or of
the 64-bit patterns of score, z and pval, which no order can change, the sum of the flags, the number of corrected items and the sum of nobs -- must equal
those of the same entries called from Python on the same seeded input.  Built by __graft_entry__.build() (make -C examples/fortran) where a Fortran compiler
exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_spa_ref as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "assoc_spa_check.out")


def _xor(a):
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(a).view(np.uint64).ravel()))


def test_the_fortran_calls_give_the_checksums_of_the_python_entries(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, n, q, z_cutoff = 301, 203, 2, 3, 1.5
    codes, Y, W = sp.rare_case(indiv, snps, n, q, seed=13)
    P = sp.pack(codes)
    for name, a in (("plink.bin", P), ("y.bin", Y.T), ("w.bin", W.T)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(n), str(q), repr(z_cutoff)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    got = re.search(r"score ([0-9A-Fa-f]{16}) z ([0-9A-Fa-f]{16}) pval ([0-9A-Fa-f]{16}) flags (\d+) corrected (\d+) nobs (\d+) PASS", p.stdout).groups()
    res = mx.assoc_logistic(P, snps, indiv, Y, covariates=W, spa=True, z_cutoff=z_cutoff)
    assert np.isfinite(res.pval).all() and (res.flag == 1).sum() >= 20
    want = (_xor(res.score), _xor(res.z), _xor(res.pval), int(res.flag.sum()), int((res.flag == 1).sum()), int(res.nobs.sum()))
    assert (int(got[0], 16), int(got[1], 16), int(got[2], 16)) + tuple(int(g) for g in got[3:]) == want, (got, [hex(v) for v in want[:3]], want[3:])
