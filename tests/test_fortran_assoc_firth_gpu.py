"""The Fortran interface block of mxa_assoc_score_firth (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by
examples/fortran/assoc_firth_check.f90: the null models and the scan with its fits are called from Fortran on raw binary inputs, and the checksums it prints --
the exclusive or of the 64-bit patterns of score, z, beta, se, chisq and pval, which no order can change, the sum of the flags, the number of fitted items and
the sum of nobs -- must equal those of the same entries called from Python on the same seeded input, for both penalties.  Built by __graft_entry__.build()
(make -C examples/fortran) where a Fortran compiler exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_spa_ref as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "assoc_firth_check.out")


def _xor(a):
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(a).view(np.uint64).ravel()))


@pytest.mark.parametrize("penalty", [0, 1])
def test_the_fortran_calls_give_the_checksums_of_the_python_entries(tmp_path, penalty):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, n, q, z_cutoff = 301, 203, 2, 3, 1.5
    codes, Y, W = sp.rare_case(indiv, snps, n, q, seed=13)
    P = sp.pack(codes)
    for name, a in (("plink.bin", P), ("y.bin", Y.T), ("w.bin", W.T)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(n), str(q), repr(z_cutoff), str(penalty)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    hexes = " ".join(r"%s ([0-9A-Fa-f]{16})" % k for k in ("score", "z", "beta", "se", "chisq", "pval"))
    got = re.search(hexes + r" flags (\d+) fitted (\d+) nobs (\d+) PASS", p.stdout).groups()
    res = mx.assoc_logistic(P, snps, indiv, Y, covariates=W, firth=True, z_cutoff=z_cutoff, penalty=penalty)
    assert np.isfinite(res.beta).all() and (res.flag == 1).sum() >= 20
    want = tuple(_xor(a) for a in (res.score, res.z, res.beta, res.se, res.chisq, res.pval)) + (int(res.flag.sum()), int((res.flag == 1).sum()), int(res.nobs.sum()))
    assert tuple(int(g, 16) for g in got[:6]) + tuple(int(g) for g in got[6:]) == want, (got, [hex(v) for v in want[:6]], want[6:])
