"""The Fortran interface blocks of the association scan (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by examples/fortran/assoc_check.f90:
mxa_assoc_basis and mxa_assoc_linear are called from Fortran on raw binary inputs, and the checksums it prints -- the exclusive or of the 64-bit patterns of
beta, se and t, which no order can change, the sum of nobs and dof -- must equal those of the same entries called from Python on the same seeded input.
Built by __graft_entry__.build() (make -C examples/fortran) where a Fortran compiler exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_ref as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "assoc_check.out")


def _xor(a):
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(a).view(np.uint64).ravel()))


def test_the_fortran_calls_give_the_checksums_of_the_python_entries(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, n, k = 301, 203, 2, 3
    codes, Y, W = ar.real_case(indiv, snps, n, k, seed=13)
    P = ar.pack(codes)
    yp = np.full((n, indiv + 2), np.nan)                          # ldy = indiv + 2: the rows behind a column are not read
    yp[:, :indiv] = Y.T
    for name, a in (("plink.bin", P), ("y.bin", yp), ("w.bin", W.T)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(n), str(k)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    got = re.search(r"beta ([0-9A-Fa-f]{16}) se ([0-9A-Fa-f]{16}) t ([0-9A-Fa-f]{16}) nobs (\d+) dof (\d+) PASS", p.stdout).groups()
    res = mx.assoc_linear(P, snps, indiv, Y, covariates=W)
    assert np.isfinite(res.t).all()
    want = (_xor(res.beta), _xor(res.se), _xor(res.t), int(res.nobs.sum()), res.dof)
    assert (int(got[0], 16), int(got[1], 16), int(got[2], 16), int(got[3]), int(got[4])) == want, (got, [hex(v) for v in want[:3]])
