"""The Fortran interface blocks of the LD operator object (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by examples/fortran/ld_op_check.f90:
mxa_ld_op_bytes, _create, _apply (n = 2, a shift), _solve and _free are called from Fortran on raw binary inputs, and the checksums it prints -- the exclusive
or of the 64-bit patterns of Y and of the solution, which no order can change -- and the iteration counts must equal those of the same entries called from
Python on the same seeded input.  Built by __graft_entry__.build() (make -C examples/fortran) where a Fortran compiler exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import _ld_ref as ref
from _util import make_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "ld_op_check.out")


def _xor(a):
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(a).view(np.uint64).ravel()))


def test_the_fortran_calls_give_the_checksums_of_the_python_entries(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, kind = 777, 203, 1
    prob = make_problem(snps, indiv, 1, seed=snps + indiv)
    X, f = prob["plink"], prob["f"]
    last = ref.sweep_window(snps, 3)
    xm = np.random.default_rng(8).standard_normal((snps, 2))
    xp = np.full((2, snps + 2), np.nan)                             # ldx = snps + 2: the rows behind a column are not read
    xp[:, :snps] = xm.T
    for name, a in (("plink.bin", X), ("f.bin", f), ("last.bin", last), ("x.bin", xp)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(kind)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    got = re.search(r"apply ([0-9A-Fa-f]{16}) solve ([0-9A-Fa-f]{16}) iters (\d+) (\d+) PASS", p.stdout).groups()
    with mx.crossproduct.LdOperator.create(X, snps, indiv, last=last, kind="r2", is_plink_format=True, allele_freq=f) as op:
        Y = op.apply(xm, shift=0.25)
        S, iters, relres, status = op.solve(xm, 2.0, tol=1e-10)
    assert np.isfinite(Y).all() and np.all(status == 0)
    assert (int(got[0], 16), int(got[1], 16), int(got[2]), int(got[3])) == (_xor(Y), _xor(S), int(iters[0]), int(iters[1])), (got, hex(_xor(Y)), hex(_xor(S)), iters)
