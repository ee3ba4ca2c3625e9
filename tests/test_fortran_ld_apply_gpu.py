"""The Fortran interface block of mxa_ld_window_apply (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by examples/fortran/ld_apply_check.f90:
the entry is called once from Fortran with n = 2 columns on raw binary inputs, and the checksum it prints -- the exclusive or of the 64-bit patterns of Y, which
no summation order can change -- must equal the checksum of the same entry called from Python on the same seeded input.  Built by __graft_entry__.build()
(make -C examples/fortran) where a Fortran compiler exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import _ld_ref as ref
from _util import make_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "ld_apply_check.out")


def test_the_fortran_call_gives_the_checksum_of_the_python_entry(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, term = 777, 203, 2
    prob = make_problem(snps, indiv, 1, seed=snps + indiv)
    X, f = prob["plink"], prob["f"]
    last = ref.sweep_window(snps, 3)
    xm = np.random.default_rng(8).standard_normal((snps, 2))
    xp = np.full((2, snps + 2), np.nan)                             # ldx = snps + 2: the rows behind a column are not read
    xp[:, :snps] = xm.T
    for name, a in (("plink.bin", X), ("f.bin", f), ("last.bin", last), ("x.bin", xp)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(term)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    got = int(re.search(r"checksum ([0-9A-Fa-f]{16}) PASS", p.stdout).group(1), 16)
    Y = mx.crossproduct.ld_window_apply(X, snps, indiv, xm, last=last, term="r2_adj", is_plink_format=True, allele_freq=f)
    assert np.isfinite(Y).all() and Y.shape == (snps, 2)
    want = int(np.bitwise_xor.reduce(np.ascontiguousarray(Y).view(np.uint64).ravel()))
    assert got == want, (hex(got), hex(want))
