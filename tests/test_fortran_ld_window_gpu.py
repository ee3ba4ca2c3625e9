"""The Fortran interface blocks of the windowed LD family (miraculix_amd/bindings/fortran/modmiraculix_amd.f90), exercised by examples/fortran/ld_window_check.f90:
mxa_ld_window_bounds and the eight device entries are called once each from Fortran on raw binary inputs, and every output file must equal, bit for bit, the
same entry called through ctypes; last / rowptr must equal the numpy restatement of the two-pointer sweep (tests/_ld_ref.py).  A wrong kind, order or `value`
attribute in an interface block shows here and nowhere else.  Built by __graft_entry__.build() (make -C examples/fortran) where a Fortran compiler exists."""
import os
import subprocess

import numpy as np
import pytest

import _ld_ref as ref
from _util import pack_plink, synth_genotypes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fortran", "ld_window_check.out")


def test_fortran_calls_give_the_bits_of_the_c_entries(tmp_path):
    if not os.path.exists(EXE):
        pytest.skip(f"{EXE} not built (make -C examples/fortran needs a Fortran compiler)")
    import miraculix_amd as mx
    mx.load_shared_library()
    snps, indiv, window, max_dist = 777, 203, 40, 25_000.0
    Z, miss = synth_genotypes(snps, indiv, seed=snps + indiv, missing_frac=0.05)
    X = np.ascontiguousarray(pack_plink(Z.T.copy()))
    Xm = np.ascontiguousarray(pack_plink(Z.T.copy(), miss.T.copy()))
    f = Z.astype(np.float64).mean(axis=0) / 2.0
    rng = np.random.default_rng(7)
    chrom = np.repeat(np.array([1, 2, 5], dtype=np.int32), [256, 300, snps - 556])            # three chromosomes, the first one ends on a tile edge
    pos = np.concatenate([np.cumsum(rng.integers(0, 2000, size=int(n))) for n in np.bincount(chrom)[[1, 2, 5]]]).astype(np.float64)
    for name, a in (("plink.bin", X), ("plink_missing.bin", Xm), ("f.bin", f), ("pos.bin", pos), ("chrom.bin", chrom)):
        a.tofile(str(tmp_path / name))
    p = subprocess.run([EXE, str(snps), str(indiv), str(window), repr(max_dist)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, text=True)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("PASS"), p.stdout[-3000:]
    got = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype=dtype)
    # the window: the numpy restatement, and the C entry through ctypes
    last, rowptr = ref.window_bounds(pos, chrom, max_dist)
    assert np.array_equal(got("last.bin", np.int32), last) and np.array_equal(got("rowptr.bin", np.int64), rowptr)
    cl, cr = mx.crossproduct.ld_window_bounds(pos, chrom, max_dist=max_dist)
    assert np.array_equal(cl, last) and np.array_equal(cr, rowptr)
    reach = last - np.arange(snps)
    assert reach.max() > 1 and reach.min() == 0 and last[255] == 255 and last[555] == 555 and f"{rowptr[-1]} stored entries" in p.stdout
    cp = mx.crossproduct
    want = {
        "band.bin": cp.ld_band(X, snps, indiv, window, is_plink_format=True, allele_freq=f),
        "scores.bin": cp.ld_scores(X, snps, indiv, window, adjust=True, is_plink_format=True, allele_freq=f),
        "band_pairwise.bin": cp.ld_band_pairwise(Xm, snps, indiv, window),
        "scores_pairwise.bin": cp.ld_scores_pairwise(Xm, snps, indiv, window, adjust=True),
        "rows.bin": cp.ld_window_rows(X, snps, indiv, last, is_plink_format=True, allele_freq=f),
        "wscores.bin": cp.ld_window_scores(X, snps, indiv, last, adjust=True, is_plink_format=True, allele_freq=f),
        "rows_pairwise.bin": cp.ld_window_rows_pairwise(Xm, snps, indiv, last),
        "wscores_pairwise.bin": cp.ld_window_scores_pairwise(Xm, snps, indiv, last, adjust=True),
    }
    for name, w in want.items():
        g = got(name, np.float64)
        assert np.isfinite(w).all() and g.shape == (w.size,) and np.array_equal(g, w.ravel()), name
