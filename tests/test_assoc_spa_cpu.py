"""mxa_assoc_score_spa without a device: why the entry exists (the saddlepoint p-value against the exact one, beside the normal p-value), the two references of
tests/_assoc_spa_ref.py against each other, the argument errors of the entry (decided before a device is selected), and the symbol in every layer.

The exactness check.  No covariates and no projection (kh = 0, p_i = the case fraction of the sample), integer genotypes without missing calls: the null
distribution of U = sum x_i (y_i - p_i) is that of sum x_i y_i with independent Bernoulli y_i, enumerated by convolution.  indiv in {259, 1027}, case fractions
0.03 and 0.1, MAF from {0.01, 0.02, 0.05, 0.2}; the SNPs are drawn with the allele enriched among the cases by a factor from {1, 2, 3, 4} (a scan asks for
the significance of SNPs that carry a signal: under the global null hardly any SNP reaches the |z| where the two p-values part), and those with |z| >= 2
count.  Measured with the seeds below (reference in np.longdouble): indiv 259: the saddlepoint p-value is the closer one in |log ratio| on 262 of 284 SNPs
(92.3 %), median |log ratio| 0.60 against 1.56 for the normal p-value; indiv 1027: 415 of 437 (95.0 %), medians 0.52 against 2.85.  A run without the
enrichment (factor 1 only, 2000 SNPs per case fraction) gave 113 of 141 (80 %) and 73 of 134 (54 %): at |z| between 2 and 3 and 1027 individuals both
p-values sit inside the lattice error of an integer statistic (about e^0.5), and the comparison decides nothing."""
import ctypes
import fnmatch
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_spa_ref as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "mxa_assoc_score_spa"
WANT = ("const unsigned char * plink, int snps, int indiv, const double * P, long ldp, const double * R, long ldr, const double * Wt, long ldw, const double * H, "
        "long ldh, int n, int kh, double z_cutoff, double tol, int max_iter, double * score, double * var, double * zstat, double * pval, long ldo, int * flag, "
        "int * nobs")


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.mark.parametrize("indiv, per_fraction", [(259, 400), (1027, 400)])
def test_the_saddlepoint_p_value_is_closer_to_the_exact_one_than_the_normal_p_value(indiv, per_fraction):
    LD = sp.LD
    rng = np.random.default_rng([1, indiv])
    closer, err_spa, err_normal = 0, [], []
    for fraction in (0.03, 0.1):
        y = (rng.random(indiv) < fraction).astype(np.float64)
        y[:2] = 1.0
        p = np.full(indiv, y.mean())
        for s in range(per_fraction):
            maf, enrich = (0.01, 0.02, 0.05, 0.2)[s % 4], (1, 2, 3, 4)[(s // 4) % 4]
            x = rng.binomial(2, np.minimum(0.5, maf * np.where(y > 0, enrich, 1.0)))
            if not x.any():
                continue
            U, V = float((x * (y - p)).sum()), float((p * (1 - p) * x * x).sum())
            z = U / math.sqrt(V)
            if abs(z) < 2:
                continue
            flag, pval, _, _ = sp.spa_item(x.astype(LD), p.astype(LD), np.zeros((0, indiv), LD), np.zeros(0, LD), LD(U), LD(z), sp.TOL_LD, 200, LD)
            exact = sp.exact_two_sided(x, p, U)
            a, b = abs(math.log(float(pval) / exact)), abs(math.log(float(sp.normal_p(z)) / exact))
            assert flag in (1, 2) and exact > 0
            err_spa.append(a)
            err_normal.append(b)
            closer += a < b
    total = len(err_spa)
    print(f"indiv {indiv}: {total} SNPs with |z| >= 2, the saddlepoint p-value closer on {closer} ({100.0 * closer / total:.1f} %); median |log ratio| "
          f"{np.median(err_spa):.2f} (saddlepoint) against {np.median(err_normal):.2f} (normal)")
    assert total >= 150 and closer >= 0.9 * total


def test_the_exact_p_value_is_what_it_claims():
    """against the enumeration of all 2^k outcomes of the carriers"""
    import itertools
    rng = np.random.default_rng(8)
    x = np.array([0, 1, 2, 0, 1, 1, 2, 0, 2, 1])
    p = rng.uniform(0.05, 0.4, len(x))
    mean = float((x * p).sum())
    for U in (0.7, 2.3, mean, 6 - mean, 1e-12):
        want = 0.0
        for ys in itertools.product((0, 1), repeat=len(x)):
            pr = np.prod(np.where(np.array(ys) > 0, p, 1 - p))
            if abs(float((x * np.array(ys)).sum()) - mean) >= abs(U) - 1e-9:
                want += pr
        assert abs(sp.exact_two_sided(x, p, U) - want) <= 1e-14, U


@pytest.mark.parametrize("indiv, snps, n, kh, z_cutoff", [(67, 33, 1, 1, 1.0), (259, 130, 3, 3, 2.0), (259, 33, 1, 0, 1.0), (1027, 33, 3, 3, 1.0)])
def test_the_float64_and_the_long_double_reference_agree_on_every_flag(mx, indiv, snps, n, kh, z_cutoff):
    codes, _, Y, _, P, R, Wt, H = sp.null_operands(mx, indiv, snps, n, kh, 3)
    assert np.all((P > 0) & (P < 1)) and np.all(Wt > 0)
    p64, f64, z64, e64, _ = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, 2.0 ** -30, 50, np.float64)
    pld, fld, zld, eld, _ = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, sp.TOL_LD, 200, sp.LD)
    assert np.array_equal(f64, fld) and (f64 == 1).sum() >= 5 and max(e64.max(), eld.max()) <= 12
    eps = float(np.abs(np.log(p64.astype(sp.LD)) - np.log(pld)).max())
    print(f"indiv {indiv} snps {snps} n {n} kh {kh}: flags {np.bincount(f64.ravel(), minlength=4)}, eps {eps:.3g}")
    assert eps <= 2.0 ** -40
    # one evaluation solves nothing: every corrected item falls back to the normal p-value with the flag 2
    p1, f1, _, _, _ = sp.spa_reference(codes, P, R, Wt, H, z_cutoff, 2.0 ** -30, 1, np.float64)
    assert np.array_equal(f1, np.where(f64 == 1, 2, f64))
    assert all(p1[s, c] == sp.normal_p(z64[s, c]) for s, c in np.argwhere(f1 == 2))


def _header_prototype(sym):
    header = re.sub(r"/\*.*?\*/", "", _read("include", "miraculix_amd.h"), flags=re.S)
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % sym, header).group(1)
    out = []
    for a in args.split(","):
        t, name = re.match(r"\s*(.*?)(\w+)\s*$", a, flags=re.S).groups()
        out.append((" ".join(t.replace("*", " * ").split()), name))
    return out


def test_the_entry_is_in_every_layer_with_the_headers_prototype(mx):
    fortran = _read("miraculix_amd", "bindings", "fortran", "modmiraculix_amd.f90")
    public = " ".join(re.findall(r"^\s*public\s*::(.*)$", fortran, flags=re.M))
    patterns = re.findall(r"([\w*]+)\s*;", re.sub(r"/\*.*?\*/", "", _read("miraculix_amd", "csrc", "exports.map"), flags=re.S).split("local:")[0])
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "miraculix_amd", "lib", "libmiraculix_amd.so")],
                                                                 text=True).splitlines() if ln.strip()}
    proto = _header_prototype(SYM)
    assert ", ".join(f"{t} {n}" for t, n in proto) == WANT
    assert any(fnmatch.fnmatchcase(SYM, p) for p in patterns) and SYM in exported
    fn = getattr(mx.lib.check_library_handle(), SYM)
    scalar = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(proto)
    for (t, name), at in zip(proto, fn.argtypes):
        assert at is (ctypes.c_void_p if "*" in t else scalar[t]), (name, t, at)
    assert re.search(r"bind\(C,\s*name='%s'\)" % SYM, fortran) and re.search(r"\b%s\b" % SYM, public)
    header = _read("include", "miraculix_amd.h")
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % SYM, header, flags=re.S).group(1)
    for phrase in ("2^-30 A", "no atomics", "MXA_ASSOC_SPA_BATCH", "MXA_ASSOC_CHUNK_ROWS", "NOT promised bit-equal", "flag 2", "outputs untouched"):
        assert phrase in comment, phrase
    assert header.index("int mxa_assoc_logistic_null(") < header.index(comment[:60]) < header.index("int %s(" % SYM)
    assert mx.assoc_score_spa is mx.assoc.assoc_score_spa and mx.assoc.AssocSpaResult._fields == ("score", "var", "z", "pval", "flag", "nobs")
    assert "assoc_score_spa_args" in _read("miraculix_amd", "csrc", "mxa_assoc_host.h") and "hip/" not in _read("miraculix_amd", "csrc", "mxa_assoc_host.h")


def test_argument_errors_are_decided_before_a_device_is_selected(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n, kh = 5, 12, 2, 3
    X = np.zeros((snps, 3), np.uint8)
    Pm, R, Wt, H = np.full((n, indiv), 0.25), np.ones((n, indiv)), np.ones((n, indiv)), np.ones((n * kh, indiv))

    def run(plink=X, snps_=snps, indiv_=indiv, pm=Pm, ldp=indiv, r=R, ldr=indiv, wt=Wt, ldw=indiv, h=H, ldh=indiv, n_=n, kh_=kh, zc=2.0, tol=2.0 ** -30, max_iter=50,
            outs=(1, 1, 1), pv=True, ldo=snps):
        res = [np.full((n + 1, snps + 2), -7.5) for _ in range(4)]
        flag, nobs = np.full((n + 1, snps + 2), -3, np.int32), np.full(snps, -3, np.int32)
        rc = L.mxa_assoc_score_spa(p(plink), snps_, indiv_, p(pm), ldp, p(r), ldr, p(wt), ldw, p(h), ldh, n_, kh_, zc, tol, max_iter,
                                   *[p(a) if o else None for a, o in zip(res, tuple(outs) + (pv,))], ldo, p(flag), p(nobs))
        return rc, L.mxa_last_error(), all(bool(np.all(a == -7.5)) for a in res) and bool(np.all(flag == -3)) and bool(np.all(nobs == -3))

    big = 47453133
    score_errors = (dict(plink=None), dict(r=None), dict(wt=None), dict(snps_=0), dict(indiv_=0), dict(n_=0), dict(n_=-1), dict(kh_=-1), dict(h=None), dict(ldr=indiv - 1),
                    dict(ldw=indiv - 1), dict(ldh=indiv - 1), dict(ldo=snps - 1), dict(indiv_=big, ldp=big, ldr=big, ldw=big, ldh=big), dict(outs=(0, 0, 0)),
                    dict(n_=13108, kh_=3), dict(n_=1, kh_=65534))
    own_errors = (dict(pm=None), dict(pv=False), dict(ldp=indiv - 1), dict(zc=-1e-300), dict(zc=-math.inf), dict(zc=math.nan), dict(tol=0.0), dict(tol=1.0), dict(tol=-0.5),
                  dict(tol=math.nan), dict(tol=math.inf), dict(max_iter=0), dict(max_iter=-3))
    for bad in score_errors + own_errors:
        assert run(**bad) == (1, 1, True), (bad, mx.lib.last_error())
        assert SYM in mx.lib.last_error()[1]
    for kw, words in ((dict(zc=math.nan), "z_cutoff"), (dict(tol=1.0), "tol"), (dict(max_iter=0), "max_iter"), (dict(pm=None), "P and pval"), (dict(ldp=3), "ldp")):
        run(**kw)
        assert words in mx.lib.last_error()[1], (words, mx.lib.last_error())
    # valid calls (an infinite cutoff, a cutoff of zero, kh = 0 with a NULL H) pass the argument checks: they fail loudly for want of a device, or run where there
    # is one -- never code 1, never a crash
    for kw in (dict(zc=math.inf), dict(zc=0.0), dict(h=None, kh_=0), dict(tol=0.5, max_iter=1)):
        rc, code, untouched = run(**kw)
        assert code != 1 and (rc == 0) == (code == 0), mx.lib.last_error()
        assert rc == 0 or (untouched and mx.lib.last_error()[1]), mx.lib.last_error()


def test_python_argument_checks_raise_before_any_library_call(mx, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(mx.lib, "check_library_handle", no_library)
    snps, indiv = 5, 12
    X, R, H = np.zeros((snps, 3), np.uint8), np.full((indiv, 2), 0.5), np.ones((indiv, 6))
    with pytest.raises(ValueError, match="wrong dimensions"):
        mx.assoc_score_spa(np.zeros((snps, 4), np.uint8), snps, indiv, R, R, R)
    with pytest.raises(ValueError, match="P needs"):
        mx.assoc_score_spa(X, snps, indiv, np.ones((indiv + 1, 2)), R, R)
    with pytest.raises(ValueError, match="as many columns as R"):
        mx.assoc_score_spa(X, snps, indiv, np.ones((indiv, 3)), R, R)
    for kw in (dict(z_cutoff=-1.0), dict(z_cutoff=math.nan), dict(tol=0.0), dict(tol=1.5), dict(max_iter=0)):
        with pytest.raises(ValueError, match="|".join(kw)):
            mx.assoc_score_spa(X, snps, indiv, R, R, R, H, **kw)
    for out in ({}, {"z": np.zeros((snps, 2), order="F")}, {"pval": np.zeros((snps, 2), order="F")}, {"pval": np.zeros((snps, 2)), "z": np.zeros((snps, 2), order="F")},
                {"pval": np.zeros((snps, 2), order="F"), "t": np.zeros((snps, 2), order="F")}):
        with pytest.raises(ValueError, match="out"):
            mx.assoc_score_spa(X, snps, indiv, R, R, R, H, out=out)
    with pytest.raises(ValueError, match="spa=True"):
        mx.assoc_logistic(X, snps, indiv, np.ones((indiv, 2)), z_cutoff=3.0)
