"""mxa_assoc_score_firth without a device: the symbol in every layer, the argument errors of the entry (decided before a device is selected; the stand-alone
sanitizer program drives the same rules), the algebra of the header from first principles, and why the entry exists.

The algebra.  The header fits logit pi_i = logit p_i + beta g_i through the cumulant generating function K of the saddlepoint entry: log likelihood ratio
beta U - K(beta), no y.  Here y is rebuilt from the null residual (y = 1 where r > 0) and the penalised log likelihood
l*(beta) = sum [y log pi + (1 - y) log(1 - pi)] + (penalty / 2) log sum g^2 pi (1 - pi) is summed directly in float64: the long-double reference's beta^ must be
a local maximum of it, and its chisq must equal 2 (l*(beta^) - l*(0)).  The bound: a float64 sum of indiv terms is off by at most indiv 2^-53 sum |terms|
(every term's own rounding, a few 2^-53 of itself, is far below that); the difference of two such sums, doubled, by at most indiv 2^-52 (sum |terms| at beta^ +
sum |terms| at 0): ONE such unit is the bound.  Measured: at most 0.0032 units (259 individuals) and 0.0008 (1027); the references need at most 8 evaluations.

Why it is worth it.  (a) Intercept-only null, carriers exactly the cases: the unpenalised likelihood rises for ever (flag 2, no estimate), the penalised one has
a finite maximum.  (b) 1027 individuals, 5 % cases, MAF 0.01, true log odds ratio 1, 200 SNPs (seed 1): the penalised estimate is closer to the truth than
the one-step estimate U / V on 183 SNPs and than the maximum-likelihood estimate on 107 (on all 200 the latter exists); medians of |estimate - 1|: 0.44
(penalised), 0.50 (maximum likelihood), 1.02 (U / V); root mean squares 0.69, 1.37, 1.62.  Required against U / V, whose bias is of the order of the effect itself:
at least three quarters of the SNPs (150).  Against the maximum-likelihood estimate no majority is required: where it exists the two differ by its O(1 / n) bias,
which lies below the sampling error of a single SNP, so SNP by SNP the comparison is close to a coin (seeds 1 to 5 gave 107, 100, 102, 89, 103); what the
penalty buys there is the smaller error over the scan, and the penalised estimate must have the smallest median and the smallest root mean square error of the
three."""
import ctypes
import fnmatch
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_firth_ref as fr
import _assoc_spa_ref as sp
from _assoc_score_ref import score_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "mxa_assoc_score_firth"
WANT = ("const unsigned char * plink, int snps, int indiv, const double * P, long ldp, const double * R, long ldr, const double * Wt, long ldw, const double * H, "
        "long ldh, int n, int kh, double z_cutoff, int penalty, double tol, int max_iter, double * score, double * var, double * zstat, double * beta, double * se, "
        "double * chisq, double * pval, long ldo, int * flag, int * nobs")
LD = fr.LD


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


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
    block = re.search(r"function %s\((.*?)\)\s*bind\(C,\s*name='%s'\)" % (SYM, SYM), fortran, flags=re.S)
    assert block and re.search(r"\b%s\b" % SYM, public)
    assert len(re.sub(r"[&\s]", "", block.group(1)).split(",")) == len(proto)
    header = _read("include", "miraculix_amd.h")
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % SYM, header, flags=re.S).group(1)
    for phrase in ("2^-30 A", "no atomics", "MXA_ASSOC_SPA_BATCH", "MXA_ASSOC_SPA_ITEMS", "MXA_ASSOC_CHUNK_ROWS", "NOT promised bit-equal", "flag 2", "outputs untouched",
                   "penalty not 0 or 1", "K''''", "1 - 6 omega_i"):
        assert phrase in comment, phrase
    assert header.index("int mxa_assoc_score_spa(") < header.index(comment[:60]) < header.index("int %s(" % SYM)
    assert "wrapper's business" not in header.split("int mxa_assoc_score(")[0].split("Association scan for binary traits")[1]
    assert mx.assoc_score_firth is mx.assoc.assoc_score_firth
    assert mx.assoc.AssocFirthResult._fields == ("score", "var", "z", "beta", "se", "chisq", "pval", "flag", "nobs")
    assert "assoc_score_firth_args" in _read("miraculix_amd", "csrc", "mxa_assoc_host.h") and "hip/" not in _read("miraculix_amd", "csrc", "mxa_assoc_host.h")


def test_argument_errors_are_decided_before_a_device_is_selected(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n, kh = 5, 12, 2, 3
    X = np.zeros((snps, 3), np.uint8)
    Pm, R, Wt, H = np.full((n, indiv), 0.25), np.ones((n, indiv)), np.ones((n, indiv)), np.ones((n * kh, indiv))

    def run(plink=X, snps_=snps, indiv_=indiv, pm=Pm, ldp=indiv, r=R, ldr=indiv, wt=Wt, ldw=indiv, h=H, ldh=indiv, n_=n, kh_=kh, zc=2.0, penalty=1, tol=2.0 ** -30,
            max_iter=50, outs=(1, 1, 1), beta=True, ldo=snps):
        res = [np.full((n + 1, snps + 2), -7.5) for _ in range(7)]
        flag, nobs = np.full((n + 1, snps + 2), -3, np.int32), np.full(snps, -3, np.int32)
        rc = L.mxa_assoc_score_firth(p(plink), snps_, indiv_, p(pm), ldp, p(r), ldr, p(wt), ldw, p(h), ldh, n_, kh_, zc, penalty, tol, max_iter,
                                     *[p(a) if o else None for a, o in zip(res, tuple(outs) + (beta, 1, 1, 1))], ldo, p(flag), p(nobs))
        return rc, L.mxa_last_error(), all(bool(np.all(a == -7.5)) for a in res) and bool(np.all(flag == -3)) and bool(np.all(nobs == -3))

    big = 47453133
    score_errors = (dict(plink=None), dict(r=None), dict(wt=None), dict(snps_=0), dict(indiv_=0), dict(n_=0), dict(n_=-1), dict(kh_=-1), dict(h=None), dict(ldr=indiv - 1),
                    dict(ldw=indiv - 1), dict(ldh=indiv - 1), dict(ldo=snps - 1), dict(indiv_=big, ldp=big, ldr=big, ldw=big, ldh=big), dict(outs=(0, 0, 0)),
                    dict(n_=13108, kh_=3), dict(n_=1, kh_=65534))
    spa_errors = (dict(pm=None), dict(beta=False), dict(ldp=indiv - 1), dict(zc=-1e-300), dict(zc=-math.inf), dict(zc=math.nan), dict(tol=0.0), dict(tol=1.0), dict(tol=-0.5),
                  dict(tol=math.nan), dict(tol=math.inf), dict(max_iter=0), dict(max_iter=-3))
    own_errors = (dict(penalty=-1), dict(penalty=2), dict(penalty=2 ** 31 - 1), dict(penalty=-2 ** 31))
    for bad in score_errors + spa_errors + own_errors:
        assert run(**bad) == (1, 1, True), (bad, mx.lib.last_error())
        assert SYM in mx.lib.last_error()[1]
    for kw, words in ((dict(zc=math.nan), "z_cutoff"), (dict(tol=1.0), "tol"), (dict(max_iter=0), "max_iter"), (dict(pm=None), "P and beta"), (dict(beta=False), "P and beta"),
                      (dict(ldp=3), "ldp"), (dict(penalty=2), "penalty must be 0 or 1")):
        run(**kw)
        assert words in mx.lib.last_error()[1], (words, mx.lib.last_error())
    # valid calls pass the argument checks: they fail loudly for want of a device, or run where there is one -- never code 1, never a crash
    for kw in (dict(zc=math.inf), dict(zc=0.0), dict(h=None, kh_=0), dict(tol=0.5, max_iter=1), dict(penalty=0)):
        rc, code, untouched = run(**kw)
        assert code != 1 and (rc == 0) == (code == 0), mx.lib.last_error()
        assert rc == 0 or (untouched and mx.lib.last_error()[1]), mx.lib.last_error()


def test_the_stand_alone_sanitizer_program_passes(tmp_path):
    """tools/assoc_firth_host_check.cpp, compiled here for the CPU with the sanitizers' runtimes linked statically, so that the program is self-contained; run as a
    plain child process in the inherited environment"""
    exe = str(tmp_path / "assoc_firth_host_check")
    build = subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            os.path.join(ROOT, "tools", "assoc_firth_host_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("PASS"), run.stdout[-3000:]


def test_python_argument_checks_raise_before_any_library_call(mx, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(mx.lib, "check_library_handle", no_library)
    snps, indiv = 5, 12
    X, R, H = np.zeros((snps, 3), np.uint8), np.full((indiv, 2), 0.5), np.ones((indiv, 6))
    with pytest.raises(ValueError, match="wrong dimensions"):
        mx.assoc_score_firth(np.zeros((snps, 4), np.uint8), snps, indiv, R, R, R)
    with pytest.raises(ValueError, match="P needs"):
        mx.assoc_score_firth(X, snps, indiv, np.ones((indiv + 1, 2)), R, R)
    with pytest.raises(ValueError, match="as many columns as R"):
        mx.assoc_score_firth(X, snps, indiv, np.ones((indiv, 3)), R, R)
    for kw in (dict(z_cutoff=-1.0), dict(z_cutoff=math.nan), dict(tol=0.0), dict(tol=1.5), dict(max_iter=0), dict(penalty=2), dict(penalty=-1), dict(penalty=0.5)):
        with pytest.raises(ValueError, match="|".join(kw)):
            mx.assoc_score_firth(X, snps, indiv, R, R, R, H, **kw)
    F = lambda: np.zeros((snps, 2), order="F")          # noqa: E731
    for out in ({}, {"z": F()}, {"beta": F()}, {"beta": np.zeros((snps, 2)), "z": F()}, {"beta": F(), "t": F()}, {"beta": F(), "se": F(), "pval": F()}):
        with pytest.raises(ValueError, match="out"):
            mx.assoc_score_firth(X, snps, indiv, R, R, R, H, out=out)
    with pytest.raises(ValueError, match="exclude"):
        mx.assoc_logistic(X, snps, indiv, np.ones((indiv, 2)), spa=True, firth=True)
    with pytest.raises(ValueError, match="firth=True"):
        mx.assoc_logistic(X, snps, indiv, np.ones((indiv, 2)), penalty=0)


def _adjusted_genotypes(codes, R, Wt, H, T):
    """(g (snps, indiv), U (snps,)) of a one-trait case from the operands, as the references form them"""
    N, Sz, D, M, E = score_sums(codes, R, Wt, H, T)
    mu = Sz.astype(T) / N.astype(T)
    a = mu[:, None] * M + D
    tau = (H.astype(T) / Wt.astype(T)).T
    g = np.where(codes < 0, mu[:, None], np.maximum(codes, 0).astype(T))
    for j in range(H.shape[1]):
        g = g - a[:, 2 + j][:, None] * tau[j][None, :]
    return g, a[:, 0]


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("indiv, snps", [(259, 60), (1027, 40)])
def test_the_fit_maximises_the_penalised_likelihood_summed_directly_from_y(mx, indiv, snps, penalty):
    codes, _, Y, W, P, R, Wt, H = sp.null_operands(mx, indiv, snps, 1, 3, 3)
    y = (R[:, 0] > 0).astype(np.float64)
    assert np.array_equal(y, Y[:, 0]) and W.shape[1] == 2
    ref = fr.firth_reference(codes, P, R, Wt, H, 1.0, penalty, fr.TOL_LD, 200, LD)
    r64 = fr.firth_reference(codes, P, R, Wt, H, 1.0, penalty)
    assert np.array_equal(ref["flag"], r64["flag"]) and max(ref["evals"].max(), r64["evals"].max()) <= 20
    fitted = np.flatnonzero(ref["flag"][:, 0] == 1)
    assert len(fitted) >= 10
    g_all, U = _adjusted_genotypes(codes, R, Wt, H, LD)
    p = P[:, 0]
    worst = 0.0
    for s in fitted:
        g = g_all[s].astype(np.float64)
        assert abs(float(U[s] - (g_all[s] * R[:, 0]).sum())) <= indiv * 2.0 ** -52 * float(np.abs(g_all[s] * R[:, 0]).sum())      # U = g^T (y - p): C^T r = 0
        b = float(ref["beta"][s, 0])
        at, terms_at = fr.penalised_loglik(b, g, p, y, penalty)
        zero, terms_zero = fr.penalised_loglik(0.0, g, p, y, penalty)
        unit = indiv * 2.0 ** -52 * (terms_at + terms_zero)
        worst = max(worst, abs(2 * (at - zero) - float(ref["chisq"][s, 0])) / unit)
        assert abs(2 * (at - zero) - float(ref["chisq"][s, 0])) <= unit, s
        gl = g_all[s]
        top = fr.penalised_loglik(ref["beta"][s, 0], gl, p.astype(LD), y, penalty)[0]
        for h in (1e-2, 1e-4):                                   # a local maximum (long double: at 1e-4 the drop is some 1e-9 of a unit of l*)
            assert all(fr.penalised_loglik(ref["beta"][s, 0] * LD(f), gl, p.astype(LD), y, penalty)[0] < top for f in (1 - h, 1 + h)), (s, h)
    print(f"indiv {indiv} penalty {penalty}: {len(fitted)} fits, |2 (l*(beta^) - l*(0)) - chisq| <= {worst:.3g} units, evaluations <= {ref['evals'].max()}")


def test_separation_has_no_maximum_likelihood_estimate_and_a_finite_penalised_one():
    """intercept-only null (p = the case fraction, g = x - mean(x)), the carriers are exactly the cases"""
    for T, tol, cap in ((np.float64, 2.0 ** -30, 50), (LD, fr.TOL_LD, 200)):
        indiv, cases = 1027, 7
        y = np.zeros(indiv, T)
        y[:cases] = 1
        x = y.copy()
        x[2] = 2
        p = np.full(indiv, y.mean(), T)
        g = x - (x * p * (1 - p)).sum() / (p * (1 - p)).sum()
        U, V = (g * (y - p)).sum(), (g * g * p * (1 - p)).sum()
        z = U / np.sqrt(V)
        mle = fr.fit(g, p, U, 0, tol, cap, T)
        assert mle[0] == fr.OUTSIDE and abs(mle[6]) <= 2.0 ** -40 and z > 10
        assert fr.results_of_fit(mle, U, V, z, 0, T)[:2] == (2, U / V)
        pen = fr.fit(g, p, U, 1, tol, cap, T)
        flag, beta, se, chisq, pval = fr.results_of_fit(pen, U, V, z, 1, T)
        assert flag == 1 and pen[5] <= 20 and np.isfinite(beta) and beta > 1 and np.isfinite(se) and se > 0 and chisq > 20 and 0 < pval < 1e-5
        top = fr.penalised_loglik(beta, g, p, y, 1)[0]           # (with the null as a fixed offset the non-carriers, all controls, pull beta^ far out: some 340)
        assert all(fr.penalised_loglik(beta * T(f), g, p, y, 1)[0] < top for f in (0.5, 0.99, 1.01, 2.0))
        # without the support test Newton on the unpenalised score runs away: beta grows until the evaluations are used up or the bracket has no finite middle
        K1 = [fr.cgf4(T(b), g, p, (g * p).sum())[0] - U for b in (5, 10, 20, 40)]
        assert all(v < 0 for v in K1) and all(b > a for a, b in zip(K1, K1[1:]))


def test_the_penalised_estimate_is_closer_to_the_truth_than_the_one_step_and_the_maximum_likelihood_estimate():
    indiv, snps, fraction, maf, truth = 1027, 200, 0.05, 0.01, 1.0
    rng = np.random.default_rng([1, indiv])
    b0 = math.log(fraction / (1 - fraction))
    est = []
    while len(est) < snps:
        x = rng.binomial(2, maf, indiv).astype(np.float64)
        if x.sum() < 1:
            continue
        y = (rng.random(indiv) < 1 / (1 + np.exp(-(b0 + truth * x)))).astype(np.float64)
        if y.sum() < 2:
            continue
        p = np.full(indiv, y.mean())
        g = x - x.mean()
        U, V = float((g * (y - p)).sum()), float((g * g * p * (1 - p)).sum())
        fits = [fr.fit(g, p, U, penalty, 2.0 ** -30, 50, np.float64) for penalty in (1, 0)]
        assert fits[0][0] == fr.SOLVED and max(f[5] for f in fits) <= 20
        est.append((float(fits[0][1]), float(fits[1][1]) if fits[1][0] == fr.SOLVED else math.inf, U / V))
    err = np.abs(np.array(est) - truth)
    beats_mle, beats_one_step = int((err[:, 0] < err[:, 1]).sum()), int((err[:, 0] < err[:, 2]).sum())
    med, rms = np.median(err, axis=0), np.sqrt((err * err).mean(axis=0))
    print(f"{snps} SNPs: the penalised estimate is closer to {truth} than the maximum-likelihood estimate on {beats_mle}, than U / V on {beats_one_step}; "
          f"medians of |estimate - truth| {med[0]:.2f} (penalised), {med[1]:.2f} (maximum likelihood), {med[2]:.2f} (U / V), root mean squares {rms[0]:.2f}, {rms[1]:.2f}, "
          f"{rms[2]:.2f}")
    assert np.all(np.isfinite(err[:, 1])) and beats_one_step >= 3 * snps // 4 and med[0] < min(med[1:]) and rms[0] < min(rms[1:])
