"""mxa_assoc_score / mxa_assoc_logistic_null without a device: the two symbols in every layer that names the C ABI, the argument errors of the scan (decided
before a device is selected), the errors and the accuracy of the host-only null model, the stand-alone sanitizer program, and the references of the GPU
tests (tests/_assoc_score_ref.py) checked against themselves.

Null-fit accuracy: gamma, r, w and H against a Newton iteration in np.longdouble run to a fixed point (the norm-wise relative error max |got - ref| /
max |ref| per array).  Largest value measured over all cases below, on an x86-64 CPU with an 80-bit long double: 1.0e-16 (gamma at indiv = 12, q = 1; the
results are long-double sums rounded once to double, so the error is that rounding).  Asserted at 8 x that = 8e-16, because the summation order may differ
between compilers; the cap 1e-9 is never approached.  Cases left out: indiv = 12 with q = 5 only, at both case fractions, raw and
through assoc_basis (six parameters on twelve individuals: the data are separated, the reference iteration itself does not reach a fixed point and the library
reports no convergence).  indiv = 12 at the case fraction 0.05 (a single case) stays in for q = 0 and q = 1: the reference converges there."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import _assoc_score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mxa_assoc_score", "mxa_assoc_logistic_null")
WANT = {"mxa_assoc_score": "const unsigned char * plink, int snps, int indiv, const double * R, long ldr, const double * Wt, long ldw, const double * H, long ldh, int n, "
                           "int kh, double * score, double * var, double * zstat, long ldo, int * nobs",
        "mxa_assoc_logistic_null": "int indiv, const double * y, const double * W, long ldw, int q, double tol, int max_iter, double * gamma, double * r, double * w, "
                                   "double * H, long ldh, int * iters"}
MEASURED_NULL_ERROR = 1.0e-16
NULL_TOLERANCE = 8 * MEASURED_NULL_ERROR
assert NULL_TOLERANCE <= 1e-9


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


def test_both_entries_are_in_every_layer_with_the_headers_prototypes(mx):
    fortran = _read("miraculix_amd", "bindings", "fortran", "modmiraculix_amd.f90")
    public = " ".join(re.findall(r"^\s*public\s*::(.*)$", fortran, flags=re.M))
    patterns = re.findall(r"([\w*]+)\s*;", re.sub(r"/\*.*?\*/", "", _read("miraculix_amd", "csrc", "exports.map"), flags=re.S).split("local:")[0])
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "miraculix_amd", "lib", "libmiraculix_amd.so")],
                                                                 text=True).splitlines() if ln.strip()}
    L = mx.lib.check_library_handle()
    scalar = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double}
    for sym in SYMBOLS:
        proto = _header_prototype(sym)
        assert ", ".join(f"{t} {n}" for t, n in proto) == WANT[sym], sym
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns) and sym in exported, sym
        fn = getattr(L, sym)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(proto), sym
        for (t, name), at in zip(proto, fn.argtypes):
            assert at is (ctypes.c_void_p if "*" in t else scalar[t]), (sym, name, t, at)
        assert re.search(r"bind\(C,\s*name='%s'\)" % sym, fortran) and re.search(r"\b%s\b" % sym, public), sym
    header = _read("include", "miraculix_amd.h")
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int mxa_assoc_score\(", header, flags=re.S).group(1)
    for phrase in ("fma(2.0, E_c, D_w)", "no atomics", "There is no special case", "MXA_ASSOC_CHUNK_ROWS", "NOT promised bit-identical"):
        assert phrase in comment, phrase
    # the comment stands behind the declaration of mxa_assoc_linear, not inside the comment in front of mxa_assoc_basis
    assert header.index("int mxa_assoc_linear(") < header.index(comment[:60]) < header.index("int mxa_assoc_score(")
    for name in ("assoc_score", "assoc_logistic_null", "assoc_logistic"):
        assert getattr(mx, name) is getattr(mx.assoc, name)
    for host in ("mxa_assoc_host.h", "mxa_assoc_null_host.h"):
        assert "hip/" not in _read("miraculix_amd", "csrc", host)          # the host-only parts compile without HIP
    assert "assoc_score_args" in _read("miraculix_amd", "csrc", "mxa_assoc_host.h") and "mxa_assoc_null_host.h" in _read("miraculix_amd", "csrc", "Makefile")


def test_score_argument_errors_decided_before_a_device_is_selected(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps, indiv, n, kh = 5, 12, 2, 3
    X = np.zeros((snps, 3), np.uint8)
    R, Wt, H = np.ones((n, indiv)), np.ones((n, indiv)), np.ones((n * kh, indiv))

    def run(plink=X, snps_=snps, indiv_=indiv, r=R, ldr=indiv, wt=Wt, ldw=indiv, h=H, ldh=indiv, n_=n, kh_=kh, outs=(1, 1, 1), ldo=snps):
        res = [np.full((n + 1, snps + 2), -7.5) for _ in range(3)]
        nobs = np.full(snps, -3, np.int32)
        rc = L.mxa_assoc_score(p(plink), snps_, indiv_, p(r), ldr, p(wt), ldw, p(h), ldh, n_, kh_, *[p(a) if o else None for a, o in zip(res, outs)], ldo, p(nobs))
        return rc, L.mxa_last_error(), all(bool(np.all(a == -7.5)) for a in res) and bool(np.all(nobs == -3))

    big = 47453133
    for bad in (dict(plink=None), dict(r=None), dict(wt=None), dict(snps_=0), dict(indiv_=0), dict(n_=0), dict(n_=-1), dict(kh_=-1), dict(h=None), dict(ldr=indiv - 1),
                dict(ldw=indiv - 1), dict(ldh=indiv - 1), dict(ldo=snps - 1), dict(indiv_=big, ldr=big, ldw=big, ldh=big), dict(outs=(0, 0, 0)),
                dict(n_=13108, kh_=3), dict(n_=1, kh_=65534)):
        assert run(**bad) == (1, 1, True), (bad, mx.lib.last_error())
    assert "65535" in mx.lib.last_error()[1]
    # a valid call (kh = 0 takes a NULL H) passes the argument checks: it fails loudly for want of a device, or runs where there is one -- never code 1, never a crash
    for kw in (dict(h=None, kh_=0), dict()):
        rc, code, untouched = run(**kw)
        assert code != 1 and (rc == 0) == (code == 0), mx.lib.last_error()
        assert rc == 0 or (untouched and mx.lib.last_error()[1]), mx.lib.last_error()


def test_null_model_errors_leave_the_outputs_untouched(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    indiv, q = 40, 2
    rng = np.random.default_rng(5)
    W = np.asfortranarray(rng.standard_normal((indiv, q)) + 3.0)
    y = (rng.random(indiv) < 0.5).astype(np.float64)
    y[:2] = (0.0, 1.0)

    def run(indiv_=indiv, y_=y, w=W, ldw=indiv, q_=q, max_iter=50, outs=(1, 1, 1, 1), ldh=indiv):
        gamma, r, wt, H = np.full(q + 2, -7.5), np.full(indiv + 1, -7.5), np.full(indiv + 1, -7.5), np.full((q + 2, indiv + 1), -7.5)
        iters = ctypes.c_int(-3)
        bufs = (gamma, r, wt, H)
        rc = L.mxa_assoc_logistic_null(indiv_, p(y_), p(w), ldw, q_, 1e-10, max_iter, *[p(b) if o else None for b, o in zip(bufs, outs)], ldh, ctypes.byref(iters))
        return rc, L.mxa_last_error(), all(bool(np.all(b == -7.5)) for b in bufs) and iters.value == -3

    half, nan_y, same = y.copy(), y.copy(), np.ones(indiv)
    half[7], nan_y[3] = 0.5, np.nan
    bad_nan, bad_inf, const, dup, sep = (W.copy(order="F") for _ in range(5))
    bad_nan[3, 1], bad_inf[0, 0] = np.nan, np.inf
    const[:, 1] = 4.25
    dup[:, 1] = 2.0 * dup[:, 0] + 3.0
    sep[:, 0] = y
    for bad in (dict(y_=None), dict(w=None), dict(outs=(0, 1, 1, 1)), dict(outs=(1, 0, 1, 1)), dict(outs=(1, 1, 0, 1)), dict(outs=(1, 1, 1, 0)), dict(indiv_=0),
                dict(q_=-1), dict(indiv_=3), dict(indiv_=2), dict(ldw=indiv - 1), dict(ldh=indiv - 1), dict(y_=half), dict(y_=nan_y), dict(y_=same),
                dict(y_=np.zeros(indiv)), dict(w=bad_nan), dict(w=bad_inf), dict(w=const), dict(w=dup), dict(w=sep), dict(max_iter=1)):
        assert run(**bad) == (1, 1, True), (bad, mx.lib.last_error())
    # the message names the cause and the column
    for kw, words in ((dict(y_=half), "y[7]"), (dict(w=bad_nan), "column 1 of W holds a non-finite"), (dict(w=const), "column 1 of W is constant or depends"),
                      (dict(w=dup), "column 1 of W is constant or depends"), (dict(y_=same), "all entries of y are equal"), (dict(w=sep), "no convergence")):
        run(**kw)
        assert words in mx.lib.last_error()[1], (words, mx.lib.last_error())
    with pytest.raises(RuntimeError, match="no convergence"):
        mx.assoc_logistic_null(y, sep)
    with pytest.raises(ValueError, match="covariates need to be"):
        mx.assoc_logistic_null(y, np.ones((indiv + 1, 2)))
    with pytest.raises(ValueError, match="exceed"):
        mx.assoc_logistic_null(y[:3], np.ones((3, 2)))
    assert run()[:2] == (0, 0) and run(w=None, q_=0)[:2] == (0, 0)          # ... and the valid calls pass (q = 0 takes a NULL W)


def _null_case(indiv, q, fraction, basis, mx):
    rng = np.random.default_rng([31, indiv, q, int(100 * fraction), int(basis)])
    W = rng.standard_normal((indiv, q)) * rng.uniform(0.5, 3, q) + rng.uniform(-3, 3, q) + 0.4 * rng.standard_normal((indiv, 1))
    eta = np.full(indiv, np.log(fraction / (1 - fraction)))
    if q:
        eta = eta + (W - W.mean(0)) @ (0.4 * rng.standard_normal(q)) / np.maximum(1.0, W.std(0)).mean()
    y = (rng.random(indiv) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    y[:2] = (1.0, 0.0)
    if basis and q:
        W = mx.assoc_basis(W)
    return y, np.asfortranarray(W)


NULL_CASES = [(indiv, q, fr, basis) for indiv in (12, 259, 4099) for q in (0, 1, 5) for fr in (0.5, 0.05) for basis in (False, True)
              if not (indiv == 12 and q == 5) and not (basis and q == 0)]


@pytest.mark.parametrize("indiv, q, fraction, basis", NULL_CASES)
def test_null_model_against_a_long_double_newton_iteration_at_its_fixed_point(mx, indiv, q, fraction, basis):
    y, W = _null_case(indiv, q, fraction, basis, mx)
    C = np.concatenate([np.ones((indiv, 1)), W], axis=1)
    ref = sr.newton_ld(y, C)
    fit = mx.assoc_logistic_null(y, W if q else None)
    assert 1 <= fit.iters <= 50 and fit.H.shape == (indiv, q + 1) and fit.H.flags.f_contiguous
    worst = 0.0
    for name, g, r in zip(("gamma", "r", "w", "H"), fit[:4], ref):
        diff, top = float(np.abs(g.astype(sr.LD) - r).max()), float(np.abs(r).max())
        err = diff / top if top > 0 else (0.0 if diff == 0 else np.inf)          # (an all-zero reference, gamma at ybar = 1/2 without covariates, is met exactly)
        print(f"indiv {indiv} q {q} fraction {fraction} basis {basis} {name}: relative error {err:.3g}")
        worst = max(worst, err)
        assert err <= NULL_TOLERANCE, (name, err)
    # what H stands for: C^T H = L is lower triangular with a positive diagonal, and L L^T = C^T diag(w) C
    CL, HL = C.astype(sr.LD), fit.H.astype(sr.LD)
    Lm = CL.T @ HL
    A = CL.T @ (fit.w.astype(sr.LD)[:, None] * CL)
    scale = np.sqrt(np.outer(np.diag(A), np.diag(A)))
    assert np.all(np.diag(Lm) > 0) and np.abs(np.triu(Lm, 1) / np.sqrt(np.diag(A))[:, None]).max(initial=0.0) <= 64 * indiv * sr.U
    assert (np.abs(Lm @ Lm.T - A) / scale).max() <= 64 * indiv * sr.U
    # leading dimensions larger than needed: the rows behind a column are neither read nor written
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    Wp, Hp = np.full((max(q, 1), indiv + 3), np.nan), np.full((q + 1, indiv + 2), -7.5)
    Wp[:q, :indiv] = W.T
    gamma, r, w = np.zeros(q + 1), np.zeros(indiv), np.zeros(indiv)
    assert L.mxa_assoc_logistic_null(indiv, p(y), p(Wp) if q else None, indiv + 3, q, 1e-10, 50, p(gamma), p(r), p(w), p(Hp), indiv + 2, None) == 0
    assert np.array_equal(Hp[:, :indiv].T, fit.H) and np.all(Hp[:, indiv:] == -7.5) and np.array_equal(gamma, fit.gamma) and np.array_equal(r, fit.r)


def test_the_stand_alone_sanitizer_program_passes(tmp_path):
    exe = str(tmp_path / "assoc_score_host_check")
    """compiled here for the CPU with the sanitizers' runtimes linked statically, so that the program is self-contained; run as a plain child process in the
    inherited environment"""
    build = subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            os.path.join(ROOT, "tools", "assoc_score_host_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("PASS"), run.stdout[-3000:]


def test_python_argument_checks_raise_before_any_library_call(mx, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(mx.lib, "check_library_handle", no_library)
    snps, indiv = 5, 12
    X, R, H = np.zeros((snps, 3), np.uint8), np.ones((indiv, 2)), np.ones((indiv, 6))
    with pytest.raises(ValueError, match="wrong dimensions"):
        mx.assoc_score(np.zeros((snps, 4), np.uint8), snps, indiv, R, R)
    with pytest.raises(ValueError, match="positive"):
        mx.assoc_score(X, 0, indiv, R, R)
    with pytest.raises(ValueError, match="R needs to be"):
        mx.assoc_score(X, snps, indiv, np.ones((indiv + 1, 2)), R)
    with pytest.raises(ValueError, match="as many columns"):
        mx.assoc_score(X, snps, indiv, R, np.ones((indiv, 3)))
    with pytest.raises(ValueError, match="n kh columns"):
        mx.assoc_score(X, snps, indiv, R, R, np.ones((indiv, 5)))
    for out in ({}, {"t": np.zeros((snps, 2), order="F")}, {"z": np.zeros((snps, 2))}, {"var": np.zeros((snps, 3), order="F")}):
        with pytest.raises(ValueError, match="out"):
            mx.assoc_score(X, snps, indiv, R, R, H, out=out)
    with pytest.raises(ValueError, match="Y needs to be"):
        mx.assoc_logistic(X, snps, indiv, np.ones((indiv + 1, 2)))


def test_the_exact_family_and_the_chain_are_what_they_claim():
    from fractions import Fraction
    for indiv, n, kh in ((19, 1, 1), (19, 2, 3), (67, 3, 4), (259, 1, 16), (259, 17, 2), (1027, 2, 17), (67, 2, 0)):
        R, Wt, H = sr.score_family(indiv, n, kh, seed=5)
        assert H.shape == (indiv, n * kh) and set(np.unique(Wt * 16)) <= {1.0, 2.0, 3.0, 4.0} and np.abs(H[indiv - 3:] * 16).max(initial=0) <= 2
        codes = sr.genotypes(9, indiv, seed=4)
        N, Sz, D, M, E = sr.score_sums(codes, R, Wt, H)
        _, _, Dr, Mr, Er = sr.score_sums(codes[:, ::-1], R[::-1], Wt[::-1], H[::-1])
        assert np.array_equal(D, Dr) and np.array_equal(M, Mr) and np.array_equal(E, Er)          # exact in two orders ...
        B = np.concatenate([R, Wt, H], axis=1)
        for s in (0, 3, 8):                                                                        # ... and against rational arithmetic
            for b in (0, n, B.shape[1] - 1):
                col = [Fraction(float(v)) for v in B[:, b]]
                assert Fraction(float(D[s, b])) == sum(c * int(max(g, 0)) for c, g in zip(col, codes[s]))
                assert Fraction(float(M[s, b])) == sum(c for c, g in zip(col, codes[s]) if g < 0)
            assert Fraction(float(E[s, 0])) == sum(Fraction(float(v)) for v, g in zip(Wt[:, 0], codes[s]) if g == 2)
        # sum w z^2 = sum w z + 2 sum_{z = 2} w
        z = np.where(codes < 0, 0, codes).astype(np.float64)
        assert np.array_equal((z * z) @ Wt, D[:, n:2 * n] + 2 * E)
        score, var, zs, nobs = sr.chain_score(codes, R, Wt, H)
        assert np.all(np.isnan(score[0])) and np.all(var[6:] > 0) and np.all(np.isfinite(zs[6:])) and nobs[0] == 0 and nobs[2] == indiv


@pytest.mark.parametrize("indiv", [67, 1027, 4099])
@pytest.mark.parametrize("n, q", [(1, 3), (4, 10)])
def test_a_float64_restatement_in_reversed_order_meets_the_bound_of_the_gpu_test(mx, indiv, n, q):
    """the bound of tests/test_assoc_score_gpu.py is one a correct implementation can meet (plain float64 numpy, the individuals summed in reversed order), and
    the library's H means what the header says: U^2 / V of the long-double reference equals the textbook form with an explicit (C^T W C)^-1 within it"""
    snps = 40
    codes, Y, W = sr.binary_case(indiv, snps, n, q, seed=21)
    fits = [mx.assoc_logistic_null(Y[:, c], W) for c in range(n)]
    R, Wt, H = (np.asfortranarray(np.concatenate([np.reshape(getattr(f, k), (indiv, -1)) for f in fits], axis=1)) for k in ("r", "w", "H"))
    (Uv, V, zv), (dU, dV, dz), sww = sr.bounded_score(codes, R, Wt, H)
    keep = V > 1e-6 * sww
    assert keep.mean() > 0.9 and 0.2 < Y.mean() < 0.6
    N, Sz, D, M, E = sr.score_sums(codes[:, ::-1], R[::-1], Wt[::-1], H[::-1])
    mu = (Sz / N)[:, None]
    a = mu * M + D
    kh = q + 1
    got_U = a[:, :n]
    got_V = D[:, n:2 * n] + 2 * E + mu * mu * M[:, n:2 * n] - np.stack([(a[:, 2 * n + c * kh: 2 * n + (c + 1) * kh] ** 2).sum(1) for c in range(n)], axis=1)
    for name, g, r, b in (("score", got_U, Uv, dU), ("var", got_V, V, dV), ("z", got_U / np.sqrt(got_V), zv, dz)):
        err = np.abs(g.astype(sr.LD) - r)[keep]
        print(f"indiv {indiv} n {n} q {q} {name}: max |err| / bound = {float((err / b[keep]).max()):.3g}")
        assert np.all(err <= 4 * b[keep]), name
    C = np.concatenate([np.ones((indiv, 1)), W], axis=1)
    for c in range(n):
        chi2 = sr.textbook_chi2(codes, Y[:, c], C, fits[c].gamma)
        ref = Uv[:, c] ** 2 / V[:, c]
        bound = 2 * np.abs(Uv[:, c]) * dU[:, c] / V[:, c] + ref * dV[:, c] / V[:, c]
        k = keep[:, c]
        assert np.all(np.abs(chi2 - ref)[k] <= 4 * bound[k]), float((np.abs(chi2 - ref)[k] / bound[k]).max())
